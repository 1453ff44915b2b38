"""Writes tests/golden/zstd_enc_v1.json: per case of tests/zstd_enc_inputs.py the length and the SHA-256 of the frame that
the CPU build of pbs_plus_amd/csrc/zstd_encode.h writes (tests/native/test_zstd_encode.cpp, built and run here under
ASan + UBSan). tests/test_zstd_encode_native.py asserts that the CPU build still produces exactly these, and
tests/test_gpu_zstd_encode.py that the kernels do.

Run: `python tests/golden/make_zstd_enc_golden.py`. It needs g++ and nothing else.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zstd_enc_inputs  # noqa: E402


def main():
    code, out, err, frames, rows = zstd_enc_inputs.run_native()
    assert code == 0 and "zstd-encode-ok" in out, out[-4000:] + err[-4000:]
    cases = zstd_enc_inputs.cases()
    assert len(frames) == len(cases)
    table = {name: [len(f), hashlib.sha256(f).hexdigest()] for (name, _), f in zip(cases, frames)}
    with open(zstd_enc_inputs.GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in table.items()) + "\n}\n")
    print("%s: %d cases" % (os.path.basename(zstd_enc_inputs.GOLDEN), len(table)))


if __name__ == "__main__":
    main()
