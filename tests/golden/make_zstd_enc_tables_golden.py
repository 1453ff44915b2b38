"""Writes tests/golden/zstd_enc_tables_v1.json: per case of tests/zstd_enc_tables_inputs.py the length and the SHA-256 of
the frame that the CPU build of pbs_plus_amd/csrc/zstd_encode.h writes in the mode with per-block sequence tables and
repeat codes (tests/native/test_zstd_encode_tables.cpp, built and run here under ASan + UBSan).
tests/test_zstd_encode_tables_native.py asserts that the CPU build still produces exactly these, and
tests/test_gpu_zstd_encode_tables.py that the kernel does. The other mode's frames are those of zstd_enc_v1.json.

Run: `python tests/golden/make_zstd_enc_tables_golden.py`. It needs g++ and nothing else.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zstd_enc_tables_inputs as ti  # noqa: E402


def main():
    code, out, err, frames, rows = ti.run_native()
    assert code == 0 and "zstd-encode-tables-ok" in out, out[-4000:] + err[-4000:]
    cases = ti.cases()
    assert len(frames[1]) == len(cases)
    table = {name: [len(f), hashlib.sha256(f).hexdigest()] for (name, _), f in zip(cases, frames[1])}
    with open(ti.GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in table.items()) + "\n}\n")
    print("%s: %d cases" % (os.path.basename(ti.GOLDEN), len(table)))


if __name__ == "__main__":
    main()
