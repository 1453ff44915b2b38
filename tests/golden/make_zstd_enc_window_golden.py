"""Writes tests/golden/zstd_enc_window_v1.json: per case of tests/zstd_enc_window_inputs.py and per window mode (window
log 17 and 19, without and with per-block sequence tables) the length and the SHA-256 of the frame that the CPU build of
pbs_plus_amd/csrc/zstd_encode.h writes with the long-range match finder (tests/native/test_zstd_encode_window.cpp, built
and run here under ASan + UBSan). tests/test_zstd_encode_window_native.py asserts that the CPU build still produces
exactly these, and tests/test_gpu_zstd_encode_window.py that the kernels do. The frames of window 0 are those of
zstd_enc_v1.json and zstd_enc_tables_v1.json.

Run: `python tests/golden/make_zstd_enc_window_golden.py`. It needs g++ and nothing else.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zstd_enc_window_inputs as wi  # noqa: E402


def main():
    code, out, err, frames, rows = wi.run_native()
    assert code == 0 and "zstd-encode-window-ok" in out, out[-4000:] + err[-4000:]
    cases = wi.cases()
    table = {}
    for i, (name, _) in enumerate(cases):
        table[name] = {wi.KEY[m]: [len(frames[m][i]), hashlib.sha256(frames[m][i]).hexdigest()] for m in wi.WINDOW_MODES}
    with open(wi.GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in table.items()) + "\n}\n")
    print("%s: %d cases" % (os.path.basename(wi.GOLDEN), len(table)))


if __name__ == "__main__":
    main()
