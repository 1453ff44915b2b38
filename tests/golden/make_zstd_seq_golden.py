"""Writes tests/golden/zstd_seq_v1.json: per case of tests/zstd_seq_inputs.py the frame's length and SHA-256, the content's
length and SHA-256 and the status a decoder must report.

Run on a machine where libzstd.so.1 loads: `python tests/golden/make_zstd_seq_golden.py`. Every case is regenerated and set
against libzstd first: an OK frame must decode there to exactly execute()'s bytes, a BAD_FRAME one must be refused. The
tests regenerate the frames and compare them with the file; they never need libzstd."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zstd_inputs  # noqa: E402
import zstd_seq_inputs  # noqa: E402

PATH = os.path.join(HERE, "zstd_seq_v1.json")


def rows(cases):
    return [{"name": c["name"], "status": c["status"], "frame_length": len(c["frame"]), "frame_sha256": hashlib.sha256(c["frame"]).hexdigest(),
             "length": c["length"], "sha256": c["sha256"].hex()} for c in cases]


def main():
    g = zstd_inputs.golden()
    z = g.load_libzstd()
    assert z is not None, "libzstd.so.1 does not load here"
    cases = zstd_seq_inputs.cases()
    for c in cases:
        got, err = g.decompress(z, c["frame"], max(c["length"], 64 << 10))
        if c["status"] == zstd_seq_inputs.OK:
            assert err is None and got == c["content"], c["name"]
        else:
            assert c["status"] == zstd_seq_inputs.BAD_FRAME and got is None, c["name"]
    with open(PATH, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows(cases)) + "\n]\n")
    print("%s: %d cases, %d bytes" % (os.path.basename(PATH), len(cases), os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
