"""Writes tests/golden/zstd_huf_v1.json: per case of tests/zstd_huf_inputs.py the frame's length and SHA-256, the content's
length and SHA-256, the status a decoder must report, and what libzstd made of the frame ("same": the same bytes,
"error": refused).

Run on a machine where libzstd.so.1 loads: `python tests/golden/make_zstd_huf_golden.py`. Every case is regenerated and set
against libzstd first: what libzstd decodes must be OK here with exactly the expected bytes, and what is refused here
must be refused there. The only cases that are OK here and an error there are those that zstd_huf_inputs.ok_here_only
names: codes of 12 bits and fewer spare bits than the table is deep. The tests regenerate the frames and
compare them with the file; they need libzstd only for the last column."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zstd_huf_inputs  # noqa: E402
import zstd_inputs  # noqa: E402

PATH = os.path.join(HERE, "zstd_huf_v1.json")


def rows(cases, z=None):
    """the file's rows; with libzstd (z) the column "libzstd" too, checked against the expectation"""
    g = zstd_inputs.golden()
    out = []
    for c in cases:
        r = {"name": c["name"], "status": c["status"], "frame_length": len(c["frame"]), "frame_sha256": hashlib.sha256(c["frame"]).hexdigest(),
             "length": c["length"], "sha256": c["sha256"].hex()}
        if z is not None:
            got, err = g.decompress(z, c["frame"], max(c["length"], 64 << 10))
            if got is not None:  # nothing that libzstd accepts is refused here or decodes to other bytes
                assert c["status"] == zstd_huf_inputs.OK and got == c["content"], c["name"]
            else:
                assert c["status"] == zstd_huf_inputs.BAD_FRAME or zstd_huf_inputs.ok_here_only(c["name"]), c["name"]
            assert (got is None) == (c["status"] != zstd_huf_inputs.OK or zstd_huf_inputs.ok_here_only(c["name"])), c["name"]
            r["libzstd"] = "error" if got is None else "same"
        out.append(r)
    return out


def main():
    z = zstd_inputs.golden().load_libzstd()
    assert z is not None, "libzstd.so.1 does not load here"
    cases = zstd_huf_inputs.cases()
    with open(PATH, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows(cases, z)) + "\n]\n")
    print("%s: %d cases, %d bytes" % (os.path.basename(PATH), len(cases), os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
