"""Writes tests/golden/zstd_checksum_v1.json: what the checksum and stream tests read (tests/test_zstd_checksum_native.py,
tests/test_gpu_zstd_checksum.py through tests/zstd_checksum_inputs.py).

Run where libzstd.so.1 loads and the `xxhash` module imports: `python tests/golden/make_zstd_checksum_golden.py`. The tests
need neither: the file holds
  * XXH64 (xxhash) of pattern(length) from base offset `base` on, per (length, seed, base);
  * libzstd frames WITH a content checksum (ZSTD_c_checksumFlag) at levels 1 and 3 of contents that make_zstd_golden.py
    regenerates from their name, with the XXH64 of the content;
  * XXH64 of the contents the encoder tests compress.
While writing, libzstd is asked what the tests rely on: the flag sets descriptor bit 2, the last four bytes are the low
word of XXH64(content, 0), a flipped checksum byte and a flipped byte of a raw block are "doesn't match checksum", and
every stream of zstd_checksum_inputs.streams() gives what is recorded for it there.
"""
import base64
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import zstd_checksum_inputs as zi  # noqa: E402


def _golden():
    spec = importlib.util.spec_from_file_location("make_zstd_golden", os.path.join(HERE, "make_zstd_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import xxhash
    g = _golden()
    z = g.load_libzstd()
    assert z is not None, "libzstd.so.1 does not load here"
    out = {"version": 1, "xxh64": [], "frames": [], "contents": {}}
    for n in zi.XXH_LENGTHS:
        for seed in zi.XXH_SEEDS:
            for base in range(8):
                out["xxh64"].append([n, seed, base, "%016x" % xxhash.xxh64(zi.pattern(base + n)[base:], seed=seed).intdigest()])
    for name, length in zi.FRAME_CONTENTS:
        data = g.content_of(name, length)
        for level in (1, 3):
            frame = g.compress(z, data, level=level, checksum=True)
            low = xxhash.xxh64(data).intdigest() & 0xFFFFFFFF
            assert frame[4] & 4 and int.from_bytes(frame[-4:], "little") == low, name
            got, err = g.decompress(z, frame, length)
            assert err is None and got == data, name
            got, err = g.decompress(z, frame[:-1] + bytes([frame[-1] ^ 0x40]), length)
            assert got is None, name  # "Restored data doesn't match checksum"
            out["frames"].append({"name": "%s-level%d" % (name, level), "content": name, "length": length,
                                  "xxh64": "%016x" % xxhash.xxh64(data).intdigest(),
                                  "frame": base64.b64encode(frame).decode()})
    for name, n in zi.ENC_CONTENTS:
        out["contents"]["%s-%d" % (name, n)] = "%016x" % xxhash.xxh64(zi.enc_content(name, n)).intdigest()
    path = os.path.join(HERE, "zstd_checksum_v1.json")
    with open(path, "w") as f:  # one line per frame, the hashes on one line
        f.write('{"version": 1,\n"xxh64": %s,\n"contents": %s,\n"frames": [\n%s\n]}\n' % (
            json.dumps(out["xxh64"], separators=(",", ":")), json.dumps(out["contents"]),
            ",\n".join(json.dumps(fr) for fr in out["frames"])))
    zi._cache.clear()
    # what libzstd says to the derived cases the tests are built from
    for c in zi.flipped():
        got, err = g.decompress(z, c["frame"], c["length"])
        assert got is None, c["name"]
    for s in zi.streams():
        got, err = g.decompress(z, s["stream"], s["room"])
        if s["status"] == zi.OK:
            assert err is None and got == s["content"], s["name"]
        else:
            assert got is None, s["name"]
    print("%s: %d hashes, %d frames, %d bytes" % (os.path.basename(path), len(out["xxh64"]), len(out["frames"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
