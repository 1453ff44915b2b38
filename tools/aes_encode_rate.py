"""Rate of writing encrypted blobs on the device (pbsgpu_blob_encode3_device), in GB/s of chunk bytes, beside what it is
measured against in the same run:

* the three-step sequence it replaces: aes_gcm_many(encrypt) straight into the blobs' layout, crc32_many over the
  ciphertexts, and the 44-byte headers assembled on the host (one numpy array of n x 44 bytes; NOT uploaded: a caller may
  send header and payload from two places, so the sequence is given that for free);
* blob_encode of the same chunks: what framing costs when nothing is encrypted;
* blob_encode3 with F_AES | F_ZSTD beside blob_encode2 with F_ZSTD: what encryption adds to the compressing encoder.

The chunks: `--chunks` of seeded sizes between 64 KiB and 4 MiB (4 096 by default, about 8 GiB; tools/aes_rate.py's), filled
on the device. Each figure is the median of `--reps` synchronous calls timed with a host clock after one warm-up call, with
the fastest and the slowest beside it: the spread is what a difference has to be read against. The new call's blobs are
compared with the sequence's on the first, a middle and the last chunk. Prints one JSON line.

    python tools/aes_encode_rate.py [--chunks 4096] [--reps 5] [--no-zstd]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _spread(fn, reps):
    """[fastest, median, slowest] of reps calls after one warm-up, in seconds"""
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), statistics.median(ts), max(ts)


def _put(res, name, total, ts):
    res[name + "_ms"] = [round(t * 1e3, 3) for t in ts]
    res[name + "_GBps"] = round(total / ts[1] / 1e9, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-zstd", action="store_true", help="leave the two compressing calls out")
    a = ap.parse_args()
    import aes_inputs as ai
    from pbs_plus_amd import AesKey, Engine, blob_magic, buzhash

    rng = np.random.default_rng(4096)
    sizes = rng.integers(64 << 10, (4 << 20) + 1, a.chunks).astype(np.uint64)
    ends = np.cumsum(sizes)
    segs = np.stack([ends - sizes, sizes], axis=1)
    total = int(ends[-1])
    ivs = np.frombuffer(ai.pattern(16 * a.chunks, 9002), np.uint8).reshape(-1, 16)
    eng = Engine(buzhash.NewConfig(4 << 20), device=0)
    key = AesKey(eng, ai.pattern(32, 9001))
    blens = sizes + np.uint64(44)
    boffs = np.cumsum(blens) - blens
    where = np.stack([boffs + np.uint64(44), sizes], axis=1)
    plain, blobs, steps = eng.alloc(total), eng.alloc(int(blens.sum())), eng.alloc(int(blens.sum()))
    eng.fill(plain.ptr, total, 7, 0)
    res = {"chunks": a.chunks, "payload_bytes": total, "reps": a.reps}

    def encode3(zstd):
        return eng.blob_encode3(plain, segs, key=key, ivs=ivs, dst=blobs, zstd=zstd)

    magic = np.frombuffer(blob_magic(2), np.uint8)
    heads = np.empty((a.chunks, 44), np.uint8)

    def three_steps():
        _, status, tags, _ = eng.aes_gcm_many(key, plain, segs, ivs, out=where, dst=steps, encrypt=True)
        crcs = eng.crc32_many(steps, where)
        heads[:, :8] = magic
        heads[:, 8:12] = crcs.astype("<u4").view(np.uint8).reshape(-1, 4)
        heads[:, 12:28] = ivs
        heads[:, 28:44] = tags
        return status, crcs

    _, offs, lens, kinds, crcs, st, _ = encode3(False)
    status, crcs3 = three_steps()
    assert not status.any() and np.array_equal(offs[:-1], boffs) and np.array_equal(lens, blens) and np.all(kinds == 2)
    assert np.array_equal(crcs, crcs3) and st["aes_bytes"] == total
    for i in (0, a.chunks // 2, a.chunks - 1):  # the same blob either way
        o, n = int(boffs[i]), int(blens[i])
        got = blobs.download(o, n)
        assert np.array_equal(got[:44], heads[i]) and np.array_equal(got[44:], steps.download(o + 44, n - 44)), i
    _put(res, "blob_encode3_aes", total, _spread(lambda: encode3(False), a.reps))
    _put(res, "three_steps", total, _spread(three_steps, a.reps))
    _put(res, "three_steps_cipher_only", total, _spread(lambda: eng.aes_gcm_many(key, plain, segs, ivs, out=where, dst=steps, encrypt=True), a.reps))
    _put(res, "three_steps_crc_only", total, _spread(lambda: eng.crc32_many(steps, where), a.reps))

    def plain_encode():
        old, _, _ = eng.blob_encode(plain, segs)
        old.free()

    # (blob_encode allocates its own buffer: the figure holds one allocation and one release per call)
    _put(res, "blob_encode_plain", total, _spread(plain_encode, a.reps))
    _put(res, "blob_encode2_plain", total, _spread(lambda: eng.blob_encode2(plain, segs, dst=steps, zstd=False), a.reps))
    if not a.no_zstd:
        _, _, lens_z, kinds_z, _, st_z, _ = encode3(True)
        _, _, lens_2, kinds_2, _, st_2 = eng.blob_encode2(plain, segs, dst=steps, zstd=True)
        assert np.array_equal(kinds_z, kinds_2 + 2) and np.array_equal(lens_z, lens_2 + 32)  # the same verdicts, the same frames
        res["compressed_blobs"] = int(st_z["blobs"][3])
        _put(res, "blob_encode3_aes_zstd", total, _spread(lambda: encode3(True), a.reps))
        _put(res, "blob_encode2_zstd", total, _spread(lambda: eng.blob_encode2(plain, segs, dst=steps, zstd=True), a.reps))
    print(json.dumps(res), flush=True)
    key.close()
    for b in (plain, blobs, steps):
        b.free()
    eng.close()


if __name__ == "__main__":
    main()
