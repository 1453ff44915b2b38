"""Rate of the restore with zstd-compressed chunks decoded on the device (pbsgpu_blob_decode2_device with F_ZSTD), in GB/s
of DECODED bytes, beside what it is measured against:

* blob_decode of the same chunks stored uncompressed (what the restore could do before it could decode);
* ZSTD_decompress of the same frames on 16 host threads, where libzstd.so.1 loads (ctypes releases the GIL).

And, on the same chunks compressed WITH a content checksum, the stand-alone calls: pbsgpu_zstd_decode_device, which
verifies nothing, pbsgpu_zstd_decode2_device without flags (the same work by promise) and with F_CHECKSUM (XXH64 of every
frame's output inside its wave), and pbsgpu_xxh64_many_device over the decoded chunks alone. For these the fastest and
the slowest call are printed beside the median: the spread is what a difference has to be read against.

Two batches, NewConfig(4 << 20)'s and NewConfig(4096)'s chunk sizes (fixed 4 MiB and 4 KiB chunks), each on data of two
compressibilities (words over a small alphabet; skewed bytes over 220 values). The chunks are cut from an 8 MiB pool at
scattered offsets and compressed here at level 3, the stock client's default, so the tool needs libzstd where it runs.
Each figure is the median of a few synchronous calls timed with a host clock, after one warm-up call. Not measured: the
share of the serial sequence lane (it needs a kernel variant, not a clock around the call).

    python tools/zstd_rate.py [--big 64] [--small 4096] [--reps 5]
"""
import argparse
import ctypes as C
import hashlib
import importlib.util
import json
import os
import statistics
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MAGIC_PLAIN = hashlib.sha256(b"Proxmox Backup uncompressed blob v1.0").digest()[:8]
MAGIC_ZSTD = hashlib.sha256(b"Proxmox Backup zstd compressed blob v1.0").digest()[:8]


def _median_s(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def _spread_ms(fn, reps):
    """[fastest, median, slowest] of reps calls after one warm-up, in ms"""
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return [round(v * 1e3, 3) for v in (min(ts), statistics.median(ts), max(ts))]


def _golden():
    spec = importlib.util.spec_from_file_location("make_zstd_golden", os.path.join(ROOT, "tests", "golden", "make_zstd_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", type=int, default=64, help="number of 4 MiB chunks")
    ap.add_argument("--small", type=int, default=4096, help="number of 4 KiB chunks")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    g = _golden()
    z = g.load_libzstd()
    if z is None:
        sys.exit("libzstd.so.1 does not load here: the tool compresses its chunks itself")
    from pbs_plus_amd import RECORD_DTYPE, Engine, buzhash

    eng = Engine(buzhash.NewConfig(4 << 20), device=0)
    pools = {"words": g._text_few(8 << 20, 31), "skewed": g._text_many(8 << 20, 32)}
    pool16 = ThreadPoolExecutor(16)
    for kind, pool in pools.items():
        for label, size, count in (("4MiB", 4 << 20, a.big), ("4KiB", 4096, a.small)):
            offs = [(i * 977_003) % (len(pool) - size) for i in range(count)]
            chunks = [pool[o:o + size] for o in offs]
            frames = list(pool16.map(lambda c: g.compress(z, c, level=3), chunks))
            idx = np.zeros(count, dtype=RECORD_DTYPE)
            idx["size"] = size
            idx["end"] = np.cumsum(np.full(count, size, dtype=np.uint64))
            idx["digest"] = [np.frombuffer(hashlib.sha256(c).digest(), np.uint8) for c in chunks]
            total = size * count
            res = {"data": kind, "chunks": label, "count": count, "decoded_bytes": total, "frame_bytes": sum(map(len, frames))}
            dst = eng.alloc(total)
            for name, magic, bodies in (("zstd", MAGIC_ZSTD, frames), ("plain", MAGIC_PLAIN, chunks)):
                blob = b"".join(magic + zlib.crc32(b).to_bytes(4, "little") + b for b in bodies)
                lens = np.array([12 + len(b) for b in bodies], dtype=np.uint64)
                ranges = np.stack([np.cumsum(lens) - lens, lens], axis=1)
                dev = eng.alloc(len(blob))
                dev.upload(np.frombuffer(blob, np.uint8))
                for digest in (False, True):
                    if name == "zstd":
                        fn = lambda: eng.blob_decode2(dev, ranges, idx, None, None, None, digest, dst=dst, zstd=True)  # noqa: E731
                    else:
                        fn = lambda: eng.blob_decode(dev, ranges, idx, None, None, None, digest, dst=dst)  # noqa: E731
                    _, status, st = fn()
                    assert not status.any(), (name, np.flatnonzero(status)[:4], status[status != 0][:4])
                    t = _median_s(fn, a.reps)
                    res["%s_%s_ms" % (name, "digest" if digest else "nodigest")] = round(t * 1e3, 3)
                    res["%s_%s_GBps" % (name, "digest" if digest else "nodigest")] = round(total / t / 1e9, 2)
                dev.free()
            # the stand-alone calls, on frames that carry a checksum
            summed = list(pool16.map(lambda c: g.compress(z, c, level=3, checksum=True), chunks))
            lens = np.array([len(f) for f in summed], dtype=np.uint64)
            fr = np.stack([np.cumsum(lens) - lens, lens], axis=1)
            out = np.stack([np.arange(count, dtype=np.uint64) * size, np.full(count, size, dtype=np.uint64)], axis=1)
            dev = eng.alloc(int(lens.sum()))
            dev.upload(np.frombuffer(b"".join(summed), np.uint8))
            for name, fn in (("decode", lambda: eng.zstd_decode(dev, fr, out=out, dst=dst)),
                             ("decode2", lambda: eng.zstd_decode2(dev, fr, out=out, dst=dst)),
                             ("decode2_checksum", lambda: eng.zstd_decode2(dev, fr, out=out, dst=dst, checksum=True))):
                assert not fn()[1].any(), name
                ms = _spread_ms(fn, a.reps)
                res[name + "_ms"] = ms
                res[name + "_GBps"] = round(total / ms[1] / 1e6, 2)
            ms = _spread_ms(lambda: eng.xxh64_many(dst, out), a.reps)
            res["xxh64_many_ms"] = ms
            res["xxh64_many_GBps"] = round(total / ms[1] / 1e6, 2)
            dev.free()
            dst.free()
            bufs = [C.create_string_buffer(size) for _ in range(16)]

            def host_all():
                def part(k):
                    for f in frames[k::16]:
                        n = z.ZSTD_decompress(bufs[k], size, f, len(f))
                        assert n == size
                list(pool16.map(part, range(16)))

            t = _median_s(host_all, a.reps)
            res["host16_ms"] = round(t * 1e3, 3)
            res["host16_GBps"] = round(total / t / 1e9, 2)
            print(json.dumps(res), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
