"""Rate of the blob encode with chunks compressed on the device (pbsgpu_blob_encode2_device with PBSGPU_ENCODE_F_ZSTD), in
GiB/s of CONTENT, beside what it is measured against:

* with --seq-tables the same call on an engine created with zstd_seq_tables=1 (repeat offsets and per-block sequence
  tables): its rate and its bytes per content byte beside the default mode's;
* with --window-log N (17, 18 or 19) the same call on an engine created with zstd_window_log=N (the long-range match
  finder: a block's matches may start up to 2^N bytes in front of it), and with --seq-tables as well on one with both;
* the plain pbsgpu_blob_encode_device of the same chunks (what the write side did before it could compress);
* ZSTD_compress level 1 of the same chunks on 16 host threads, where libzstd.so.1 loads (ctypes releases the GIL); where it
  does not load, the leg says so and is left out.

The batch is --chunks chunks (4 096 by default) of 64 KiB to 4 MiB, cut at scattered offsets from three 8 MiB pools: words
over a small alphabet (text), the mixed content of the decoder's fixtures, and random bytes, a third of the chunks each.
Every leg runs in a child process of its own under a time limit of its own, and a leg that fails or runs out of time ends
the run. Each figure is the median of --reps synchronous calls timed with a host clock after one warm-up call, with the
fastest and the slowest beside it. Not measured: the share of the serial lane (sequence and Huffman code), which needs a
kernel variant or a trace, not a clock around the call.

    python tools/zstd_encode_rate.py [--chunks 4096] [--reps 5] [--limit 600] [--seq-tables] [--window-log N]
"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
POOL = 8 << 20
KINDS = ("text", "mixed", "rand")


def _golden():
    spec = importlib.util.spec_from_file_location("make_zstd_golden", os.path.join(ROOT, "tests", "golden", "make_zstd_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def _batch(count):
    """(the three pools back to back, chunk ranges (count, 2) into them, kind of each chunk)"""
    g = _golden()
    pools = g._text_few(POOL, 31) + g._mixed(POOL, 33) + g._rand(POOL, 34)
    rng = np.random.default_rng(35)
    sizes = rng.integers(64 << 10, (4 << 20) + 1, size=count, dtype=np.int64)
    kinds = np.arange(count) % 3
    offs = kinds * POOL + (rng.integers(0, POOL, size=count) % (POOL - sizes + 1))
    return np.frombuffer(pools, np.uint8), np.stack([offs, sizes], axis=1).astype(np.uint64), kinds


def _rates(total, t):
    gib = total / (1 << 30)
    return {"ms": round(t[0] * 1e3, 2), "GiBps": round(gib / t[0], 3), "GiBps_slowest": round(gib / t[2], 3),
            "GiBps_fastest": round(gib / t[1], 3)}


def leg_device(a, zstd, tables=False, window_log=0):
    from pbs_plus_amd import Engine, buzhash

    host, ranges, kinds = _batch(a.chunks)
    total = int(ranges[:, 1].sum())
    options = dict({"zstd_seq_tables": 1} if tables else {}, **({"zstd_window_log": window_log} if window_log else {}))
    eng = Engine(buzhash.NewConfig(4 << 20), device=0, **options)
    dev = eng.alloc(host.size)
    dev.upload(host)
    dst = eng.alloc(total + 12 * a.chunks)
    name = ("encode2_zstd_seq_tables" if tables else "encode2_zstd") + ("_window%d" % window_log if window_log else "")
    res = {"leg": name if zstd else "blob_encode_device", "chunks": a.chunks, "content_bytes": total}
    if zstd:
        fn = lambda: eng.blob_encode2(dev, ranges, dst=dst, zstd=True)  # noqa: E731
        _, offs, lens, kd, crcs, stats = fn()
        res["blob_bytes"] = int(lens.sum())
        res["bytes_per_content_byte"] = round(float(lens.sum()) / total, 4)
        res["compressed_blobs"] = int(kd.sum())
        for k, name in enumerate(KINDS):
            m = kinds == k
            res["ratio_" + name] = round(float(lens[m].sum()) / float(ranges[m, 1].sum() + 12 * m.sum()), 4)
        blocks = int(((ranges[:, 1] + (128 << 10) - 1) // (128 << 10)).sum())
        res["blocks"] = blocks
    else:
        total_c = C.c_uint64()
        segs = np.ascontiguousarray(ranges)
        offs = np.zeros(a.chunks + 1, dtype=np.uint64)

        def fn():
            st = eng._L.pbsgpu_blob_encode_device(eng._h, dev.ptr, dev.nbytes, segs.ctypes.data, a.chunks, dst.ptr, dst.nbytes,
                                                  C.byref(total_c), offs.ctypes.data, None)
            assert st == 0, st
    res.update(_rates(total, _timed(fn, a.reps)))
    dst.free()
    dev.free()
    eng.close()
    print(json.dumps(res), flush=True)


def leg_host(a):
    g = _golden()
    z = g.load_libzstd()
    if z is None:
        print(json.dumps({"leg": "host16_zstd1", "skipped": "libzstd.so.1 does not load on this machine"}), flush=True)
        return
    z.ZSTD_compress.restype = C.c_size_t
    z.ZSTD_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
    host, ranges, kinds = _batch(a.chunks)
    total = int(ranges[:, 1].sum())
    base = host.ctypes.data
    cap = z.ZSTD_compressBound(4 << 20)
    bufs = [C.create_string_buffer(cap) for _ in range(16)]
    out = np.zeros(a.chunks, dtype=np.int64)
    pool16 = ThreadPoolExecutor(16)

    def part(k):
        for i in range(k, a.chunks, 16):
            n = z.ZSTD_compress(bufs[k], cap, base + int(ranges[i, 0]), int(ranges[i, 1]), 1)
            assert not z.ZSTD_isError(n)
            out[i] = n

    def fn():
        list(pool16.map(part, range(16)))

    res = {"leg": "host16_zstd1", "chunks": a.chunks, "content_bytes": total}
    res.update(_rates(total, _timed(fn, a.reps)))
    res["frame_bytes"] = int(out.sum())
    for k, name in enumerate(KINDS):
        m = kinds == k
        res["ratio_" + name] = round(float(out[m].sum()) / float(ranges[m, 1].sum()), 4)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=600, help="seconds each leg may take")
    ap.add_argument("--seq-tables", action="store_true", help="also the zstd leg on an engine with zstd_seq_tables=1")
    ap.add_argument("--window-log", type=int, default=0, choices=(0, 17, 18, 19),
                    help="also the zstd leg (with --seq-tables: both) on an engine with zstd_window_log=N")
    ap.add_argument("--leg", choices=("zstd", "tables", "wzstd", "wtables", "plain", "host"), help="(internal) run one leg in this process")
    a = ap.parse_args()
    if a.leg:
        {"zstd": lambda: leg_device(a, True), "tables": lambda: leg_device(a, True, True), "plain": lambda: leg_device(a, False),
         "wzstd": lambda: leg_device(a, True, False, a.window_log), "wtables": lambda: leg_device(a, True, True, a.window_log),
         "host": lambda: leg_host(a)}[a.leg]()
        return
    legs = ["plain", "zstd"] + (["tables"] if a.seq_tables else [])
    if a.window_log:
        legs += ["wzstd"] + (["wtables"] if a.seq_tables else [])
    legs.append("host")
    for leg in legs:  # each in a fresh process under its own limit; the first that fails ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--chunks", str(a.chunks), "--reps", str(a.reps),
               "--window-log", str(a.window_log)]
        try:
            r = subprocess.run(cmd, timeout=a.limit)
        except subprocess.TimeoutExpired:
            sys.exit("leg %s did not finish in %d s: nothing more is started" % (leg, a.limit))
        if r.returncode != 0:
            sys.exit("leg %s ended with status %d: nothing more is started" % (leg, r.returncode))


if __name__ == "__main__":
    main()
