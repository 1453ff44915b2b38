"""Rates of the ring-sourced blob encode (pbsgpu_ring_blob_encode_device) and the cost of holding pages, on one GPU:

* (a) the encode of polled chunks straight out of the pages of a holding ring, in GB/s of chunk bytes: one stream at
  NewConfig(4 << 20) with the default pages and one at NewConfig(4096) with 64 KiB pages, every record of the stream in
  one call (the ring is quiesced first: the figure is the encode alone);
* (b) blob_encode_device over the same chunks, copied into one contiguous buffer with pbsgpu_ring_copy_device, in the same
  run; and the ratio (a) / (b);
* (d) the same ring-sourced encode with the known-chunk check in front of it, half of the digests in the set beforehand and
  insert = 0 (so that repeated calls see the same set): pbsgpu_ring_upload_new_device, which keeps the flags on the device
  and builds the plan there, against pbsgpu_known_classify_host + pbsgpu_ring_blob_encode_device(skip = known), on the same
  polled records, alternating in the same run;
* (e) the compressing writer's call (--zstd, only these legs): pbsgpu_ring_upload_new2_device with PBSGPU_ENCODE_F_ZSTD
  against the route it replaces, pbsgpu_known_classify_host -> pbsgpu_ring_copy_device of every new chunk into one flat
  buffer -> pbsgpu_blob_encode2_device(F_ZSTD), on the same polled records with half of the digests known, alternating;
  the same call with flags = 0 against pbsgpu_ring_upload_new_device; and both with EVERY digest known, which is the
  cost of the encoder's grid when it has nothing to do;
* (c) the feed rate of a ring with the flag on whose consumer releases after every poll against the same ring with the flag
  off (GiB/s from the first fill to the last record), and the share of the arena that was held on average.

(a), (b) and (d) are the median of a few synchronous calls timed with a host clock, after one warm-up call; (c) alternates
the two rings and reports the median of its runs (--no-feed leaves it out).

    python tools/ring_upload_rate.py [--big-gib 2] [--small-mib 256] [--feed-gib 512] [--reps 5] [--no-feed] [--zstd]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_s(fn, reps):
    fn()  # warm-up (first-use allocation of the leased work buffers)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def _ingest(ring, seed, kind, nbytes):
    """one whole synthetic stream into a holding ring that releases nothing: (stream, records)"""
    sid = ring.open()
    left, recs, fin = nbytes, [], False
    while not fin:
        if left:
            want = min(left, 64 * ring.page_bytes)
            left -= ring.fill(sid, seed, kind, want, final=(want == left))
        ring.pump()
        r, fin = ring.poll(sid, cap=1 << 16)
        recs.append(r.copy())
    return sid, np.concatenate(recs)


def _alternating_ms(fns, reps):
    """every function once as a warm-up, then `reps` rounds that run them one after the other: [ms per round] per function"""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for t, fn in zip(ts, fns):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
    return ts


def fused_against_two_calls(a, eng, ring, sid, recs, dst):
    """(d): the row's "upload_new" entry"""
    from pbs_plus_amd import KnownChunks, _lib

    L = _lib.lib()
    n = int(recs.size)
    known = KnownChunks(eng, capacity=2 * n)
    known.add(recs[::2])
    out = [dict(flags=np.zeros(n, dtype=np.uint8), offs=np.zeros(n, dtype=np.uint64), crcs=np.zeros(n, dtype=np.uint32),
                used=C.c_uint64(), st=_lib.DedupStats()) for _ in range(2)]

    def two_calls():
        o = out[0]
        _lib.check(L.pbsgpu_known_classify_host(known._h, recs.ctypes.data, n, 0, o["flags"].ctypes.data, C.byref(o["st"])),
                   "known_classify_host")
        _lib.check(L.pbsgpu_ring_blob_encode_device(ring._h, sid, recs.ctypes.data, n, o["flags"].ctypes.data, dst.ptr, dst.nbytes,
                                                    o["offs"].ctypes.data, o["crcs"].ctypes.data, C.byref(o["used"])),
                   "ring_blob_encode_device")

    def fused():
        o = out[1]
        _lib.check(L.pbsgpu_ring_upload_new_device(ring._h, known._h, sid, recs.ctypes.data, n, 0, dst.ptr, dst.nbytes,
                                                   o["flags"].ctypes.data, o["offs"].ctypes.data, o["crcs"].ctypes.data,
                                                   C.byref(o["used"]), C.byref(o["st"])), "ring_upload_new_device")

    t_two, t_fused = _alternating_ms((two_calls, fused), a.reps)
    for k in ("flags", "offs", "crcs"):
        assert np.array_equal(out[0][k], out[1][k]), k
    assert out[0]["used"].value == out[1]["used"].value and len(known) == recs[::2].size
    new_bytes = int(out[1]["st"].unique_bytes)
    known.close()
    med2, medf = statistics.median(t_two), statistics.median(t_fused)
    return {"new_chunks": int(out[1]["st"].nunique), "new_bytes": new_bytes,
            "two_calls_ms": [round(x, 3) for x in t_two], "fused_ms": [round(x, 3) for x in t_fused],
            "two_calls_median_ms": med2, "fused_median_ms": medf,
            "two_calls_GBps": new_bytes / med2 / 1e6, "fused_GBps": new_bytes / medf / 1e6, "fused_over_two_calls": med2 / medf}


def zstd_against_three_calls(a, eng, ring, sid, recs, dst):
    """(e): the row's "upload_new2" entry"""
    from pbs_plus_amd import KnownChunks, _lib

    L = _lib.lib()
    n = int(recs.size)
    half, every = KnownChunks(eng, capacity=2 * n), KnownChunks(eng, capacity=2 * n)
    half.add(recs[::2])
    every.add(recs)
    starts = (recs["end"] - recs["size"]).astype(np.uint64)
    flat = eng.alloc(max(int(recs["size"].astype(np.uint64).sum()), 16))

    def outputs():
        return dict(flags=np.zeros(n, dtype=np.uint8), offs=np.zeros(n, dtype=np.uint64), lens=np.zeros(n, dtype=np.uint32),
                    kinds=np.zeros(n, dtype=np.uint8), crcs=np.zeros(n, dtype=np.uint32), used=C.c_uint64(), st=_lib.DedupStats(),
                    enc=_lib.EncodeStats())

    out = {k: outputs() for k in ("three", "fused", "plain_old", "plain_new", "known_old", "known_new")}

    def three_calls():
        o = out["three"]
        _lib.check(L.pbsgpu_known_classify_host(half._h, recs.ctypes.data, n, 0, o["flags"].ctypes.data, C.byref(o["st"])),
                   "known_classify_host")
        new = np.flatnonzero(o["flags"] == 0)
        sizes = recs["size"][new].astype(np.uint64)
        ends = np.cumsum(sizes)
        for j, i in enumerate(new):
            _lib.check(L.pbsgpu_ring_copy_device(ring._h, sid, int(starts[i]), int(sizes[j]), flat.ptr + int(ends[j] - sizes[j])),
                       "ring_copy_device")
        segs = np.ascontiguousarray(np.stack([ends - sizes, sizes], axis=1))
        offs = np.zeros(new.size + 1, dtype=np.uint64)
        lens, kinds, crcs = (np.zeros(new.size, dtype=t) for t in (np.uint32, np.uint8, np.uint32))
        _lib.check(L.pbsgpu_blob_encode2_device(eng._h, flat.ptr, int(ends[-1]), segs.ctypes.data, new.size, _lib.ENCODE_F_ZSTD,
                                                dst.ptr, dst.nbytes, offs.ctypes.data, lens.ctypes.data, kinds.ctypes.data,
                                                crcs.ctypes.data, C.byref(o["enc"])), "blob_encode2_device")
        o["offs"][new], o["lens"][new], o["kinds"][new], o["crcs"][new] = offs[:-1], lens, kinds, crcs
        o["used"].value = int(offs[-1])

    def new2(key, known, flags):
        def run():
            o = out[key]
            _lib.check(L.pbsgpu_ring_upload_new2_device(ring._h, known._h, sid, recs.ctypes.data, n, 0, flags, dst.ptr, dst.nbytes,
                                                        o["flags"].ctypes.data, o["offs"].ctypes.data, o["lens"].ctypes.data,
                                                        o["kinds"].ctypes.data, o["crcs"].ctypes.data, C.byref(o["used"]),
                                                        C.byref(o["st"]), C.byref(o["enc"])), "ring_upload_new2_device")
        return run

    def old(key, known):
        def run():
            o = out[key]
            _lib.check(L.pbsgpu_ring_upload_new_device(ring._h, known._h, sid, recs.ctypes.data, n, 0, dst.ptr, dst.nbytes,
                                                       o["flags"].ctypes.data, o["offs"].ctypes.data, o["crcs"].ctypes.data,
                                                       C.byref(o["used"]), C.byref(o["st"])), "ring_upload_new_device")
        return run

    t_three, t_fused = _alternating_ms((three_calls, new2("fused", half, _lib.ENCODE_F_ZSTD)), a.reps)
    for k in ("flags", "offs", "lens", "kinds", "crcs"):
        assert np.array_equal(out["three"][k], out["fused"][k]), k
    assert out["three"]["used"].value == out["fused"]["used"].value
    t_old, t_new = _alternating_ms((old("plain_old", half), new2("plain_new", half, 0)), a.reps)
    for k in ("flags", "offs", "crcs"):
        assert np.array_equal(out["plain_old"][k], out["plain_new"][k]), k
    t_kold, t_knew = _alternating_ms((old("known_old", every), new2("known_new", every, _lib.ENCODE_F_ZSTD)), a.reps)
    assert out["known_new"]["used"].value == 0 and np.all(out["known_new"]["flags"] == 1)
    new_bytes = int(out["fused"]["st"].unique_bytes)
    enc = out["fused"]["enc"]
    half.close()
    every.close()
    flat.free()

    def leg(ts):
        return {"ms": [round(x, 3) for x in ts], "median_ms": statistics.median(ts)}

    m3, mf = statistics.median(t_three), statistics.median(t_fused)
    return {"new_chunks": int(out["fused"]["st"].nunique), "new_bytes": new_bytes, "compressed_blobs": int(enc.blobs[1]),
            "three_calls": leg(t_three), "fused_zstd": leg(t_fused), "fused_over_three_calls": m3 / mf,
            "three_calls_GiBps": new_bytes / m3 * 1e3 / (1 << 30), "fused_zstd_GiBps": new_bytes / mf * 1e3 / (1 << 30),
            "plain_upload_new": leg(t_old), "plain_upload_new2": leg(t_new),
            "all_known_upload_new": leg(t_kold), "all_known_upload_new2_zstd": leg(t_knew)}


def zstd_rates(a, name, avg, nbytes, ring_opt):
    """(e) alone, on the records of one stream held by the ring"""
    from pbs_plus_amd import Engine, PageRing, buzhash

    eng = Engine(buzhash.NewConfig(avg), device=0)
    ring = PageRing(eng, hold=True, **ring_opt)
    sid, recs = _ingest(ring, 0xB10B, 0, nbytes)
    ring.quiesce()
    n = int(recs.size)
    dst = eng.alloc(int(recs["size"].astype(np.uint64).sum()) + 12 * n)
    row = {"batch": name, "chunks": n, "bytes": nbytes, "page_bytes": ring.page_bytes,
           "upload_new2": zstd_against_three_calls(a, eng, ring, sid, recs, dst)}
    print(json.dumps(row), flush=True)
    dst.free()
    ring.close_stream(sid)
    ring.close()
    eng.close()
    return row


def encode_rates(a, name, avg, nbytes, ring_opt):
    from pbs_plus_amd import Engine, PageRing, _lib, buzhash
    from pbs_plus_amd.engine import _segs

    eng = Engine(buzhash.NewConfig(avg), device=0)
    L = _lib.lib()
    ring = PageRing(eng, hold=True, **ring_opt)
    page = ring.page_bytes
    assert ring.stats()["pages_total"] * page >= nbytes + 4 * page, "the arena must hold the whole stream"
    sid, recs = _ingest(ring, 0xB10B, 0, nbytes)
    ring.quiesce()
    n = int(recs.size)
    data = int(recs["size"].astype(np.uint64).sum())
    starts = recs["end"] - recs["size"]
    two_pages = int((starts // page != (recs["end"] - 1) // page).sum())
    dst = eng.alloc(data + 12 * n)
    offs = np.zeros(n + 1, dtype=np.uint64)
    crcs = np.zeros(n, dtype=np.uint32)
    used = C.c_uint64()

    def from_ring():
        _lib.check(L.pbsgpu_ring_blob_encode_device(ring._h, sid, recs.ctypes.data, n, None, dst.ptr, dst.nbytes,
                                                    offs.ctypes.data, crcs.ctypes.data, C.byref(used)), "ring_blob_encode_device")

    t_ring = _median_s(from_ring, a.reps)
    crc_ring = crcs.copy()
    upload_new = fused_against_two_calls(a, eng, ring, sid, recs, dst)
    flat = ring.copy(sid, 0, nbytes)
    segs, ns = _segs(list(zip(starts.tolist(), recs["size"].tolist())))

    def contiguous():
        _lib.check(L.pbsgpu_blob_encode_device(eng._h, flat.ptr, nbytes, segs, ns, dst.ptr, dst.nbytes, C.byref(used),
                                               offs.ctypes.data, crcs.ctypes.data), "blob_encode_device")

    t_flat = _median_s(contiguous, a.reps)
    assert np.array_equal(crc_ring, crcs)
    row = {"batch": name, "chunks": n, "bytes": data, "chunks_in_two_pages": two_pages, "page_bytes": page,
           "ring_encode_GBps": data / t_ring / 1e9, "contiguous_encode_GBps": data / t_flat / 1e9,
           "ring_over_contiguous": t_flat / t_ring, "ms": {"ring": t_ring * 1e3, "contiguous": t_flat * 1e3}, "upload_new": upload_new}
    print(json.dumps(row), flush=True)
    flat.free()
    dst.free()
    ring.close_stream(sid)
    ring.close()
    eng.close()
    return row


def feed_once(eng, hold, total, nstreams, arena):
    """(GiB/s from the first fill to the last record, mean share of the arena held by handed-back pages, arena bytes)"""
    from pbs_plus_amd import PageRing

    ring = PageRing(eng, hold=hold, arena_bytes=arena, max_streams=nstreams)  # arena 0: what is free minus 8 GiB
    per = total // nstreams
    left = {ring.open(): per for _ in range(nstreams)}
    live = set(left)
    pages = ring.stats()["pages_total"]
    shares = []
    t0 = time.perf_counter()
    while live:
        for sid in live:
            if left[sid]:
                want = min(left[sid], 64 * ring.page_bytes)
                left[sid] -= ring.fill(sid, 1000 + sid, 4, want, final=(want == left[sid]))
        ring.pump()
        recs, fins = ring.poll_any()
        if hold and recs.size:
            sids = recs["segment"] & 0x0FFFFFFF
            shares.append(sum(ring.held(s)[1] for s in live) / pages)   # before the release: what the consumer was keeping
            for s in np.unique(sids):
                ring.release(int(s), int(recs["end"][sids == s].max()))
        for s in fins:
            ring.close_stream(int(s))
            live.discard(int(s))
    dt = time.perf_counter() - t0
    ring.quiesce()
    ring.close()
    return per * nstreams / dt / (1 << 30), (statistics.mean(shares) if shares else 0.0), pages * ring.page_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big-gib", type=float, default=2.0, help="stream of the 4 MiB-average encode")
    ap.add_argument("--small-mib", type=int, default=256, help="stream of the 4 KiB-average encode")
    ap.add_argument("--feed-gib", type=float, default=512.0, help="bytes of one feed-rate run")
    ap.add_argument("--feed-streams", type=int, default=8)
    ap.add_argument("--feed-arena-gib", type=float, default=0.0, help="0 = the ring's default arena, as the benchmark's")
    ap.add_argument("--feed-reps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-feed", action="store_true", help="only the encode legs")
    ap.add_argument("--zstd", action="store_true", help="only the legs of the compressing call (e)")
    a = ap.parse_args()

    from pbs_plus_amd import Engine, buzhash

    big = int(a.big_gib * (1 << 30))
    small = a.small_mib << 20
    shapes = (("4MiB-avg", 4 << 20, big, dict(arena_bytes=big + (256 << 20), max_streams=2)),
              ("4KiB-avg", 4096, small,
               dict(arena_bytes=(small // 65536 + 64) * (65536 + 256), page_bytes=65536, max_streams=2, round_pages=256)))
    for shape in shapes:
        (zstd_rates if a.zstd else encode_rates)(a, *shape)
    if a.zstd:
        return
    if a.no_feed:
        return
    eng = Engine(buzhash.NewConfig(4 << 20), device=0)
    total, arena = int(a.feed_gib * (1 << 30)), int(a.feed_arena_gib * (1 << 30))
    feed_once(eng, False, total // 8, a.feed_streams, arena)  # warm-up
    runs = {False: [], True: []}
    share = []
    for _ in range(a.feed_reps):
        for hold in (False, True):
            rate, sh, arena_used = feed_once(eng, hold, total, a.feed_streams, arena)
            runs[hold].append(rate)
            if hold:
                share.append(sh)
    row = {"batch": "feed", "bytes": total, "streams": a.feed_streams, "arena_bytes": arena_used,
           "plain_GiBps": statistics.median(runs[False]), "holding_GiBps": statistics.median(runs[True]),
           "plain_runs": [round(x, 1) for x in runs[False]], "holding_runs": [round(x, 1) for x in runs[True]],
           "arena_share_held_mean": statistics.mean(share)}
    print(json.dumps(row), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
