"""Rates of the known-chunk set (pbsgpu_known_*) on one GPU: records/s of classify_device and classify_host, and of
add_device, for batches of 1 M and 16 M records against sets of 16 M and 64 M digests.

Records are pseudo-random bytes written on the device by the engine's fill kernel (a random 32-byte digest and size per
48-byte record), so nothing large crosses the host. Each figure is the median of a few synchronous calls timed with a
host clock, after one warm-up call. Queries are either drawn from the set (all known) or fresh (all new); classify
runs with insert=0 so that every repetition sees the same set.

    python tools/known_set_rate.py [--sets 16,64] [--batches 1,16] [--reps 5]
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

M = 1 << 20


def _median_s(fn, reps):
    fn()  # warm-up (first-use allocation of the leased work buffers)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="16,64", help="set sizes in Mi digests")
    ap.add_argument("--batches", default="1,16", help="batch sizes in Mi records")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()

    from pbs_plus_amd import Engine, KnownChunks, buzhash

    eng = Engine(buzhash.NewConfig(4 << 20), device=0)
    sets = [int(x) * M for x in a.sets.split(",")]
    batches = [int(x) * M for x in a.batches.split(",")]
    nq = max(batches)
    qbuf = eng.alloc(nq * 48)
    eng.fill(qbuf.ptr, nq * 48, seed=0xF12E5, kind=0)              # fresh digests
    host_fresh = qbuf.download()
    rows = []
    for S in sets:
        sbuf = eng.alloc(S * 48)
        eng.fill(sbuf.ptr, S * 48, seed=0x5E7 + S, kind=0)
        # add rate: with growth from the default size (this first call also sizes the leased work buffers), then into
        # an empty set sized for S (no growth) — the set the classify rates run against
        k = KnownChunks(eng)
        t0 = time.perf_counter()
        k.add_device(sbuf.ptr, S)
        t_grow = time.perf_counter() - t0
        assert len(k) == S, (len(k), S)
        k.close()
        k = KnownChunks(eng, capacity=S)
        t0 = time.perf_counter()
        k.add_device(sbuf.ptr, S)
        t_add = time.perf_counter() - t0
        assert len(k) == S, (len(k), S)
        rows.append({"op": "add_device", "set": S, "n": S, "s": round(t_add, 4), "rec_per_s": S / t_add,
                     "with_growth_s": round(t_grow, 4), "with_growth_rec_per_s": S / t_grow})
        host_known = sbuf.download(0, nq * 48)
        for n in batches:
            for what, dptr, host in (("known", sbuf.ptr, host_known), ("new", qbuf.ptr, host_fresh)):
                res = {}

                def dev():
                    res["f"], res["st"] = k.classify_device(dptr, n, insert=False)

                tdev = _median_s(dev, a.reps)
                assert res["st"]["nunique"] == (0 if what == "known" else n), res["st"]
                recs = host[: n * 48].view(np.dtype([("end", "<u8"), ("digest", "u1", (32,)), ("segment", "<u4"),
                                                     ("size", "<u4")]))

                def hst():
                    res["fh"], res["sth"] = k.classify(recs, insert=False)

                thost = _median_s(hst, a.reps)
                assert np.array_equal(res["f"], res["fh"])
                rows.append({"op": "classify", "queries": what, "set": S, "n": n, "device_s": round(tdev, 5),
                             "device_rec_per_s": n / tdev, "host_s": round(thost, 5), "host_rec_per_s": n / thost})
        k.close()
        sbuf.free()
    qbuf.free()
    eng.close()
    for r in rows:
        print(json.dumps(r))
    print("\n| op | queries | set | n | device rec/s | host rec/s |\n|---|---|---|---|---|---|")
    for r in rows:
        if r["op"] == "classify":
            print(f"| classify | {r['queries']} | {r['set'] // M} Mi | {r['n'] // M} Mi | {r['device_rec_per_s']:.3g} "
                  f"| {r['host_rec_per_s']:.3g} |")
        else:
            print(f"| add_device | - | {r['set'] // M} Mi | {r['n'] // M} Mi | {r['rec_per_s']:.3g} "
                  f"(growing from the default: {r['with_growth_rec_per_s']:.3g}) | - |")


if __name__ == "__main__":
    main()
