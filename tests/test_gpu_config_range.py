"""Every chunker configuration NewConfig accepts (avg = 2^8 .. 2^28) on every cut path, against the CPU oracle and hashlib.

Where the engine branches on the configuration — the scan's pre-rotated break test (9 to 29 mask bits), the batch path's tile
size and per-tile slot capacity, the page ring's default page geometry (small tiles up to avg 128 KiB, big ones from 256 KiB,
pages of up to ~1 GiB), the express thresholds derived from max, SHA-256 chains of up to 1 GiB — each side runs here at every
average. The bytes are the planned streams of tests/config_inputs.py (a content cut at exactly effmin behind an ignored
candidate at effmin - 1, a forced cut at exactly max with no candidate, a candidate exactly at max, content cuts at random
distances, a final chunk below the minimum) plus the 0-byte and the 1-byte stream. Every record is compared field by field
with oracle.chunk_and_digest and every digest with hashlib.

  (a) batch path: one submit below 48 MiB (32 KiB scan tiles) and one of at least 48 MiB (272 KiB tiles), several segments;
  (b) page ring with page_bytes = 0 (its own geometry) through an explicit arena of 10 pages, two streams at once fed from
      the host (reserve -> pbsgpu_memcpy_h2d -> commit), with the express service and without;
  (c) a host-fed payload stream on the engine's ring with default options, written in random sizes;
  (d) pbsgpu_comm_split_stream with one rank.
"""
import hashlib
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import config_inputs as CI  # noqa: E402
from helpers import describe_mismatch, records_equal  # noqa: E402

pytestmark = pytest.mark.gpu

RING_OFF = 0xFFFFFFFF
BIG_BATCH = 48 << 20                   # scan.hip scan_tile_bytes: 272 KiB tiles from here on
TILE_BIG, TILE_SMALL = 64 * 34 * 128, 64 * 4 * 128
ARENA_PAGES = 10


class Plan:
    """the planned streams of one average and their oracle records"""

    def __init__(self, O, avg):
        t0 = time.time()
        self.avg = avg
        self.cfg, self.full, _ = CI.plan_stream(O, avg, seed=avg % 1009 + 3, full=True, target=4 << 20)
        _, self.short, _ = CI.plan_stream(O, avg, seed=avg % 1009 + 5, full=False, target=2 << 20)
        self.tiny = CI.tiny_streams(O, avg, seed=avg % 1009 + 7)
        self.want = {}
        for name, d in (("full", self.full), ("short", self.short), ("tiny0", self.tiny[0]), ("tiny1", self.tiny[1])):
            self.want[name] = O.chunk_and_digest(self.cfg, d, [(0, d.size)]) if d.size else np.zeros(0, O.RECORD_DTYPE)
        self.prep_s = time.time() - t0

    def streams(self):
        return [("full", self.full), ("short", self.short), ("tiny0", self.tiny[0]), ("tiny1", self.tiny[1])]


@pytest.fixture(scope="module", params=CI.AVGS, ids=lambda a: f"avg{a}")
def plan(request, O):
    # module scope: pytest runs every test of one average before building the next one's streams (2.5 GiB at avg 2^28)
    return Plan(O, request.param)


def _engine(avg, **kw):
    from pbs_plus_amd import Engine, buzhash

    return Engine(buzhash.NewConfig(avg), device=0, inflight=1, **kw)


def _check_stream(got, want, data, what):
    """records of one stream (end relative to the stream) vs the oracle's, every digest vs hashlib"""
    assert got.size == want.size and np.array_equal(got["end"], want["end"]), \
        (what, describe_mismatch(got, want))
    assert np.array_equal(got["size"], want["size"]) and np.array_equal(got["digest"], want["digest"]), \
        (what, describe_mismatch(got, want))
    ends = got["end"].astype(np.int64)
    for s, e, dg in zip(ends - got["size"].astype(np.int64), ends, got["digest"]):
        assert bytes(dg) == hashlib.sha256(data[s:e]).digest(), what + (int(s), int(e))


def _report(plan, path, t0):
    print(f"config range avg={plan.avg} {path}: {time.time() - t0:.1f} s (inputs {plan.prep_s:.1f} s)")


# ---- (a) batch path -------------------------------------------------------------------------------------------------------
def _batch(O, eng, plan, parts, pad_to, seed):
    """one submit of the segments `parts` (+ a synthetic pad segment up to pad_to bytes), checked against the oracle"""
    host = [d for _, d in parts]
    if pad_to:
        n = sum(d.size for d in host)
        if n < pad_to:
            host.append(O.fill(pad_to - n + 12345, seed, 0))
    segs, off = [], 0
    for d in host:
        segs.append((off, d.size))
        off += d.size
    buf = np.concatenate(host)
    dev = eng.alloc(max(buf.size, 1))
    try:
        dev.upload(buf)
        assert (buf.size >= BIG_BATCH) == (pad_to >= BIG_BATCH)
        got = eng.collect(eng.submit(dev, segs, nbytes=buf.size))
    finally:
        dev.free()
    want = O.chunk_and_digest(plan.cfg, buf, segs)
    assert records_equal(got, want), (plan.avg, buf.size, describe_mismatch(got, want))
    for k, (o, n) in enumerate(segs):
        sel = got["segment"] == k
        _check_stream(got[sel], want[want["segment"] == k], buf[o:o + n], (plan.avg, "batch", k))
    return got


def test_batch_path_small_and_big_tiles(gpu_lib, O, plan):
    t0 = time.time()
    eng = _engine(plan.avg)
    try:
        # below 48 MiB: heads of the planned streams (whole ones where they fit) and the tiny streams
        cap = 20 << 20
        small = [("full", plan.full[:cap]), ("tiny0", plan.tiny[0]), ("short", plan.short[:cap]), ("tiny1", plan.tiny[1])]
        assert sum(d.size for _, d in small) < BIG_BATCH
        _batch(O, eng, plan, small, 0, plan.avg % 31)
        # at least 48 MiB: the whole planned streams, padded with synthetic bytes where they are shorter
        big = [("tiny1", plan.tiny[1])] + [(n, d) for n, d in plan.streams() if n in ("full", "short")] + [("tiny0", plan.tiny[0])]
        got = _batch(O, eng, plan, big, BIG_BATCH + 7, plan.avg % 29 + 1)
        assert int(got["size"].max()) <= plan.cfg.max
    finally:
        eng.close()
    _report(plan, "batch", t0)


# ---- (b) page ring with its own geometry --------------------------------------------------------------------------------
def _default_page(cfg):
    """ring.cpp's default page: max rounded up to whole scan tiles (big tiles iff max >= 1 MiB), at least two small tiles"""
    tile = TILE_BIG if cfg.max >= (1 << 20) else TILE_SMALL
    page = -(-int(cfg.max) // tile) * tile
    if tile == TILE_SMALL:
        page = max(page, 2 * tile)
    return page, tile


def _feed_two(eng, ring, jobs, t_end):
    """feed host streams through the ring at once (reserve -> H2D -> commit, page by page, round robin); records per job"""
    L = eng._L
    state = []
    for data in jobs:
        state.append(dict(sid=ring.open(), data=data, off=0, done_feed=False, fin=False, recs=[]))
    while not all(s["fin"] for s in state):
        assert time.time() < t_end, ("ring timed out", [(s["off"], s["fin"]) for s in state], ring.stats())
        for s in state:
            if s["done_feed"]:
                continue
            if s["data"].size == 0:
                ring.commit(s["sid"], 0, final=True)
                s["done_feed"] = True
                continue
            r = ring.reserve(s["sid"])
            if r is None:
                continue
            n = min(int(r[1]), s["data"].size - s["off"])
            assert n > 0
            assert L.pbsgpu_memcpy_h2d(eng._h, r[0], s["data"][s["off"]:s["off"] + n].ctypes.data, n) == 0
            s["off"] += n
            s["done_feed"] = s["off"] == s["data"].size
            ring.commit(s["sid"], n, final=s["done_feed"])
        ring.pump()
        for s in state:
            if not s["fin"]:
                recs, s["fin"] = ring.poll(s["sid"])
                s["recs"].append(recs.copy())
        time.sleep(0.001)
    for s in state:
        ring.close_stream(s["sid"])
    return [np.concatenate(s["recs"]) for s in state]


@pytest.mark.parametrize("express", [True, False], ids=["express", "no_express"])
def test_page_ring_default_geometry(gpu_lib, O, plan, express):
    from pbs_plus_amd import PageRing

    t0 = time.time()
    cfg = plan.cfg
    page, tile = _default_page(cfg)
    assert page < (1 << 31)
    eng = _engine(plan.avg)
    ring = None
    try:
        opt = dict(arena_bytes=ARENA_PAGES * (page + 256), page_bytes=0, max_streams=2, sha_cus=8,
                   express_cus=2 if express else RING_OFF)
        ring = PageRing(eng, **opt)
        st = ring.stats()
        assert st["page_bytes"] == page and st["pages_total"] == ARENA_PAGES, (st, page)
        if express:
            assert ring.express() == (2, int(cfg.max) * 13 // 16)
        else:
            assert ring.express()[0] == 0
        pairs = [(plan.full, plan.want["full"], "full"), (plan.short, plan.want["short"], "short"),
                 (plan.tiny[1], plan.want["tiny1"], "tiny1"), (plan.tiny[0], plan.want["tiny0"], "tiny0")]
        for i in range(0, len(pairs), 2):
            both = pairs[i:i + 2]
            got = _feed_two(eng, ring, [d for d, _, _ in both], time.time() + 600.0)
            for g, (d, w, name) in zip(got, both):
                _check_stream(g, w, d, (plan.avg, "ring", express, name))
        ring.quiesce()
        st = ring.stats()
        assert st["pages_free"] == st["pages_total"] and st["pages_recycled"] == st["pages_enqueued"], st
        fed = plan.full.size + plan.short.size + plan.tiny[1].size
        if fed > 2 * ARENA_PAGES * page:
            assert st["pages_enqueued"] > ARENA_PAGES, st                # the arena turned over
    finally:
        if ring is not None:
            ring.close()
        eng.close()
    _report(plan, f"ring {'express' if express else 'no express'} (page {page})", t0)


# ---- (c) host-fed payload stream --------------------------------------------------------------------------------------------
def test_payload_stream_default_options(gpu_lib, O, plan):
    from pbs_plus_amd import PayloadStream

    t0 = time.time()
    eng = _engine(plan.avg)
    rng = np.random.default_rng(plan.avg % 211)
    try:
        for name, data in plan.streams():
            ps = PayloadStream(eng)
            got, pos = [], 0
            hi = max(2, min(64 << 20, data.size // 8 + 2))
            while pos < data.size:
                m = min(int(rng.integers(1, hi)), data.size - pos)
                ps.write(data[pos:pos + m])
                pos += m
                got.append(ps.poll())
            ps.finish()
            got.append(ps.poll())
            got = np.concatenate(got)
            assert (got["segment"] == 0).all()
            _check_stream(got, plan.want[name], data, (plan.avg, "payload stream", name))
            assert ps.position() == data.size
            ps.close()
    finally:
        eng.close()
    _report(plan, "payload stream", t0)


# ---- (d) one-rank split stream ----------------------------------------------------------------------------------------------
def test_comm_split_stream_one_rank(gpu_lib, O, plan):
    import gc

    from pbs_plus_amd import Comm
    from pbs_plus_amd.engine import split_plan

    gc.collect()
    t0 = time.time()
    eng = _engine(plan.avg)
    comm = None
    try:
        comm = Comm(eng, Comm.unique_id(), 0, 1)
        for name, data in plan.streams():
            n = data.size
            if n == 0:
                assert comm.split_stream(0, 0).size == 0
                continue
            assert split_plan(n, 1, 0, plan.cfg.max) == (0, n, 0, n)
            buf = eng.alloc(n + 64)
            try:
                buf.upload(data)
                got = comm.split_stream(buf.ptr, n)
            finally:
                buf.free()
            _check_stream(got, plan.want[name], data, (plan.avg, "split stream", name))
    finally:
        if comm is not None:
            comm.close()
        eng.close()
    _report(plan, "split stream", t0)
