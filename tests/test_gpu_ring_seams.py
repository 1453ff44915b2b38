"""Every page-seam and block-edge case, in each SHA-256 service form of the page ring, against the CPU oracle and hashlib.

The bytes come from tests/seam_inputs.py: streams whose serial cut list is PLANNED (and confirmed by the oracle), so each case
below is present by construction, not by chance:
  * SHA seam grid: chunks with 1..68 bytes before a seam and a second piece of 0..8 or 52..72 bytes (tail or padding block
    before, on or after the seam), every chunk-start alignment, every chunk length mod 64; chunks that end on a seam;
  * scan seam grid: chunk ends at seam + 1..64 (the window is warmed from the page's head pad) and at seam - 0..64, in a chunk
    that started in the previous page; a cut on a seam with a candidate 64 bytes behind it (one the chunker must ignore);
  * tiny streams: 0..130 bytes and min - 1, min, min + 1 — final chunks below the minimum.
The streams are fed from the host (reserve -> pbsgpu_memcpy_h2d -> commit) through an arena of 8 pages, so pages turn over
all the time and a stale pad holds another stream's bytes.

Which tier served each chunk is checked exactly (PBSGPU_RING_F_TIER_TAG: bits 28-29 of `segment`, 0 main, 1 long, 2 short).
The routing is made deterministic by pacing: one page per round, and the next page is committed only once every record the
committed bytes hold has been polled.
  * A record's flag is raised only after its chunk has been hashed, so when the next round is cut no short-queue entry is
    waiting, and k_ring_prep gives the round the whole room: short_room = lanes_cus x 32 (x 64 with the dense lanes form).
    The lanes rows are sized so that this room is at least the short chunks of any one round (asserted below): every chunk
    of at most short_bytes goes to tier 2, every other one to tier 0.
  * With long_lo_bytes = OFF a chunk goes to the long queue iff its size is at least long_bytes (tier 1). Under this pacing
    the express pairs are idle when a round is published and a round holds fewer long chunks than there are pairs
    (asserted), so pair lanes never take from the long queue (kernels.hip: only while every pair is busy, or more chunks wait
    than there are pairs): tier 1 means the express kernel hashed the chunk.
"""
import hashlib
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seam_inputs as S  # noqa: E402

pytestmark = pytest.mark.gpu

TIER_SHIFT = 28
RING_F_DENSE_SERVICE, RING_F_DENSE_LANES, RING_F_TIER_TAG = 64, 128, 256
RING_OFF = 0xFFFFFFFF
LONG_BYTES = 96                                     # express: every chunk of at least 96 bytes; shorter ones stay on the pairs
SHORT = {256: 1024, 4096: 4096, 65536: 32768}       # lanes: every chunk at avg 256, the seam-crossing and short ones otherwise
ARENA_PAGES = 8


@pytest.fixture(autouse=True)
def _short_idle_timeout(monkeypatch):
    # a service wave that sees no work gives up after this long: a bug must fail a test, not hang the box
    monkeypatch.setenv("PBSGPU_RING_IDLE_TIMEOUT_S", "5")


_PLANS = {}


def _plan(O, avg):
    if avg not in _PLANS:
        cfg, page, streams = S.plan(O, avg)
        want = [O.chunk_and_digest(cfg, d, [(0, d.size)]) if d.size else np.zeros(0, dtype=O.RECORD_DTYPE) for d, _ in streams]
        _PLANS[avg] = (cfg, page, streams, want)
    return _PLANS[avg]


def _round_sizes(ends, size, page):
    """chunk sizes of every round when one page is committed per round (the last round also takes the stream's end)"""
    e = np.asarray(ends, dtype=np.int64)
    sizes = np.diff(np.concatenate([[0], e]))
    k = np.minimum((e - 1) // page, max(0, (size - 1) // page))
    return [sizes[k == i] for i in np.unique(k)]


def _service(name, avg):
    opt = dict(page_bytes=S.PAGES[avg], arena_bytes=ARENA_PAGES * (S.PAGES[avg] + 256), max_streams=2, round_pages=1,
               min_round_pages=1, lone_defer_ms=-1.0, flags=RING_F_TIER_TAG)
    if name == "pair":
        opt.update(sha_cus=4, lanes_cus=0, express_cus=RING_OFF)
    elif name == "dense pair":
        opt.update(sha_cus=4, express_cus=RING_OFF, flags=RING_F_TIER_TAG | RING_F_DENSE_SERVICE)
    elif name in ("lanes", "dense lanes"):
        # avg 256: a page holds 65 chunks, all of them short -> 3 lanes CUs (room 96), which needs sha_cus 4 (lanes <= 3/4)
        lanes = 3 if avg == 256 else 2
        opt.update(sha_cus=4, express_cus=RING_OFF, lanes_cus=lanes, short_bytes=SHORT[avg])
        if name == "dense lanes":
            opt["flags"] |= RING_F_DENSE_LANES
    elif name == "express":
        opt.update(sha_cus=4, express_cus=2, long_bytes=LONG_BYTES, long_lo_bytes=RING_OFF)
    return opt


def _tier_of(name, size, avg):
    if name in ("lanes", "dense lanes"):
        return np.where(size <= SHORT[avg], 2, 0)
    if name == "express":
        return np.where(size >= LONG_BYTES, 1, 0)
    return np.zeros(size.shape, dtype=np.int64)


def _feed_paced(eng, ring, sid, data, ends, page, t_end):
    """one page per round; the next one only when every planned record of the committed bytes is out"""
    L = eng._L
    got, n_got, off = [ring.poll(sid)[0]], 0, 0
    ends = np.asarray(ends, dtype=np.int64)
    while True:
        if data.size == 0:
            ring.commit(sid, 0, final=True)
        else:
            r = None
            while r is None:
                r = ring.reserve(sid)
                if r is None:
                    ring.pump()
                    assert time.time() < t_end, ("no free page", ring.stats(), ring.debug())
            n = min(page, data.size - off)
            assert L.pbsgpu_memcpy_h2d(eng._h, r[0], data[off:off + n].ctypes.data, n) == 0
            off += n
            ring.commit(sid, n, final=(off == data.size))
        final = off == data.size
        need = ends.size if final else int((ends <= off).sum())
        fin = False
        t_page = min(t_end, time.time() + 10.0)       # a page's records come in milliseconds: a missing cut fails here
        while n_got < need or (final and not fin):
            ring.pump()
            recs, fin = ring.poll(sid)
            if recs.size:
                # every record as it comes is the planned one: a wrong cut fails at once, not after a wait for its count
                assert np.array_equal(recs["end"].astype(np.int64), ends[n_got:n_got + recs.size]), \
                    ("cut list differs from the plan", off, n_got, recs["end"][:4], ends[n_got:n_got + 4])
                got.append(recs.copy())
                n_got += recs.size
            assert n_got <= need, ("records beyond the committed bytes", off, n_got, need)
            assert time.time() < t_page, ("records missing", off, n_got, need, ring.stats(), ring.debug())
        if final:
            return np.concatenate(got)


SERVICES = ["pair", "dense pair", "lanes", "dense lanes", "express"]


@pytest.mark.parametrize("avg", [256, 4096, 65536])
@pytest.mark.parametrize("service", SERVICES)
def test_ring_seam_grids_in_every_service_form(gpu_lib, O, avg, service):
    from pbs_plus_amd import Engine, PageRing, buzhash

    cfg, page, streams, want = _plan(O, avg)
    opt = _service(service, avg)
    # the room rule (see the module docstring): every round's short chunks fit the lanes queue, its long ones the pairs
    per_round = [r for d, e in streams for r in _round_sizes(e, d.size, page)]
    if service in ("lanes", "dense lanes"):
        room = opt["lanes_cus"] * (64 if service == "dense lanes" else 32)
        most = max(int((r <= SHORT[avg]).sum()) for r in per_round)
        assert most <= room, (most, room)
    if service == "express":
        most = max(int((r >= LONG_BYTES).sum()) for r in per_round)
        assert most <= 2 * 64, most                                              # express_cus x 64 pairs
    eng = Engine(buzhash.NewConfig(avg), device=0, inflight=1)
    ring = PageRing(eng, **opt)
    if service == "express":
        assert ring.express() == (2, LONG_BYTES)
    t0 = time.time()
    tiers = np.zeros(3, dtype=np.int64)
    try:
        for i, ((data, ends), w) in enumerate(zip(streams, want)):
            sid = ring.open()
            got = _feed_paced(eng, ring, sid, data, ends, page, t0 + 120.0)
            ring.close_stream(sid)
            what = (avg, service, i, data.size)
            assert got.size == ends.size == w.size, what
            assert np.array_equal(got["end"], ends) and np.array_equal(got["end"], w["end"]), what
            assert np.array_equal(got["size"], w["size"]) and np.array_equal(got["digest"], w["digest"]), what
            starts = got["end"].astype(np.int64) - got["size"].astype(np.int64)
            for s, e, dg in zip(starts, got["end"].astype(np.int64), got["digest"]):
                assert bytes(dg) == hashlib.sha256(data[s:e].tobytes()).digest(), what + (int(s), int(e))
            seg = got["segment"].astype(np.int64)
            assert ((seg & ((1 << TIER_SHIFT) - 1)) == sid).all(), what
            tier = (seg >> TIER_SHIFT) & 3
            expect = _tier_of(service, got["size"].astype(np.int64), avg)
            bad = np.nonzero(tier != expect)[0]
            assert bad.size == 0, what + ("tier", [(int(got["end"][j]), int(got["size"][j]), int(tier[j]), int(expect[j]))
                                                   for j in bad[:8]])
            tiers += np.bincount(tier, minlength=3)[:3]
        ring.quiesce()
        st = ring.stats()
        assert st["pages_free"] == st["pages_total"] and st["pages_recycled"] == st["pages_enqueued"], st
        assert st["pages_enqueued"] > 4 * st["pages_total"], st                  # the arena turned over
        assert st["service_launches"] == 1, st
    finally:
        ring.close()
        eng.close()
    # every tier the form has did work
    if service in ("lanes", "dense lanes"):
        assert tiers[2] > 0 and (tiers[0] > 0 or SHORT[avg] == cfg.max), tiers
    if service == "express":
        assert tiers[1] > 0 and tiers[0] > 0, tiers
    print(f"seams avg={avg} {service}: {len(streams)} streams, tiers {tiers.tolist()}, {time.time() - t0:.1f} s")
