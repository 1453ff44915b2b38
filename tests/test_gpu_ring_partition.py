"""How the synthetic refill and the scan share the cut side of a page ring, against the CPU oracle, through the
C ABI. The refill is a fixed number of 1024-thread workgroups that take slices of the round's pages from an atomic counter. By
default it runs in turn with the scan while a service runs; with `fill_cus` it is that many whole-CU workgroups beside the
scan, which gets the rest of the cut side, so that the refill of round n + 1, the scan of round n and the control kernel of
round n - 1 run at the same time. Whatever the mode, the counts, the round size and the mix of refilled and host-fed pages,
every stream's records are those of the serial chunker + SHA-256 over the same bytes, and every page comes back.

Common shape: avg 4 KiB chunker, 64 KiB pages, an arena of 24 pages that turns over at least ten times, 4 pair + 2 express CUs.
(64 KiB pages are one partial refill slice each; the case with 320 KiB pages has whole slices and a partial last one.)"""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AVG = 4096
PAGE = 65536
ARENA_PAGES = 24
KiB, MiB = 1 << 10, 1 << 20


@pytest.fixture(autouse=True)
def _short_idle_timeout(monkeypatch):
    # a service wave that sees no work gives up after this long: a bug must fail a test, not hang the box
    monkeypatch.setenv("PBSGPU_RING_IDLE_TIMEOUT_S", "5")


_WANT = {}


def _want(O, seed, kind, n):
    """the oracle's records of one synthetic stream, computed once per session"""
    key = (seed, kind, n)
    if key not in _WANT:
        _WANT[key] = (O.chunk_and_digest(O.new_config(AVG), O.fill(n, seed, kind), [(0, n)]) if n
                      else np.zeros(0, dtype=O.RECORD_DTYPE))
    return _WANT[key]


def _same(got, want, what):
    assert got.size == want.size, (what, got.size, want.size)
    for f in ("end", "size", "digest"):
        assert np.array_equal(got[f], want[f]), (what, f)


def _engine(**options):
    from pbs_plus_amd import Engine, buzhash

    return Engine(buzhash.NewConfig(AVG), device=0, inflight=1, **options)


def _ring(eng, page=PAGE, pages=ARENA_PAGES, **opt):
    from pbs_plus_amd import PageRing

    o = dict(arena_bytes=pages * (page + 256), page_bytes=page, max_streams=8, sha_cus=4, express_cus=2, round_pages=6)
    o.update(opt)
    return PageRing(eng, **o)


def _finish(ring, turns=10):
    ring.quiesce()
    st = ring.stats()
    assert st["pages_free"] == st["pages_total"], st
    assert st["pages_recycled"] == st["pages_enqueued"], st
    assert st["pages_enqueued"] >= turns * st["pages_total"], st
    ring.close()


# every generator kind 0-4; a zero-length stream, one of 63 bytes, one that ends one byte into a page, one of exactly three pages
JOBS = [(61, 0, 4 * MiB + 5), (62, 1, 3 * MiB), (63, 2, 3 * MiB + 3), (64, 3, 3 * MiB + 77), (65, 4, 3 * MiB + PAGE + 1),
        (66, 0, 0), (67, 0, 63), (68, 4, 3 * PAGE), (69, 2, 2 * PAGE + 1)]


@pytest.mark.parametrize("round_pages", [6, 2])
@pytest.mark.parametrize("fill_cus", [1, 2, 64])
def test_fixed_refill_workgroups_and_slices(gpu_lib, O, fill_cus, round_pages):
    """refill workgroups beside the scan: 1, 2 and more than a round has pages (workgroups that find no item): the slice
    arithmetic at a page's partial slice, the ticket counter zeroed for every round."""
    eng = _engine()
    ring = _ring(eng, round_pages=round_pages, fill_cus=fill_cus)
    got = ring.ingest_synthetic(JOBS, timeout_s=60.0)
    for j, g in zip(JOBS, got):
        _same(g, _want(O, *j), (fill_cus, round_pages, j))
    _finish(ring)
    eng.close()


def test_pages_of_several_slices_with_a_partial_last_one(gpu_lib, O):
    """320 KiB pages = two whole refill slices and a half; streams that end inside the first, the second and the third slice"""
    page = 320 * KiB
    jobs = [(71, 4, 12 * MiB + 100 * KiB + 16), (72, 0, 8 * MiB + 200 * KiB + 1), (73, 3, 5 * MiB + 300 * KiB + 9), (74, 4, 2 * page)]
    eng = _engine()
    ring = _ring(eng, page=page, pages=8, fill_cus=3)
    got = ring.ingest_synthetic(jobs, timeout_s=60.0)
    for j, g in zip(jobs, got):
        _same(g, _want(O, *j), j)
    _finish(ring)
    eng.close()


@pytest.mark.parametrize("fill_cus", [2, 0])
def test_three_rounds_in_flight(gpu_lib, O, fill_cus):
    """round_pages=2, max_inflight=3, eight streams at once: with fill_cus the next round's refill runs beside this round's scan
    and the previous round's control kernel; without, behind this round's scan"""
    jobs = [(81 + i, i % 5, 2 * MiB + 4099 * i + (i % 3)) for i in range(8)]
    eng = _engine()
    ring = _ring(eng, round_pages=2, max_inflight=3, fill_cus=fill_cus)
    got = ring.ingest_synthetic(jobs, timeout_s=60.0)
    for j, g in zip(jobs, got):
        _same(g, _want(O, *j), j)
    _finish(ring)
    eng.close()


@pytest.mark.parametrize("fill_cus", [2, 0])
def test_piece_table_stream_beside_a_kind4_stream(gpu_lib, O, fill_cus):
    """generator kind 5 (a piece table over generator 4, as the rechunk workload builds it) and kind 4 in the same rounds"""
    rng = np.random.default_rng(5)
    rows, pos, npos, src = [], 0, 0, 0
    while pos < 8 * MiB:
        ln = int(rng.integers(1, 6000)) * 16
        if len(rows) % 3 == 1:                               # new bytes
            rows.append((pos, ln, npos, 777))
            npos += ln
        else:                                                # kept extent (an occasional deletion in between)
            src += int(rng.integers(0, 300)) * 16 * (len(rows) % 2)
            rows.append((pos, ln, src, 555))
            src += ln
        pos += ln
    host = np.empty(pos, dtype=np.uint8)
    for dst, ln, so, seed in rows:
        O.fill(ln, seed, 4, stream_off=so, out=host[dst:dst + ln])
    want_p = O.chunk_and_digest(O.new_config(AVG), host, [(0, pos)])
    job4 = (91, 4, 8 * MiB + 12345)
    eng = _engine()
    ring = _ring(eng, fill_cus=fill_cus)
    sp, s4 = ring.open(), ring.open()
    left = {sp: pos, s4: job4[2]}
    got = {sp: [], s4: []}
    fin = {sp: False, s4: False}
    first = True
    t0 = time.time()
    while not all(fin.values()) and time.time() - t0 < 60:
        if left[sp]:
            n = min(left[sp], 5 * PAGE)
            left[sp] -= ring.fill_pieces(sp, np.array(rows, dtype=np.uint64) if first else None, n, final=(n == left[sp]))
            first = False
        if left[s4]:
            n = min(left[s4], 5 * PAGE)
            left[s4] -= ring.fill(s4, job4[0], 4, n, final=(n == left[s4]))
        ring.pump()
        for s in (sp, s4):
            if not fin[s]:
                recs, fin[s] = ring.poll(s)
                got[s].append(recs.copy())
    assert all(fin.values()), ring.debug()
    _same(np.concatenate(got[sp]), want_p, "piece table")
    _same(np.concatenate(got[s4]), _want(O, *job4), "kind 4")
    ring.close_stream(sp)
    ring.close_stream(s4)
    _finish(ring)
    eng.close()


@pytest.mark.parametrize("fill_cus", [3, 0])
def test_host_fed_streams_beside_a_synthetic_stream(gpu_lib, O, fill_cus):
    """Rounds with and without pages to refill, back to back: a stream whose 300 KiB come from the host page by page (reserve /
    copy / commit) shares the ring with a synthetic stream, and pump() is called after either kind of page; meanwhile a payload
    stream (pbsgpu_stream_write, 300 KiB) goes through the same engine's own ring, whose rounds never refill anything."""
    from pbs_plus_amd import PayloadStream

    eng = _engine(stream_sha_cus=4, stream_express_cus=2, stream_page_bytes=PAGE, stream_ring_gib=0.02)
    L = eng._L
    cfg = O.new_config(AVG)
    n_host = 300 * KiB
    data = O.fill(n_host, 101, 0)
    pdata = O.fill(n_host, 102, 3)
    jobs = (103, 4, 16 * MiB + 7)
    ring = _ring(eng, fill_cus=fill_cus)
    sh, ss = ring.open(), ring.open()
    ps = PayloadStream(eng)
    off, poff, left = 0, 0, jobs[2]
    got = {sh: [], ss: []}
    fin = {sh: False, ss: False}
    pgot = []
    t0 = time.time()
    while not all(fin.values()) and time.time() - t0 < 60:
        if off < n_host and left < jobs[2] - 2 * MiB * (off // PAGE):     # a host page every 2 MiB of the synthetic stream
            r = ring.reserve(sh)
            if r is not None:
                n = min(PAGE, n_host - off)
                assert L.pbsgpu_memcpy_h2d(eng._h, r[0], data[off:off + n].ctypes.data, n) == 0
                off += n
                ring.commit(sh, n, final=(off == n_host))
                ring.pump()                                              # (a round without a page to refill, if nothing else waits)
                if poff < n_host:
                    ps.write(pdata[poff:poff + 50_000])
                    poff += 50_000
                    pgot.append(ps.poll())
        if left:
            n = min(left, 4 * PAGE)
            left -= ring.fill(ss, jobs[0], jobs[1], n, final=(n == left))
        ring.pump()
        for s in (sh, ss):
            if not fin[s]:
                recs, fin[s] = ring.poll(s)
                got[s].append(recs.copy())
    assert all(fin.values()) and off == n_host, (fin, off, ring.debug())
    if poff < n_host:
        ps.write(pdata[poff:])
    ps.finish()
    pgot.append(ps.poll())
    ps.close()
    _same(np.concatenate(got[sh]), O.chunk_and_digest(cfg, data, [(0, n_host)]), "host-fed ring stream")
    _same(np.concatenate(got[ss]), _want(O, *jobs), "synthetic stream")
    _same(np.concatenate(pgot), O.chunk_and_digest(cfg, pdata, [(0, n_host)]), "payload stream")
    ring.close_stream(sh)
    ring.close_stream(ss)
    _finish(ring)
    eng.close()
