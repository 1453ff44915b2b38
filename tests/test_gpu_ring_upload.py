"""Held ring pages and blobs framed straight out of them (PageRing(hold=True): release / held / blob_encode / copy).

Every blob is compared byte for byte with the generator's bytes for its stream range (Engine.fill into a buffer), its CRC
with zlib, its data with the record's SHA-256 through hashlib; the records with the CPU oracle's and with those of a ring
without the flag. The chunks whose bytes lie in two pages are counted from the oracle's cut list, so the test knows that the
two-part path was taken and how often; cuts placed by ring.suggest give first and last parts of 1, 2 and 3 bytes."""
import hashlib
import os
import sys
import time
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seam_inputs as S  # noqa: E402

pytestmark = pytest.mark.gpu

MAGIC = hashlib.sha256(b"Proxmox Backup uncompressed blob v1.0").digest()[:8]
SID_MASK = (1 << 28) - 1


@pytest.fixture(autouse=True)
def _short_idle_timeout(monkeypatch):
    # a service wave that sees no work gives up after this long: a bug must fail a test, not hang the box
    monkeypatch.setenv("PBSGPU_RING_IDLE_TIMEOUT_S", "10")


def _engine(avg):
    from pbs_plus_amd import Engine, buzhash

    return Engine(buzhash.NewConfig(avg), device=0, inflight=1)


def _generator_bytes(eng, job):
    """the stream's bytes as the device generator writes them: Engine.fill into a buffer, copied out"""
    n = job["n"]
    if n == 0:
        return np.zeros(0, dtype=np.uint8)
    buf = eng.alloc(n)
    if job["mode"] == "fill":
        eng.fill(buf.ptr, n, seed=job["seed"], kind=job["kind"])
    else:
        for dst, ln, so, seed in job["rows"]:
            eng.fill(buf.ptr + dst, ln, seed=seed, kind=4, stream_off=so)
    host = buf.download()
    buf.free()
    return host


def _edited_rows(rng, total):
    """a piece table over generator 4 (kept extents of a base file, new bytes in between), `total` bytes, all multiples of 16"""
    rows, pos, npos, src, i = [], 0, 0, 0, 0
    while pos < total:
        ln = min(int(rng.integers(1, 1 << 16)) * 16, total - pos)
        if i % 3 == 1:
            rows.append((pos, ln, npos, 777))
            npos += ln
        else:
            src += int(rng.integers(0, 300)) * 16 * (i % 2)
            rows.append((pos, ln, src, 555))
            src += ln
        pos += ln
        i += 1
    return rows


def _feed(eng, ring, sid, job, a, page):
    if a["sent_final"]:
        return
    left = job["n"] - a["off"]
    if job["mode"] == "host":
        data = job["data"]
        if data.size == 0:
            ring.commit(sid, 0, final=True)
            a["sent_final"] = True
            return
        for _ in range(8):
            r = ring.reserve(sid)
            if r is None:
                return
            n = min(page, data.size - a["off"])
            assert eng._L.pbsgpu_memcpy_h2d(eng._h, r[0], data[a["off"]:a["off"] + n].ctypes.data, n) == 0
            a["off"] += n
            ring.commit(sid, n, final=(a["off"] == data.size))
            if a["off"] == data.size:
                a["sent_final"] = True
                return
        return
    want = min(left, 16 * page)
    if job["mode"] == "fill":
        got = ring.fill(sid, job["seed"], job["kind"], want, final=(want == left))
    else:
        got = ring.fill_pieces(sid, np.array(job["rows"], dtype=np.uint64) if a["off"] == 0 else None, want, final=(want == left))
    a["off"] += got
    a["sent_final"] = got == want and want == left


def _drive(eng, ring, jobs, on_records=None, any_stream=False, concurrent=None, between=None, timeout_s=240.0):
    """All jobs through the ring; on_records(job index of each record, records) after every poll that brought some (it
    encodes and releases on a holding ring). Returns one record array per job."""
    from pbs_plus_amd import RECORD_DTYPE

    page = ring.page_bytes
    res = [[] for _ in jobs]
    todo, active = list(range(len(jobs))), {}
    limit = concurrent or len(jobs)
    t0 = time.time()
    while todo or active:
        while todo and len(active) < limit:
            sid = ring.open()
            j = todo.pop(0)
            active[sid] = dict(j=j, off=0, sent_final=False)
            for b in jobs[j].get("sugg", ()):
                ring.suggest(sid, int(b))
        for sid, a in active.items():
            _feed(eng, ring, sid, jobs[a["j"]], a, page)
        ring.pump()
        if between is not None:
            between()
        finished = []
        if any_stream:
            recs, fins = ring.poll_any()
            if recs.size:
                js = np.array([active[int(s)]["j"] for s in recs["segment"] & SID_MASK])
                for j in np.unique(js):
                    res[j].append(recs[js == j].copy())
                if on_records:
                    on_records(None, js, recs)
            finished = [int(s) for s in fins]
        else:
            for sid in list(active):
                recs, fin = ring.poll(sid)
                if recs.size:
                    res[active[sid]["j"]].append(recs.copy())
                    if on_records:
                        on_records(sid, np.full(recs.size, active[sid]["j"]), recs)
                if fin:
                    finished.append(sid)
        for sid in finished:
            ring.close_stream(sid)
            del active[sid]
        assert time.time() - t0 < timeout_s, ("the ring did not finish", ring.stats(), ring.debug())
    return [np.concatenate(r) if r else np.zeros(0, dtype=RECORD_DTYPE) for r in res]


class _Checker:
    """encode every polled record, compare every blob, release"""

    def __init__(self, ring, hosts):
        self.ring, self.hosts = ring, hosts
        self.seen = set()          # (job, end) of every record encoded and compared
        self.src_align, self.dst_align = set(), set()
        self.nblob = self.nbytes = 0

    def __call__(self, sid, js, recs):
        dst, offs, crcs = self.ring.blob_encode(sid, recs)
        assert dst.used == int(recs["size"].astype(np.uint64).sum()) + 12 * recs.size
        out = dst.download(0, dst.used)
        dst.free()
        ends = recs["end"].astype(np.int64)
        sizes = recs["size"].astype(np.int64)
        assert np.array_equal(offs.astype(np.int64), np.concatenate([[0], np.cumsum(sizes + 12)[:-1]]))
        for i in range(recs.size):
            j, e, n, o = int(js[i]), int(ends[i]), int(sizes[i]), int(offs[i])
            b = out[o:o + 12 + n].tobytes()
            want = self.hosts[j][e - n:e].tobytes()
            what = (j, e, n)
            assert b[:8] == MAGIC, what
            c = zlib.crc32(want)
            assert int.from_bytes(b[8:12], "little") == c == int(crcs[i]), what
            assert b[12:] == want, what
            assert hashlib.sha256(b[12:]).digest() == recs["digest"][i].tobytes(), what
            self.seen.add((j, e))
            self.src_align.add((e - n) % 16)
            self.dst_align.add((o + 12) % 16)
        self.nblob += recs.size
        self.nbytes += dst.used
        # done with everything polled: the pages below go back
        if sid is not None:
            self.ring.release(sid, int(ends[-1]))
        else:
            sids = recs["segment"] & SID_MASK
            for s in np.unique(sids):
                self.ring.release(int(s), int(ends[sids == s].max()))


def _crossing(want, page):
    """(end, bytes in the first page, bytes in the second) of the chunks whose first and last byte lie in different pages"""
    ends = want["end"].astype(np.int64)
    starts = ends - want["size"].astype(np.int64)
    m = (starts // page) != ((ends - 1) // page)
    seam = (ends[m] - 1) // page * page
    return [(int(e), int(k - s), int(e - k)) for e, s, k in zip(ends[m], starts[m], seam)]


def _seam_suggestions(n, page, cmin):
    """cuts asked for 1, 2, 3 bytes in front of and behind page seams (each where the chunker's minimum allows it): chunks
    whose first part, or last part, is 1-3 bytes"""
    out = []
    for k in range(1, (n - 1) // page + 1):
        d = (k - 1) % 6
        out.append(k * page - 1 - d if d < 3 else k * page + d - 2)
    return [b for b in out if cmin < b < n]


def _oracle(O, cfg, host, sugg):
    if host.size == 0:
        return np.zeros(0, dtype=O.RECORD_DTYPE)
    if sugg:
        return O.chunk_and_digest_suggested(cfg, host, [(0, host.size)], [sugg])
    return O.chunk_and_digest(cfg, host, [(0, host.size)])


@pytest.mark.parametrize("avg,ring_opt,sizes,any_stream", [
    (4 << 20, dict(arena_bytes=256 << 20, max_streams=4), [(1 << 30) + 5, (96 << 20) + 16 * 3, (64 << 20) + 1], False),
    (4096, dict(arena_bytes=960 * (65536 + 256), page_bytes=65536, max_streams=4, sha_cus=32, round_pages=64),
     [(256 << 20) + 7, (24 << 20) + 16 * 5, (16 << 20) + 3], True),
])
def test_blobs_out_of_ring_pages_are_bit_exact(gpu_lib, O, avg, ring_opt, sizes, any_stream):
    """Three streams (random with cuts asked for around the seams, edited, random with zero extents) through a holding
    ring a quarter of the long stream's size or less: every polled record is framed out of the pages and compared."""
    from pbs_plus_amd import PageRing

    eng = _engine(avg)
    cfg = O.new_config(avg)
    rng = np.random.default_rng(avg)
    jobs = [dict(mode="fill", seed=101, kind=0, n=sizes[0]),
            dict(mode="pieces", rows=_edited_rows(rng, sizes[1]), n=sizes[1]),
            dict(mode="fill", seed=103, kind=3, n=sizes[2])]
    hosts = [_generator_bytes(eng, j) for j in jobs]
    ring = PageRing(eng, hold=True, **ring_opt)
    page = ring.page_bytes
    assert ring_opt["arena_bytes"] * 4 <= sizes[0]
    jobs[0]["sugg"] = _seam_suggestions(sizes[0], page, int(cfg.min))
    want = [_oracle(O, cfg, h, j.get("sugg")) for h, j in zip(hosts, jobs)]
    # what the cut list makes of the seams, before anything runs: one crossing chunk per interior seam no cut falls on
    cross = [_crossing(w, page) for w in want]
    for w, c, n in zip(want, cross, sizes):
        on_seam = int(((w["end"] % page == 0) & (w["end"] < n)).sum())
        assert len(c) == (n - 1) // page - on_seam
    assert sum(len(c) for c in cross) >= 32
    firsts = {l1 for c in cross for _, l1, _ in c}
    lasts = {l2 for c in cross for _, _, l2 in c}
    assert {1, 2, 3} <= firsts and {1, 2, 3} <= lasts, (sorted(firsts)[:6], sorted(lasts)[:6])
    chk = _Checker(ring, hosts)
    got = _drive(eng, ring, jobs, chk, any_stream=any_stream)
    ring.quiesce()
    st = ring.stats()
    assert st["pages_free"] == st["pages_total"], st                     # close released what was left
    assert st["pages_enqueued"] >= 4 * st["pages_total"], st             # the arena turned over
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.size == w.size and np.array_equal(g["end"], w["end"]) and np.array_equal(g["size"], w["size"]), j
        assert np.array_equal(g["digest"], w["digest"]), j
        assert {(j, int(e)) for e in w["end"]} <= chk.seen, j            # every record was encoded and compared ...
        assert {(j, e) for e, _, _ in cross[j]} <= chk.seen, j           # ... the seam-crossing ones among them
    assert chk.nblob == sum(w.size for w in want)
    assert chk.src_align == set(range(16)) and chk.dst_align == set(range(16))
    ring.close()
    # the same streams through a ring without the flag: the same records
    plain = PageRing(eng, **ring_opt)
    got2 = _drive(eng, plain, jobs, any_stream=any_stream)
    plain.quiesce()
    for g, g2 in zip(got, got2):
        assert g.size == g2.size and np.array_equal(g["end"], g2["end"]) and np.array_equal(g["digest"], g2["digest"])
    plain.close()
    eng.close()
    print(f"ring upload avg={avg}: {chk.nblob} blobs, {chk.nbytes} bytes, {sum(len(c) for c in cross)} of them out of two pages")


def test_planted_seam_cases_are_framed_exactly(gpu_lib, O):
    """The streams of tests/seam_inputs.py at NewConfig(4096), 64 KiB pages: chunks with 1..68 bytes before a seam and a
    second piece of 0..8 or 52..72 bytes, every start alignment, chunks that end on a seam, tiny streams — fed from the
    host through a holding ring of 48 pages, every record framed and compared with the planted bytes."""
    from pbs_plus_amd import PageRing

    cfg, page, streams = S.plan(O, 4096)
    eng = _engine(4096)
    ring = PageRing(eng, hold=True, arena_bytes=48 * (page + 256), page_bytes=page, max_streams=8, sha_cus=8, round_pages=8)
    jobs = [dict(mode="host", data=d, n=int(d.size)) for d, _ in streams]
    hosts = [d for d, _ in streams]
    chk = _Checker(ring, hosts)
    got = _drive(eng, ring, jobs, chk, concurrent=8)
    ring.quiesce()
    ncross, parts = 0, set()
    for j, ((d, ends), g) in enumerate(zip(streams, got)):
        assert np.array_equal(g["end"], ends), j
        cr, _, _ = S.census(ends, page)
        ncross += len(cr)
        parts |= {(l1, p2) for l1, p2, _, _ in cr}
        assert {(j, int(e)) for e in ends} <= chk.seen
    assert ncross >= 32 and {l for l, _ in parts} >= set(range(1, 69)) and {p for _, p in parts} >= {1, 2, 3}
    st = ring.stats()
    assert st["pages_free"] == st["pages_total"], st
    ring.close()
    eng.close()


def _held_ring(avg=65536, page=262144, pages=64, n=(6 << 20) + 11, **opt):
    """a holding ring that has taken a whole stream and released nothing: (engine, ring, stream, records, bytes)"""
    from pbs_plus_amd import PageRing

    eng = _engine(avg)
    job = dict(mode="fill", seed=31, kind=0, n=n)
    host = _generator_bytes(eng, job)
    ring = PageRing(eng, arena_bytes=pages * (page + 256), page_bytes=page, max_streams=2, sha_cus=8, round_pages=8, **opt)
    sid = ring.open()
    a = dict(off=0, sent_final=False)
    recs, fin, t0 = [], False, time.time()
    while not fin:
        _feed(eng, ring, sid, job, a, page)
        ring.pump()
        r, fin = ring.poll(sid)
        recs.append(r.copy())
        assert time.time() - t0 < 60, ring.debug()
    return eng, ring, sid, np.concatenate(recs), host


def _guarded(eng, nbytes):
    g = eng.alloc(nbytes + 128)
    g.upload(np.full(nbytes + 128, 0xA5, dtype=np.uint8))
    return g


def test_lifecycle_hold_stall_release_resume_close(gpu_lib, O):
    """An arena an eighth of the stream: without a release the ring stops taking bytes (fill takes 0, reserve is BUSY), held()
    shows the pages and every polled record is still encodable; release brings the pages back and the stream runs to its
    end; a record below the watermark's page is E_STATE with nothing written; close frees what is left."""
    import ctypes as C

    from pbs_plus_amd import PageRing, PbsGpuError, _lib

    avg, page, pages, n = 65536, 262144, 16, (32 << 20) + 77
    eng = _engine(avg)
    cfg = O.new_config(avg)
    job = dict(mode="fill", seed=41, kind=0, n=n)
    host = _generator_bytes(eng, job)
    want = _oracle(O, cfg, host, None)
    ring = PageRing(eng, hold=True, arena_bytes=pages * (page + 256), page_bytes=page, max_streams=2, sha_cus=8, round_pages=4)
    assert ring.stats()["pages_total"] * page * 8 <= n
    sid = ring.open()
    a = dict(off=0, sent_final=False)
    recs, idle_since = [], None
    t0 = time.time()
    while True:                                    # feed without releasing until nothing moves any more
        before = a["off"]
        _feed(eng, ring, sid, job, a, page)
        ring.pump()
        r, fin = ring.poll(sid)
        assert not fin
        if r.size:
            recs.append(r.copy())
        if r.size or a["off"] != before:
            idle_since = None
        elif idle_since is None:
            idle_since = time.time()
        elif time.time() - idle_since > 1.0:
            break
        assert time.time() - t0 < 60, ring.debug()
    recs = np.concatenate(recs)
    assert a["off"] <= pages * page and a["off"] < n                     # the arena's worth, no more
    assert ring.fill(sid, 41, 0, page, final=False) == 0
    assert ring.reserve(sid) is None                                     # PBSGPU_E_BUSY
    first, nheld = ring.held(sid)
    st = ring.stats()
    assert first == 0 and nheld >= pages - 3 and st["pages_free"] == 0, (first, nheld, st)
    assert np.array_equal(recs["end"], want["end"][:recs.size]) and recs.size > 32
    chk = _Checker(ring, [host])
    ring_release, ring.release = ring.release, lambda *args: None        # compare everything polled, release nothing yet
    chk(sid, np.zeros(recs.size, dtype=np.int64), recs)
    ring.release = ring_release
    assert chk.nblob == recs.size and ring.held(sid) == (0, nheld)
    # the watermark: not beyond what was polled, never backwards
    last = int(recs["end"][-1])
    with pytest.raises(PbsGpuError) as ei:
        ring.release(sid, last + 1)
    assert ei.value.status == _lib.E_INVALID
    mid = int(recs["end"][recs.size // 2])
    ring.release(sid, mid)
    first, nheld2 = ring.held(sid)
    assert first == mid // page * page and nheld2 == nheld - mid // page
    ring.release(sid, mid // 2)                                          # lower: a no-op
    assert ring.held(sid) == (first, nheld2)
    assert ring.stats()["pages_free"] == mid // page
    # a record that begins below the watermark's page is gone: E_STATE, nothing written; the ones from that page on are not
    L = eng._L
    gone = recs[(recs["end"] - recs["size"]) < first]
    kept = recs[(recs["end"] - recs["size"]) >= first]
    assert gone.size and kept.size
    for batch in (gone[-1:], np.concatenate([kept[:3], gone[:1]])):
        g = _guarded(eng, int(batch["size"].sum()) + 12 * batch.size)
        offs, used = np.zeros(batch.size, dtype=np.uint64), C.c_uint64()
        stt = L.pbsgpu_ring_blob_encode_device(ring._h, sid, batch.ctypes.data, batch.size, None, g.ptr + 64, g.nbytes - 128,
                                               offs.ctypes.data, None, C.byref(used))
        assert stt == _lib.E_STATE
        assert np.all(g.download() == 0xA5)
        g.free()
    with pytest.raises(PbsGpuError) as ei:
        ring.copy(sid, first - 1, 100)
    assert ei.value.status == _lib.E_STATE
    with pytest.raises(PbsGpuError) as ei:
        ring.copy(sid, last - 10, 11)                                    # beyond what was polled
    assert ei.value.status == _lib.E_STATE
    chk2 = _Checker(ring, [host])
    ring.release = lambda *args: None
    chk2(sid, np.zeros(kept.size, dtype=np.int64), kept)
    ring.release = ring_release
    # release and go on to the end, releasing after every poll
    ring.release(sid, last)
    rest = []
    fin = False
    t0 = time.time()
    while not fin:
        _feed(eng, ring, sid, job, a, page)
        ring.pump()
        r, fin = ring.poll(sid)
        if r.size:
            rest.append(r.copy())
            chk2(sid, np.zeros(r.size, dtype=np.int64), r)
        assert time.time() - t0 < 120, ring.debug()
    got = np.concatenate([recs] + rest)
    assert got.size == want.size and np.array_equal(got["end"], want["end"]) and np.array_equal(got["digest"], want["digest"])
    first, nheld = ring.held(sid)
    assert first == n // page * page and nheld >= 1                      # the short last page stays until close
    ring.close_stream(sid)
    ring.quiesce()
    st = ring.stats()
    assert st["pages_free"] == st["pages_total"] == pages, st
    ring.close()
    eng.close()


def test_a_too_small_destination_is_capacity_with_the_size_needed(gpu_lib):
    import ctypes as C

    from pbs_plus_amd import _lib

    eng, ring, sid, recs, host = _held_ring(hold=True)
    need = int(recs["size"].sum()) + 12 * recs.size
    L = eng._L
    for cap in (need - 1, 12, 0):
        g = _guarded(eng, need)
        offs, used = np.full(recs.size, 7, dtype=np.uint64), C.c_uint64()
        st = L.pbsgpu_ring_blob_encode_device(ring._h, sid, recs.ctypes.data, recs.size, None, g.ptr + 64, cap, offs.ctypes.data,
                                              None, C.byref(used))
        assert st == _lib.E_CAPACITY and used.value == need
        assert np.all(g.download() == 0xA5) and np.all(offs == 7)
        g.free()
    # exactly enough: everything inside, the guards intact; skipped records leave their outputs alone
    skip = (np.arange(recs.size) % 3 == 1).astype(np.uint8)
    need2 = int(recs["size"][skip == 0].sum()) + 12 * int((skip == 0).sum())
    g = _guarded(eng, need2)
    offs, crcs, used = np.full(recs.size, 7, dtype=np.uint64), np.full(recs.size, 9, dtype=np.uint32), C.c_uint64()
    st = L.pbsgpu_ring_blob_encode_device(ring._h, sid, recs.ctypes.data, recs.size, skip.ctypes.data, g.ptr + 64, need2,
                                          offs.ctypes.data, crcs.ctypes.data, C.byref(used))
    assert st == 0 and used.value == need2
    out = g.download()
    assert np.all(out[:64] == 0xA5) and np.all(out[64 + need2:] == 0xA5)
    assert np.all(offs[skip == 1] == 7) and np.all(crcs[skip == 1] == 9)
    pos = 0
    for i in np.nonzero(skip == 0)[0]:
        e, n = int(recs["end"][i]), int(recs["size"][i])
        assert int(offs[i]) == pos
        data = host[e - n:e].tobytes()
        assert out[64 + pos:64 + pos + 12 + n].tobytes() == MAGIC + zlib.crc32(data).to_bytes(4, "little") + data
        assert int(crcs[i]) == zlib.crc32(data)
        pos += 12 + n
    g.free()
    ring.close_stream(sid)
    ring.close()
    eng.close()


def test_the_whole_incremental_loop(gpu_lib, O):
    """1 GiB at NewConfig(4 MiB) through a holding ring of 256 MiB, half of the digests already known: per poll classify,
    frame the new chunks only, verify the blobs against the records, release. The ring finishes; what was framed is what
    classify called new."""
    from pbs_plus_amd import KnownChunks, PageRing

    avg, n = 4 << 20, (1 << 30) + 5
    eng = _engine(avg)
    job = dict(mode="fill", seed=101, kind=0, n=n)
    host = _generator_bytes(eng, job)
    want = _oracle(O, O.new_config(avg), host, None)
    known = KnownChunks(eng)
    known.add(want[::2])
    ring = PageRing(eng, hold=True, arena_bytes=256 << 20, max_streams=2)
    tot = dict(unique_bytes=0, blobs=0, encoded=0, ok=0, polls=0)

    def on_records(sid, js, recs):
        flags, st = known.classify(recs, insert=True)
        new = recs[flags == 0]
        dst, offs, crcs = ring.blob_encode(sid, recs, skip=flags)
        if new.size:
            blobs = np.stack([offs[flags == 0], new["size"].astype(np.uint64) + 12], axis=1)
            status, vst = eng.blob_verify(dst, blobs, digests=new["digest"], sizes=new["size"], nbytes=dst.used)
            assert np.all(status == 0), status
            tot["ok"] += vst["ok"]
        tot["unique_bytes"] += st["unique_bytes"]
        tot["blobs"] += int(new.size)
        tot["encoded"] += dst.used
        tot["polls"] += 1
        dst.free()
        ring.release(sid, int(recs["end"][-1]))

    got = _drive(eng, ring, [job], on_records)[0]
    ring.quiesce()
    assert got.size == want.size and np.array_equal(got["end"], want["end"]) and np.array_equal(got["digest"], want["digest"])
    assert tot["blobs"] == want.size - want[::2].size == tot["ok"]
    assert tot["unique_bytes"] == int(want["size"][1::2].astype(np.uint64).sum())
    assert tot["encoded"] == tot["unique_bytes"] + 12 * tot["blobs"]
    st = ring.stats()
    assert st["pages_free"] == st["pages_total"] and st["pages_enqueued"] >= 4 * st["pages_total"], st
    assert tot["polls"] > 4
    known.close()
    ring.close()
    eng.close()


def test_encode_and_copy_beside_the_running_services(gpu_lib, O):
    """Two streams on a holding ring; between pumps, while the services run, polled records of the first are framed again
    and ranges of it copied out. Both exact every time, and the ring's records still equal the oracle's."""
    from pbs_plus_amd import PageRing

    avg, page = 65536, 262144
    eng = _engine(avg)
    cfg = O.new_config(avg)
    jobs = [dict(mode="fill", seed=51, kind=0, n=(96 << 20) + 5), dict(mode="fill", seed=52, kind=3, n=(64 << 20) + 77)]
    hosts = [_generator_bytes(eng, j) for j in jobs]
    want = [_oracle(O, cfg, h, None) for h in hosts]
    ring = PageRing(eng, hold=True, arena_bytes=96 * (page + 256), page_bytes=page, max_streams=2, sha_cus=16, round_pages=8)
    state = dict(recs=None, sid=None, runs=0)
    rng = np.random.default_rng(9)
    chk = _Checker(ring, hosts)

    def on_records(sid, js, recs):
        if js[0] == 0:
            ring.release(sid, int(recs["end"][0] - recs["size"][0]))     # what came before this poll has had its turn
            if int(recs["end"][-1]) == jobs[0]["n"]:                     # the stream's last records: it is closed after this poll
                chk(sid, js, recs)
            else:
                state["recs"], state["sid"] = recs.copy(), sid           # not released: still there after the next pump
        else:
            chk(sid, js, recs)

    def between():
        if state["recs"] is None or ring.stats()["service_launches"] < 1:
            return
        recs, sid = state["recs"], state["sid"]
        rel, ring.release = ring.release, lambda *args: None
        chk(sid, np.zeros(recs.size, dtype=np.int64), recs)
        ring.release = rel
        lo, hi = int(recs["end"][0] - recs["size"][0]), int(recs["end"][-1])
        o = int(rng.integers(lo, hi))
        ln = int(rng.integers(1, min(hi - o, 3 * page) + 1))
        buf = ring.copy(sid, o, ln)
        assert buf.download(0, ln).tobytes() == hosts[0][o:o + ln].tobytes(), (o, ln)
        buf.free()
        state["runs"] += 1
        state["recs"] = None

    got = _drive(eng, ring, jobs, on_records, between=between)
    ring.quiesce()
    assert state["runs"] >= 4
    for g, w in zip(got, want):
        assert g.size == w.size and np.array_equal(g["end"], w["end"]) and np.array_equal(g["digest"], w["digest"])
    st = ring.stats()
    assert st["pages_free"] == st["pages_total"], st
    ring.close()
    eng.close()


def test_without_the_flag_every_call_is_a_state_error(gpu_lib):
    from pbs_plus_amd import PbsGpuError, _lib

    eng, ring, sid, recs, host = _held_ring(n=(1 << 20) + 3)
    for call in (lambda: ring.release(sid, 0), lambda: ring.held(sid), lambda: ring.blob_encode(sid, recs),
                 lambda: ring.copy(sid, 0, 100)):
        with pytest.raises(PbsGpuError) as ei:
            call()
        assert ei.value.status == _lib.E_STATE
    ring.close_stream(sid)
    ring.quiesce()
    st = ring.stats()
    assert st["pages_free"] == st["pages_total"]
    ring.close()
    eng.close()
