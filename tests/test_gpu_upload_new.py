"""Classify and frame in one device-side call (PageRing.upload_new / KnownChunks.upload_new).

The yardstick is always the unchanged two-call path on a twin set: two KnownChunks seeded identically, one taken through
classify + blob_encode(skip = known), the other through the fused call; every output is compared for equality, and so is
len(set) afterwards. Beside it an independent check: the flags against a Python set of digests, every new record's blob
against the generator's bytes, zlib.crc32 and hashlib."""
import ctypes as C
import hashlib
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seam_inputs as S  # noqa: E402
from test_gpu_ring_upload import (MAGIC, SID_MASK, _drive, _engine, _generator_bytes, _guarded, _held_ring, _oracle,  # noqa: E402
                                  _seam_suggestions)

pytestmark = pytest.mark.gpu
PIECE = 1 << 16


@pytest.fixture(autouse=True)
def _short_idle_timeout(monkeypatch):
    monkeypatch.setenv("PBSGPU_RING_IDLE_TIMEOUT_S", "10")


def _stats(st):
    from pbs_plus_amd import _lib

    return {k: int(getattr(st, k)) for k, _ in _lib.DedupStats._fields_}


def _raw(ring, known, sid, recs, insert, ptr, cap):
    """the C call with outputs pre-set to sentinels: (status, flags, offsets, crcs, used, stats)"""
    from pbs_plus_amd import _lib

    n = int(recs.size)
    flags = np.full(max(n, 1), 9, dtype=np.uint8)
    offs = np.full(max(n, 1), 7, dtype=np.uint64)
    crcs = np.full(max(n, 1), 9, dtype=np.uint32)
    used, st = C.c_uint64(123), _lib.DedupStats()
    rc = ring._L.pbsgpu_ring_upload_new_device(ring._h, known._h, _lib.RING_ANY_STREAM if sid is None else sid,
                                               recs.ctypes.data if n else None, n, int(insert), ptr, cap, flags.ctypes.data,
                                               offs.ctypes.data, crcs.ctypes.data, C.byref(used), C.byref(st))
    return rc, flags[:n], offs[:n], crcs[:n], int(used.value), _stats(st)


def _parts(recs, page):
    """(bytes in the first page, bytes in the second) of every record"""
    ends = recs["end"].astype(np.int64)
    sizes = recs["size"].astype(np.int64)
    starts = ends - sizes
    first = np.minimum(sizes, page - starts % page)
    return first, sizes - first


class _Twins:
    """two sets seeded identically + the model; check() runs one batch through both paths and compares everything"""

    def __init__(self, eng, seed=None, capacity=0):
        from pbs_plus_amd import KnownChunks

        self.fused, self.twin, self.model = KnownChunks(eng, capacity), KnownChunks(eng, capacity), set()
        if seed is not None and seed.size:
            self.fused.add(seed)
            self.twin.add(seed)
            self.model |= {d.tobytes() for d in seed["digest"]}
        self.nnew = self.nknown = self.ndup = 0
        self.firsts, self.lasts = set(), set()
        self.multi = 0

    def close(self):
        self.fused.close()
        self.twin.close()

    def check(self, ring, sid, recs, bytes_of, insert=True):
        recs = np.ascontiguousarray(recs)
        flags2, st2 = self.twin.classify(recs, insert=insert)
        dst2, offs2, crcs2 = ring.blob_encode(sid, recs, skip=flags2)
        out2 = dst2.download(0, dst2.used) if dst2.used else np.zeros(0, dtype=np.uint8)
        used2 = dst2.used
        dst2.free()
        dst, flags, offs, crcs, st = ring.upload_new(self.fused, sid, recs, insert=insert)
        out = dst.download(0, dst.used) if dst.used else np.zeros(0, dtype=np.uint8)
        used = dst.used
        dst.free()
        assert np.array_equal(flags, flags2)
        assert st == st2, (st, st2)
        assert used == used2
        assert np.array_equal(offs, offs2) and np.array_equal(crcs, crcs2)
        assert out.tobytes() == out2.tobytes()
        assert len(self.fused) == len(self.twin)
        # the independent check
        seen, pos = set(), 0
        first, second = _parts(recs, ring.page_bytes)
        for i in range(recs.size):
            d = recs["digest"][i].tobytes()
            known = d in self.model or d in seen
            assert int(flags[i]) == int(known), i
            if d in seen and d not in self.model:
                self.ndup += 1
            seen.add(d)
            if known:
                self.nknown += 1
                assert offs[i] == 0 and crcs[i] == 0
                continue
            n = int(recs["size"][i])
            data = bytes_of(i)
            assert len(data) == n and int(offs[i]) == pos, i
            crc = zlib.crc32(data)
            assert out[pos:pos + 12 + n].tobytes() == MAGIC + crc.to_bytes(4, "little") + data, i
            assert int(crcs[i]) == crc and hashlib.sha256(data).digest() == d, i
            pos += 12 + n
            self.nnew += 1
            self.multi += n > PIECE
            if second[i]:
                self.firsts.add(int(first[i]))
                self.lasts.add(int(second[i]))
        assert pos == used
        if insert:
            self.model |= seen
        assert len(self.fused) == len(self.model)
        return flags


def _on_records(tw, ring, hosts, insert=True):
    """for _drive: compare every polled batch, then release what it covered"""
    def on_records(sid, js, recs):
        ends, sizes = recs["end"].astype(np.int64), recs["size"].astype(np.int64)
        tw.check(ring, sid, recs, lambda i: hosts[int(js[i])][ends[i] - sizes[i]:ends[i]].tobytes(), insert=insert)
        sids = np.full(recs.size, sid) if sid is not None else recs["segment"] & SID_MASK
        for s in np.unique(sids):
            ring.release(int(s), int(ends[sids == s].max()))
    return on_records


def _single(host, recs):
    ends, sizes = recs["end"].astype(np.int64), recs["size"].astype(np.int64)
    return lambda i: host[ends[i] - sizes[i]:ends[i]].tobytes()


def test_multi_piece_chunks_and_straddlers(gpu_lib):
    """About a hundred chunks of up to 256 KiB in 256 KiB pages, every other digest known: several pieces per chunk, about
    one in four in two pages. A second call on the same records then finds everything known and writes nothing."""
    eng, ring, sid, recs, host = _held_ring(avg=65536, page=262144, pages=64, n=(6 << 20) + 11, hold=True)
    tw = _Twins(eng, recs[::2])
    tw.check(ring, sid, recs, _single(host, recs), insert=True)
    assert tw.nnew >= 30 and tw.multi >= 10 and len(tw.firsts) >= 5, (tw.nnew, tw.multi, tw.firsts)
    g = _guarded(eng, 4096)
    rc, flags, offs, crcs, used, st = _raw(ring, tw.fused, sid, recs, 1, g.ptr + 64, 4096)
    assert rc == 0 and used == 0 and np.all(flags == 1) and np.all(offs == 7) and np.all(crcs == 9)
    assert st["nunique"] == 0 and st["nrecords"] == recs.size
    assert np.all(g.download() == 0xA5)
    assert len(tw.fused) == len(tw.twin)
    g.free()
    tw.close()
    ring.close_stream(sid)
    ring.close()
    eng.close()


def test_small_chunks_short_parts_and_duplicates_inside_a_batch(gpu_lib, O):
    """NewConfig(4096), 64 KiB pages: a zero-extent stream of 8 MiB + 13 with cuts asked for 1-3 bytes around the seams,
    and the planted streams of seam_inputs.py: first and last parts of 1, 2 and 3 bytes among the NEW chunks, and batches
    that hold duplicates of their own (first occurrence new, the rest known)."""
    from pbs_plus_amd import PageRing

    cfg, page, streams = S.plan(O, 4096)
    eng = _engine(4096)
    n = (8 << 20) + 13
    jobs = [dict(mode="fill", seed=103, kind=3, n=n, sugg=_seam_suggestions(n, page, int(cfg.min)))]
    hosts = [_generator_bytes(eng, jobs[0])]
    jobs += [dict(mode="host", data=d, n=int(d.size)) for d, _ in streams]
    hosts += [d for d, _ in streams]
    want = _oracle(O, cfg, hosts[0], jobs[0]["sugg"])
    # every other digest is known beforehand, but none of the repeated ones (the chunks of the zero extents): their first
    # occurrence is new, and the ones behind it in the same batch are known only because of it
    _, inv, cnt = np.unique(want["digest"], axis=0, return_inverse=True, return_counts=True)
    once = cnt[inv.reshape(-1)] == 1
    assert int((~once).sum()) > 100
    tw = _Twins(eng, want[once][::2])
    ring = PageRing(eng, hold=True, arena_bytes=256 * (page + 256), page_bytes=page, max_streams=8, sha_cus=8, round_pages=8)
    got = _drive(eng, ring, jobs, _on_records(tw, ring, hosts), concurrent=8)
    ring.quiesce()
    assert np.array_equal(got[0]["end"], want["end"]) and np.array_equal(got[0]["digest"], want["digest"])
    for (d, ends), g in zip(streams, got[1:]):
        assert np.array_equal(g["end"], ends)
    assert tw.nnew + tw.nknown == sum(g.size for g in got)
    assert {1, 2, 3} <= tw.firsts and {1, 2, 3} <= tw.lasts, (sorted(tw.firsts)[:8], sorted(tw.lasts)[:8])
    assert tw.ndup > 0
    st = ring.stats()
    assert st["pages_free"] == st["pages_total"], st
    tw.close()
    ring.close()
    eng.close()


def test_tiny_streams(gpu_lib):
    """streams of 1, 2, 3 and 5 bytes: chunks under 4 bytes take the init term in the fold"""
    from pbs_plus_amd import PageRing

    eng = _engine(4096)
    rng = np.random.default_rng(5)
    hosts = [rng.integers(0, 256, size=n, dtype=np.uint8) for n in (1, 2, 3, 5)]
    jobs = [dict(mode="host", data=d, n=int(d.size)) for d in hosts]
    ring = PageRing(eng, hold=True, arena_bytes=16 * (65536 + 256), page_bytes=65536, max_streams=4, sha_cus=8, round_pages=4)
    tw = _Twins(eng)
    got = _drive(eng, ring, jobs, _on_records(tw, ring, hosts), any_stream=True)
    ring.quiesce()
    assert [int(g["size"].sum()) for g in got] == [1, 2, 3, 5] and tw.nnew == 4
    tw.close()
    ring.close()
    eng.close()


def test_degenerate_batches(gpu_lib):
    """n = 0, all known, all new"""
    eng, ring, sid, recs, host = _held_ring(n=(1 << 20) + 3, hold=True)
    tw = _Twins(eng)
    tw.check(ring, sid, recs[:0], _single(host, recs[:0]))
    rc, flags, offs, crcs, used, st = _raw(ring, tw.fused, sid, recs[:0], 1, None, 0)
    assert rc == 0 and used == 0 and st == dict(nrecords=0, nunique=0, total_bytes=0, unique_bytes=0)
    both = np.concatenate([recs, recs[::3]])                             # a batch with duplicates of its own
    tw2 = _Twins(eng)
    tw2.check(ring, sid, both, _single(host, both), insert=False)
    assert tw2.ndup == recs[::3].size == tw2.nknown and tw2.nnew == recs.size and len(tw2.fused) == 0
    tw2.close()
    tw.check(ring, sid, recs, _single(host, recs))                       # all new
    assert tw.nnew == recs.size and tw.nknown == 0
    tw.check(ring, sid, recs, _single(host, recs))                       # all known
    assert tw.nnew == recs.size and tw.nknown == recs.size
    rc, flags, offs, crcs, used, st = _raw(ring, tw.fused, sid, recs, 1, None, 0)  # ... which needs no destination
    assert rc == 0 and used == 0 and np.all(flags == 1)
    tw.close()
    ring.close_stream(sid)
    ring.close()
    eng.close()


def test_any_stream(gpu_lib, O):
    """three streams polled with poll_any: every record's stream is its segment"""
    from pbs_plus_amd import PageRing

    avg, page = 65536, 262144
    eng = _engine(avg)
    jobs = [dict(mode="fill", seed=61, kind=0, n=(3 << 20) + 5), dict(mode="fill", seed=62, kind=3, n=(2 << 20) + 77),
            dict(mode="fill", seed=63, kind=0, n=(1 << 20) + 1)]
    hosts = [_generator_bytes(eng, j) for j in jobs]
    want = [_oracle(O, O.new_config(avg), h, None) for h in hosts]
    tw = _Twins(eng, np.concatenate([w[1::2] for w in want]))
    ring = PageRing(eng, hold=True, arena_bytes=48 * (page + 256), page_bytes=page, max_streams=4, sha_cus=8, round_pages=8)
    mixed = []

    def on_records(sid, js, recs):
        mixed.append(np.unique(js).size)
        _on_records(tw, ring, hosts)(sid, js, recs)

    got = _drive(eng, ring, jobs, on_records, any_stream=True)
    ring.quiesce()
    for g, w in zip(got, want):
        assert np.array_equal(g["end"], w["end"]) and np.array_equal(g["digest"], w["digest"])
    assert max(mixed) >= 2 and tw.nnew > 0 and tw.nknown > 0
    tw.close()
    ring.close()
    eng.close()


def test_capacity_leaves_destination_and_set_untouched(gpu_lib):
    from pbs_plus_amd import _lib

    eng, ring, sid, recs, host = _held_ring(hold=True)
    tw = _Twins(eng, recs[::2])
    want_flags, want_st = tw.twin.classify(recs, insert=False)
    needed = int(recs["size"][want_flags == 0].astype(np.uint64).sum()) + 12 * int((want_flags == 0).sum())
    before = len(tw.fused)
    g = _guarded(eng, needed)
    rc, flags, offs, crcs, used, st = _raw(ring, tw.fused, sid, recs, 1, g.ptr + 64, needed - 1)
    assert rc == _lib.E_CAPACITY and used == needed
    assert np.all(g.download() == 0xA5)
    assert len(tw.fused) == before
    assert np.array_equal(flags, want_flags) and st == want_st          # still valid: the caller can retry
    assert np.all(offs == 7) and np.all(crcs == 9)
    again, _ = tw.fused.classify(recs, insert=False)
    assert np.array_equal(again, want_flags)
    rc, flags, offs, crcs, used, st = _raw(ring, tw.fused, sid, recs, 1, g.ptr + 64, needed)
    assert rc == 0 and used == needed and np.array_equal(flags, want_flags) and st == want_st
    out = g.download()
    assert np.all(out[:64] == 0xA5) and np.all(out[64 + needed:] == 0xA5)
    tw.twin.classify(recs, insert=True)
    dst2, offs2, crcs2 = ring.blob_encode(sid, recs, skip=want_flags)
    assert dst2.used == needed and out[64:64 + needed].tobytes() == dst2.download(0, needed).tobytes()
    new = want_flags == 0
    assert np.array_equal(offs[new], offs2[new]) and np.array_equal(crcs[new], crcs2[new])
    assert np.all(offs[~new] == 7) and np.all(crcs[~new] == 9)
    assert len(tw.fused) == len(tw.twin) == before + int(new.sum())
    dst2.free()
    g.free()
    tw.close()
    ring.close_stream(sid)
    ring.close()
    eng.close()


def test_refusals_are_decided_before_any_device_work(gpu_lib):
    """a record below held()'s first offset, a record not yet polled, a chunk larger than a page, a host destination, a set
    of another engine, a ring without the flag: dst and the set untouched every time"""
    from pbs_plus_amd import KnownChunks, _lib

    eng, ring, sid, recs, host = _held_ring(hold=True)
    tw = _Twins(eng, recs[::2])
    before = len(tw.fused)
    ring.release(sid, int(recs["end"][recs.size // 2]))
    first, _ = ring.held(sid)
    starts = recs["end"] - recs["size"]
    gone, kept = recs[starts < first], recs[starts >= first]
    assert gone.size and kept.size
    late = kept[-1:].copy()
    late["end"] += 1
    huge = kept[-1:].copy()
    huge["size"] = ring.page_bytes + 1
    g = _guarded(eng, 1 << 20)
    cases = [(np.concatenate([kept[:3], gone[-1:]]), _lib.E_STATE), (gone[:1], _lib.E_STATE),
             (np.concatenate([kept[:2], late]), _lib.E_STATE), (huge, _lib.E_INVALID)]
    for batch, want in cases:
        rc, flags, offs, crcs, used, st = _raw(ring, tw.fused, sid, np.ascontiguousarray(batch), 1, g.ptr + 64, (1 << 20))
        assert rc == want, (rc, want)
        assert np.all(flags == 9) and np.all(offs == 7) and len(tw.fused) == before
    assert np.all(g.download() == 0xA5)
    hostbuf = np.zeros(1 << 20, dtype=np.uint8)
    rc = _raw(ring, tw.fused, sid, kept[:3], 1, hostbuf.ctypes.data, hostbuf.size)[0]
    assert rc == _lib.E_INVALID and not hostbuf.any() and len(tw.fused) == before
    eng2 = _engine(65536)
    other = KnownChunks(eng2)
    assert _raw(ring, other, sid, kept[:3], 1, g.ptr + 64, 1 << 20)[0] == _lib.E_INVALID
    other.close()
    eng2.close()
    tw.check(ring, sid, kept, _single(host, kept))                       # what is still held works as ever
    g.free()
    tw.close()
    ring.close_stream(sid)
    ring.close()
    eng.close()
    eng, ring, sid, recs, host = _held_ring(n=(1 << 20) + 3)            # no HOLD_PAGES
    known = KnownChunks(eng)
    g = _guarded(eng, 1 << 20)
    assert _raw(ring, known, sid, recs, 1, g.ptr + 64, 1 << 20)[0] == _lib.E_STATE
    assert len(known) == 0 and np.all(g.download() == 0xA5)
    g.free()
    known.close()
    ring.close_stream(sid)
    ring.quiesce()
    ring.close()
    eng.close()


def test_the_set_grows_inside_the_call(gpu_lib):
    """a set created for 16 digests takes a batch of about 2 000 new records"""
    eng, ring, sid, recs, host = _held_ring(avg=4096, page=65536, pages=192, n=(8 << 20) + 13, hold=True)
    assert recs.size >= 1500
    tw = _Twins(eng, capacity=16)
    tw.check(ring, sid, recs, _single(host, recs))
    assert len(tw.fused) == np.unique(recs["digest"], axis=0).shape[0] == tw.nnew
    again, _ = tw.fused.classify(recs, insert=False)
    assert np.all(again == 1)
    tw.close()
    ring.close_stream(sid)
    ring.close()
    eng.close()


def test_beside_the_running_services(gpu_lib, O):
    """Two streams on a holding ring; between pumps, while the services run, polled records of the first go through the
    fused call. Equal to the two-call path every time, and the ring's records still equal the oracle's."""
    from pbs_plus_amd import PageRing

    avg, page = 65536, 262144
    eng = _engine(avg)
    cfg = O.new_config(avg)
    jobs = [dict(mode="fill", seed=51, kind=0, n=(96 << 20) + 5), dict(mode="fill", seed=52, kind=3, n=(64 << 20) + 77)]
    hosts = [_generator_bytes(eng, j) for j in jobs]
    want = [_oracle(O, cfg, h, None) for h in hosts]
    ring = PageRing(eng, hold=True, arena_bytes=96 * (page + 256), page_bytes=page, max_streams=2, sha_cus=16, round_pages=8)
    tw = _Twins(eng, want[0][::2])
    state = dict(recs=None, sid=None, runs=0)

    def on_records(sid, js, recs):
        if js[0] == 0:
            ring.release(sid, int(recs["end"][0] - recs["size"][0]))     # what came before this poll has had its turn
            if int(recs["end"][-1]) != jobs[0]["n"]:
                state["recs"], state["sid"] = recs.copy(), sid           # not released: still there after the next pump
        else:
            ring.release(sid, int(recs["end"][-1]))

    def between():
        if state["recs"] is None or ring.stats()["service_launches"] < 1:
            return
        recs, sid = state["recs"], state["sid"]
        tw.check(ring, sid, recs, _single(hosts[0], recs))
        state["runs"] += 1
        state["recs"] = None

    got = _drive(eng, ring, jobs, on_records, between=between)
    ring.quiesce()
    assert state["runs"] >= 4 and tw.nnew > 0 and tw.nknown > 0
    for g, w in zip(got, want):
        assert g.size == w.size and np.array_equal(g["end"], w["end"]) and np.array_equal(g["digest"], w["digest"])
    st = ring.stats()
    assert st["pages_free"] == st["pages_total"], st
    tw.close()
    ring.close()
    eng.close()


def test_contiguous_form(gpu_lib):
    """8 MiB at NewConfig(4096) in a device buffer: KnownChunks.upload_new against classify + Engine.blob_encode of the new
    chunks, then every blob verifies"""
    from pbs_plus_amd import chunk_ranges

    eng = _engine(4096)
    n = 8 << 20
    buf = eng.alloc(n)
    eng.fill(buf.ptr, n, seed=71, kind=3)
    host = buf.download()
    recs = eng.chunk_and_digest(buf, nbytes=n)
    assert recs.size >= 1500
    tw = _Twins(eng, recs[::2])
    for insert in (False, True, True):
        flags2, st2 = tw.twin.classify(recs, insert=insert)
        dst, flags, offs, crcs, st = tw.fused.upload_new(buf, recs, chunk_ranges(recs), insert=insert, nbytes=n)
        new = flags2 == 0
        assert np.array_equal(flags, flags2) and st == st2 and len(tw.fused) == len(tw.twin)
        if not new.any():
            assert dst.used == 0 and not offs.any() and not crcs.any()
            dst.free()
            continue
        dst2, offs2, crcs2 = eng.blob_encode(buf, chunk_ranges(recs, known=flags2), nbytes=n)
        assert dst.used == int(offs2[-1])
        assert np.array_equal(offs[new], offs2[:-1]) and np.array_equal(crcs[new], crcs2)
        assert not offs[~new].any() and not crcs[~new].any()
        assert dst.download(0, dst.used).tobytes() == dst2.download(0, dst.used).tobytes()
        blobs = np.stack([offs[new], recs["size"][new].astype(np.uint64) + 12], axis=1)
        status, vst = eng.blob_verify(dst, blobs, digests=recs["digest"][new], sizes=recs["size"][new], nbytes=dst.used)
        assert np.all(status == 0) and vst["ok"] == int(new.sum())
        for i in np.nonzero(new)[0][:64]:
            e, m = int(recs["end"][i]), int(recs["size"][i])
            assert int(crcs[i]) == zlib.crc32(host[e - m:e].tobytes())
        dst.free()
        dst2.free()
    assert int((flags2 == 0).sum()) == 0                                 # the third pass: everything was inserted by the second
    tw.close()
    buf.free()
    eng.close()


def test_contiguous_form_edge_lengths_at_every_source_alignment(gpu_lib):
    """The piece walk of the two-part kernels on chosen part lengths: chunks of the lengths around its edge rows (under one
    16-byte unit, the row and piece edges, n = 1..3 mod 1024 above a row) at every source residue mod 16, every record
    new. Blobs and CRCs against Engine.blob_encode of the same ranges and against zlib."""
    from pbs_plus_amd import RECORD_DTYPE, KnownChunks

    lens = S.BLOB_EDGE_LENS
    chunks = np.array([(off, n) for off in range(16) for n in lens], dtype=np.uint64)
    eng = _engine(4096)
    host = np.random.default_rng(91).integers(0, 256, 2 * PIECE + 32, dtype=np.uint8)
    buf = eng.alloc(host.size)
    buf.upload(host)
    recs = np.zeros(chunks.shape[0], dtype=RECORD_DTYPE)
    recs["size"] = chunks[:, 1]
    recs["end"] = np.cumsum(chunks[:, 1])
    for i in range(recs.size):  # made-up digests, all distinct: every record is new
        recs["digest"][i] = np.frombuffer(hashlib.sha256(b"edge %d" % i).digest(), np.uint8)
    k = KnownChunks(eng)
    dst, flags, offs, crcs, st = k.upload_new(buf, recs, chunks, insert=True, nbytes=host.size)
    assert not flags.any() and st["nunique"] == recs.size == len(k)
    dst2, offs2, crcs2 = eng.blob_encode(buf, chunks, nbytes=host.size)
    assert dst.used == int(offs2[-1]) == int(chunks[:, 1].sum()) + 12 * recs.size
    assert np.array_equal(offs, offs2[:-1]) and np.array_equal(crcs, crcs2)
    # every length meets every destination residue mod 4
    assert {(int(n), (int(o) + 12) % 4) for o, n in zip(offs, chunks[:, 1])} == {(n, r) for n in lens for r in range(4)}
    out = dst.download(0, dst.used)
    assert out.tobytes() == dst2.download(0, dst.used).tobytes()
    for i, (o, n) in enumerate(chunks):
        data = host[int(o):int(o + n)].tobytes()
        crc = zlib.crc32(data)
        assert int(crcs[i]) == crc, (i, int(o), int(n))
        assert out[int(offs[i]):int(offs[i]) + 12 + int(n)].tobytes() == MAGIC + crc.to_bytes(4, "little") + data, (i, int(o), int(n))
    dst.free()
    dst2.free()
    k.close()
    buf.free()
    eng.close()
