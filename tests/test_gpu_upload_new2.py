"""Classify, compress and frame in one device-side call (PageRing.upload_new2 / KnownChunks.upload_new2 with zstd=True).

The yardstick is the route the call replaces, on a twin set seeded identically: classify, ring.copy_device of each new chunk
into one flat buffer, Engine.blob_encode2(zstd=True) over that buffer. Every output is compared for equality (flags,
stats, used, offsets, lens, kinds, CRCs, encode stats, the first lens[i] bytes of every slot, len(set)). Beside it an
independent check of every blob: the kind's magic, zlib.crc32 of the payload, a compressed blob's frame against
Engine.zstd_encode of the chunk's bytes, and all blobs through blob_decode2 back to the bytes that were fed, whose
hashlib.sha256 is the record's digest.

The ring is fed through reserve / commit with the test's own bytes (the generator's do not compress): text, random bytes
and runs of one byte value from zstd_enc_inputs.content_of, so that compressed and uncompressed blobs both occur and a
frame has compressed, raw and RLE blocks."""
import ctypes as C
import hashlib
import os
import sys
import time
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_enc_inputs as Z  # noqa: E402
from test_gpu_ring_upload import SID_MASK, _drive, _engine, _feed, _guarded, _oracle, _seam_suggestions  # noqa: E402

pytestmark = pytest.mark.gpu
BLOCK = 128 << 10
SENT_LEN, SENT_KIND, SENT_OFF, SENT_CRC, SENT_FLAG = 0xABCDEF01, 0x77, 7, 9, 9


@pytest.fixture(autouse=True)
def _short_idle_timeout(monkeypatch):
    monkeypatch.setenv("PBSGPU_RING_IDLE_TIMEOUT_S", "10")


def _u8(data):
    return np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else data


def _mix(n, seed):
    """n bytes: stretches of text, random bytes and (in streams long enough) a run of one byte value of 300 000"""
    rng = np.random.default_rng(seed)
    text, rand = _u8(Z.content_of("text-1000000")), _u8(Z.content_of("rand-1000000"))
    parts, size, k = [], 0, 0
    while size < n:
        ln = int(rng.integers(20_000, 120_000))
        at = int(rng.integers(0, 1_000_000 - ln))
        if k == 3 and n >= 1 << 20:
            parts.append(np.full(300_000, 0x5A, dtype=np.uint8))
        else:
            parts.append((text if k % 2 == 0 else rand)[at:at + ln])
        size += parts[-1].size
        k += 1
    return np.concatenate(parts)[:n].copy()


def _sparse(n, salt):
    """dots with a letter every 997 bytes: the chunker finds no cut in it, the encoder finds matches (no RLE block)"""
    a = np.full(n, 0x2E, dtype=np.uint8)
    idx = np.arange(0, n, 997)
    a[idx] = (65 + (idx // 997 * 7 + salt) % 26).astype(np.uint8)
    return a


def _seam_stream(O, cfg, page):
    """(6 MiB + 11 bytes, cuts to ask for) for 256 KiB pages and chunks of up to 256 KiB. Behind some text and random bytes
    a stretch without natural cuts, where the cuts asked for and the maximum alone decide: chunks with the page seam
    inside their block 1, exactly at the block edge, inside block 0, 1, 2 and 3 bytes behind their start and before their
    end; a chunk whose block 0 is random (a raw block in a frame that still wins, with the seam inside it); a run of one
    byte value across a seam (RLE blocks). Then more text, random bytes and text over few byte values."""
    P = page
    n = 24 * P + 11
    out, pos = np.zeros(n, dtype=np.uint8), 0
    rand = _u8(Z.content_of("rand-1000000"))
    r = O.chunk_and_digest(cfg, rand, [(0, rand.size)])
    i = int(np.argmax(r["size"] >= BLOCK + 64))  # random bytes behind a natural cut in which the chunker finds no cut
    quiet = rand[int(r["end"][i]) - int(r["size"][i]):][:BLOCK]
    pieces = [Z.content_of("text-500000"), Z.content_of("rand-200000"), Z.content_of("text10-%d" % (4 * P - 220000 - 700000)),
              _sparse(13 * P - 60000 - (4 * P - 220000), 1), quiet, _sparse(202144 + 60000 - BLOCK, 2), Z.content_of("byte-320000"),
              Z.content_of("text-1000000"), Z.content_of("rand-600000"), Z.content_of("text10-500000")]
    for p in pieces:
        p = _u8(p)
        out[pos:pos + p.size] = p
        pos += p.size
    out[pos:] = _u8(Z.content_of("text-%d" % (n - pos)))
    sugg = [4 * P - 200000, 5 * P - BLOCK, 6 * P - 50000, 7 * P - 1, 7 * P + 30000, 8 * P - 2, 8 * P + 20000, 9 * P - 3,
            9 * P + 20000, 10 * P + 1, 10 * P + 100000, 11 * P + 2, 11 * P + 100000, 12 * P + 3, 13 * P - 60000]
    return out, sugg


def _held(avg, page, pages, data, sugg=()):
    """a holding ring that has taken `data` through reserve / commit and released nothing: (engine, ring, stream, records)"""
    from pbs_plus_amd import PageRing

    eng = _engine(avg)
    ring = PageRing(eng, hold=True, arena_bytes=pages * (page + 256), page_bytes=page, max_streams=2, sha_cus=8, round_pages=8)
    sid = ring.open()
    for b in sugg:
        ring.suggest(sid, int(b))
    job, a = dict(mode="host", data=data, n=int(data.size)), dict(off=0, sent_final=False)
    recs, fin, t0 = [], False, time.time()
    while not fin:
        _feed(eng, ring, sid, job, a, page)
        ring.pump()
        r, fin = ring.poll(sid)
        recs.append(r.copy())
        assert time.time() - t0 < 60, ring.debug()
    return eng, ring, sid, np.concatenate(recs)


def _parts(recs, page):
    """(bytes in the first page, bytes in the second) of every record"""
    sizes = recs["size"].astype(np.int64)
    starts = recs["end"].astype(np.int64) - sizes
    first = np.minimum(sizes, page - starts % page)
    return first, sizes - first


def _dedup(st):
    from pbs_plus_amd import _lib

    return {k: int(getattr(st, k)) for k, _ in _lib.DedupStats._fields_}


def _raw(ring, known, sid, recs, insert, zstd, ptr, cap):
    """pbsgpu_ring_upload_new2_device with its outputs pre-set to sentinels:
    (status, flags, offsets, lens, kinds, crcs, used, stats, encode stats)"""
    from pbs_plus_amd import _lib
    from pbs_plus_amd.engine import _encode_stats

    n = int(recs.size)
    flags = np.full(max(n, 1), SENT_FLAG, dtype=np.uint8)
    offs = np.full(max(n, 1), SENT_OFF, dtype=np.uint64)
    lens = np.full(max(n, 1), SENT_LEN, dtype=np.uint32)
    kinds = np.full(max(n, 1), SENT_KIND, dtype=np.uint8)
    crcs = np.full(max(n, 1), SENT_CRC, dtype=np.uint32)
    used, st, enc = C.c_uint64(123), _lib.DedupStats(), _lib.EncodeStats()
    rc = ring._L.pbsgpu_ring_upload_new2_device(ring._h, known._h, _lib.RING_ANY_STREAM if sid is None else sid,
                                                recs.ctypes.data if n else None, n, int(insert), zstd, ptr, cap, flags.ctypes.data,
                                                offs.ctypes.data, lens.ctypes.data, kinds.ctypes.data, crcs.ctypes.data,
                                                C.byref(used), C.byref(st), C.byref(enc))
    return rc, flags[:n], offs[:n], lens[:n], kinds[:n], crcs[:n], int(used.value), _dedup(st), _encode_stats(enc)


def _untouched(flags, offs, lens, kinds, crcs):
    return (np.all(flags == SENT_FLAG) and np.all(offs == SENT_OFF) and np.all(lens == SENT_LEN) and np.all(kinds == SENT_KIND)
            and np.all(crcs == SENT_CRC))


def _check_blobs(eng, dstbuf, out, offs, lens, kinds, crcs, datas, digests):
    """the independent check of the blobs of the new records (all arrays over the new records only): magic, CRC, a
    compressed blob's frame = Engine.zstd_encode of the chunk's bytes, everything back through blob_decode2"""
    from pbs_plus_amd import RECORD_DTYPE, blob_magic

    n = len(datas)
    if n == 0:
        return
    flat = np.concatenate([_u8(d) for d in datas]) if sum(len(d) for d in datas) else np.zeros(0, dtype=np.uint8)
    sizes = np.array([len(d) for d in datas], dtype=np.uint64)
    ends = np.cumsum(sizes)
    comp = np.flatnonzero(kinds == 1)
    frames = {}
    if comp.size:
        src = eng.alloc(max(int(flat.size), 16))
        src.upload(flat)
        fdst, status, flen, rooms = eng.zstd_encode(src, np.stack([ends - sizes, sizes], axis=1)[comp])
        fout = fdst.download()
        assert np.all(status == 0)
        for j, i in enumerate(comp):
            frames[int(i)] = fout[int(rooms[j, 0]):int(rooms[j, 0]) + int(flen[j])].tobytes()
        fdst.free()
        src.free()
    for i in range(n):
        o, ln, k = int(offs[i]), int(lens[i]), int(kinds[i])
        blob = out[o:o + ln].tobytes()
        payload = blob[12:]
        assert blob[:8] == blob_magic(k), i
        assert int.from_bytes(blob[8:12], "little") == zlib.crc32(payload) == int(crcs[i]), i
        if k:
            assert len(payload) < len(datas[i]) and payload == frames[i], i
        else:
            assert payload == bytes(datas[i]), i
    idx = np.zeros(n, dtype=RECORD_DTYPE)
    idx["size"], idx["end"], idx["digest"] = sizes, ends, digests
    back, status, _ = eng.blob_decode2(dstbuf, np.stack([offs.astype(np.uint64), lens.astype(np.uint64)], axis=1), idx,
                                       np.arange(n, dtype=np.uint32), 0, int(ends[-1]), True, zstd=True)
    got = back.download(0, int(ends[-1])) if int(ends[-1]) else np.zeros(0, dtype=np.uint8)
    back.free()
    assert np.all(status == 0), np.flatnonzero(status)
    assert got.tobytes() == flat.tobytes()
    for i in range(n):
        assert hashlib.sha256(bytes(datas[i])).digest() == bytes(digests[i]), i


class _Twins:
    """two sets seeded identically; check() takes one batch through the three-call route and through the fused call"""

    def __init__(self, eng, seed=None, capacity=0):
        from pbs_plus_amd import KnownChunks

        self.eng = eng
        self.fused, self.twin = KnownChunks(eng, capacity), KnownChunks(eng, capacity)
        if seed is not None and seed.size:
            self.fused.add(seed)
            self.twin.add(seed)
        self.kinds = [0, 0]          # new records per kind, over all batches
        self.nknown = self.ndup = 0
        self.firsts, self.lasts = [], []  # of the new records in two pages: bytes in the first page, in the second

    def close(self):
        self.fused.close()
        self.twin.close()

    def three_calls(self, ring, sid, recs, insert):
        """classify -> ring.copy_device of each new chunk into one flat buffer -> Engine.blob_encode2(zstd=True)"""
        flags, st = self.twin.classify(recs, insert=insert)
        new = np.flatnonzero(flags == 0)
        sizes = recs["size"][new].astype(np.uint64)
        ends = np.cumsum(sizes)
        total = int(ends[-1]) if new.size else 0
        flat = self.eng.alloc(max(total, 16))
        for j, i in enumerate(new):
            s = int(recs["segment"][i]) & SID_MASK if sid is None else sid
            assert ring._L.pbsgpu_ring_copy_device(ring._h, s, int(recs["end"][i]) - int(recs["size"][i]), int(recs["size"][i]),
                                                   flat.ptr + int(ends[j] - sizes[j])) == 0
        host = flat.download(0, total) if total else np.zeros(0, dtype=np.uint8)
        if new.size == 0:
            flat.free()
            return flags, st, host, None
        dst, offs, lens, kinds, crcs, est = self.eng.blob_encode2(flat, np.stack([ends - sizes, sizes], axis=1), nbytes=total,
                                                                 zstd=True)
        out = dst.download(0, int(offs[-1]))
        dst.free()
        flat.free()
        return flags, st, host, (out, offs, lens, kinds, crcs, est)

    def check(self, ring, sid, recs, bytes_of, insert=True):
        recs = np.ascontiguousarray(recs)
        flags2, st2, flat, enc2 = self.three_calls(ring, sid, recs, insert)
        dst, flags, offs, lens, kinds, crcs, st, est = ring.upload_new2(self.fused, sid, recs, insert=insert, zstd=True)
        out = dst.download(0, dst.used) if dst.used else np.zeros(0, dtype=np.uint8)
        new = np.flatnonzero(flags2 == 0)
        try:
            assert np.array_equal(flags, flags2) and st == st2, (st, st2)
            assert len(self.fused) == len(self.twin)
            known = flags2 != 0
            assert not offs[known].any() and not lens[known].any() and not kinds[known].any() and not crcs[known].any()
            if enc2 is None:
                assert dst.used == 0 and est["blobs"] == [0, 0] and est["crc_bytes"] == 0
                return flags
            out2, offs2, lens2, kinds2, crcs2, est2 = enc2
            assert dst.used == int(offs2[-1])
            assert np.array_equal(offs[new], offs2[:-1]) and np.array_equal(lens[new], lens2)
            assert np.array_equal(kinds[new], kinds2) and np.array_equal(crcs[new], crcs2)
            assert est == est2, (est, est2)
            for j, i in enumerate(new):
                o, ln = int(offs[i]), int(lens[i])
                assert out[o:o + ln].tobytes() == out2[o:o + ln].tobytes(), (j, i)
            datas = [bytes_of(int(i)) for i in new]
            assert b"".join(datas) == flat.tobytes()  # what ring.copy_device took out of the pages is what was fed
            _check_blobs(self.eng, dst, out, offs[new], lens[new], kinds[new], crcs[new], datas, recs["digest"][new])
        finally:
            dst.free()
        first, second = _parts(recs, ring.page_bytes)
        for i in new:
            self.kinds[int(kinds[i])] += 1
            if second[i]:
                self.firsts.append(int(first[i]))
                self.lasts.append(int(second[i]))
        self.nknown += int((flags2 != 0).sum())
        digs = [d.tobytes() for d in recs["digest"]]
        self.ndup += len(digs) - len(set(digs))
        return flags


def _single(host, recs):
    ends, sizes = recs["end"].astype(np.int64), recs["size"].astype(np.int64)
    return lambda i: host[ends[i] - sizes[i]:ends[i]].tobytes()


def test_two_blocks_and_a_seam(gpu_lib, O):
    """Chunks of up to 256 KiB in 256 KiB pages, about one in four in two pages, every other one-page chunk known: the
    seam inside block 0 and inside block 1 of a chunk, exactly at the 128 KiB block edge, and 1, 2 and 3 bytes behind a
    chunk's start and before its end, all among the NEW records. A second call on the same records finds everything
    known, writes nothing and leaves lens and kinds alone."""
    page = 262144
    host, sugg = _seam_stream(O, O.new_config(65536), page)
    eng, ring, sid, recs = _held(65536, page, 64, host, sugg)
    assert set(sugg) <= set(int(e) for e in recs["end"])
    first, second = _parts(recs, page)
    one_page = np.flatnonzero(second == 0)
    tw = _Twins(eng, recs[one_page[::2]])
    tw.check(ring, sid, recs, _single(host, recs), insert=True)
    print("kinds", tw.kinds, "known", tw.nknown, "first parts", sorted(tw.firsts), "last parts", sorted(tw.lasts))
    assert tw.kinds[0] >= 3 and tw.kinds[1] >= 30 and tw.nknown >= 16, (tw.kinds, tw.nknown)
    sizes = {a: a + b for a, b in zip(tw.firsts, tw.lasts)}
    assert len(tw.firsts) >= 20
    assert [a for a in tw.firsts if a < BLOCK and sizes[a] > BLOCK]                      # inside block 0 of two
    assert [a for a in tw.firsts if BLOCK < a < sizes[a]]                                # inside block 1
    assert BLOCK in tw.firsts and sizes[BLOCK] > BLOCK                                   # exactly at the block edge
    assert {1, 2, 3} <= set(tw.firsts) and {1, 2, 3} <= set(tw.lasts)
    g = _guarded(eng, 4096)
    rc, flags, offs, lens, kinds, crcs, used, st, est = _raw(ring, tw.fused, sid, recs, 1, 1, g.ptr + 64, 4096)
    assert rc == 0 and used == 0 and np.all(flags == 1)
    assert _untouched(np.full(1, SENT_FLAG), offs, lens, kinds, crcs)
    assert st["nunique"] == 0 and st["nrecords"] == recs.size and est["blobs"] == [0, 0]
    assert np.all(g.download() == 0xA5)
    assert len(tw.fused) == len(tw.twin)
    g.free()
    tw.close()
    ring.close_stream(sid)
    ring.close()
    eng.close()


def test_small_chunks_duplicates_and_a_chunk_under_four_bytes(gpu_lib):
    """NewConfig(4096), 64 KiB pages, 2 MiB of the mix with cuts asked for 1-3 bytes around the seams, then the same
    records with some repeated inside the batch; a second stream of 3 bytes gives a chunk under 4 bytes."""
    page = 65536
    n = 2 << 20
    host = _mix(n, 7)
    eng, ring, sid, recs = _held(4096, page, 64, host, _seam_suggestions(n, page, 1024))
    tw = _Twins(eng, recs[::2])
    both = np.concatenate([recs, recs[1::5]])                            # duplicates inside the batch
    tw.check(ring, sid, both, _single(host, both), insert=True)
    print("kinds", tw.kinds, "known", tw.nknown, "dup", tw.ndup)
    assert tw.kinds[0] >= 20 and tw.kinds[1] >= 20 and tw.ndup >= recs[1::5].size and tw.nknown > recs.size // 2
    assert len(tw.firsts) >= 8
    tiny = np.array([1, 2, 3], dtype=np.uint8)
    sid2 = ring.open()
    job, a = dict(mode="host", data=tiny, n=3), dict(off=0, sent_final=False)
    got, fin, t0 = [], False, time.time()
    while not fin:
        _feed(eng, ring, sid2, job, a, page)
        ring.pump()
        r, fin = ring.poll(sid2)
        got.append(r.copy())
        assert time.time() - t0 < 60, ring.debug()
    got = np.concatenate(got)
    assert got.size == 1 and int(got["size"][0]) == 3
    before = list(tw.kinds)
    tw.check(ring, sid2, got, _single(tiny, got), insert=True)
    assert tw.kinds == [before[0] + 1, before[1]]
    tw.close()
    ring.close_stream(sid)
    ring.close_stream(sid2)
    ring.close()
    eng.close()


def test_any_stream(gpu_lib, O):
    """two streams of different content in 64 KiB pages, polled with poll_any: every record's stream is its segment"""
    from pbs_plus_amd import PageRing

    page = 65536
    eng = _engine(4096)
    hosts = [_mix((1 << 20) + 5, 11), _mix((768 << 10) + 77, 12)]
    jobs = [dict(mode="host", data=h, n=int(h.size)) for h in hosts]
    want = [_oracle(O, O.new_config(4096), h, None) for h in hosts]
    tw = _Twins(eng, np.concatenate([w[1::2] for w in want]))
    ring = PageRing(eng, hold=True, arena_bytes=64 * (page + 256), page_bytes=page, max_streams=4, sha_cus=8, round_pages=8)
    mixed = []

    def on_records(sid, js, recs):
        mixed.append(np.unique(js).size)
        ends, sizes = recs["end"].astype(np.int64), recs["size"].astype(np.int64)
        tw.check(ring, sid, recs, lambda i: hosts[int(js[i])][ends[i] - sizes[i]:ends[i]].tobytes())
        sids = recs["segment"] & SID_MASK
        for s in np.unique(sids):
            ring.release(int(s), int(ends[sids == s].max()))

    got = _drive(eng, ring, jobs, on_records, any_stream=True)
    ring.quiesce()
    for g, w in zip(got, want):
        assert np.array_equal(g["end"], w["end"]) and np.array_equal(g["digest"], w["digest"])
    print("kinds", tw.kinds, "known", tw.nknown, "batches", mixed)
    assert max(mixed) >= 2 and tw.kinds[0] > 0 and tw.kinds[1] > 0 and tw.nknown > 0
    tw.close()
    ring.close()
    eng.close()


@pytest.fixture(scope="module")
def held_mix(gpu_lib):
    """a holding ring with 1.5 MiB of the mix at NewConfig(65536) in 256 KiB pages, nothing released"""
    host = _mix((3 << 19) + 11, 21)
    eng, ring, sid, recs = _held(65536, 262144, 32, host)
    yield eng, ring, sid, recs, host
    ring.close_stream(sid)
    ring.close()
    eng.close()


def test_capacity_leaves_destination_and_set_untouched(held_mix):
    from pbs_plus_amd import _lib

    eng, ring, sid, recs, host = held_mix
    tw = _Twins(eng, recs[::2])
    want_flags, want_st = tw.twin.classify(recs, insert=False)
    new = want_flags == 0
    needed = int(recs["size"][new].astype(np.uint64).sum()) + 12 * int(new.sum())
    before = len(tw.fused)
    rc, flags, offs, lens, kinds, crcs, used, st, est = _raw(ring, tw.fused, sid, recs, 1, 1, None, 0)  # the sizing call
    assert rc == _lib.E_CAPACITY and used == needed and np.array_equal(flags, want_flags) and st == want_st
    g = _guarded(eng, needed)
    rc, flags, offs, lens, kinds, crcs, used, st, est = _raw(ring, tw.fused, sid, recs, 1, 1, g.ptr + 64, needed - 1)
    assert rc == _lib.E_CAPACITY and used == needed
    assert np.all(g.download() == 0xA5)
    assert len(tw.fused) == before
    assert np.array_equal(flags, want_flags) and st == want_st          # still valid: the caller can retry
    assert _untouched(np.full(1, SENT_FLAG), offs, lens, kinds, crcs) and est["blobs"] == [0, 0]
    again, _ = tw.fused.classify(recs, insert=False)
    assert np.array_equal(again, want_flags)
    rc, flags, offs, lens, kinds, crcs, used, st, est = _raw(ring, tw.fused, sid, recs, 1, 1, g.ptr + 64, needed)
    assert rc == 0 and used == needed and np.array_equal(flags, want_flags) and st == want_st
    out = g.download()
    assert np.all(out[:64] == 0xA5) and np.all(out[64 + needed:] == 0xA5)
    flags2, st2, flat, (out2, offs2, lens2, kinds2, crcs2, est2) = tw.three_calls(ring, sid, recs, True)
    assert np.array_equal(offs[new], offs2[:-1]) and np.array_equal(lens[new], lens2) and np.array_equal(kinds[new], kinds2)
    assert np.array_equal(crcs[new], crcs2) and est == est2 and 0 < est["blobs"][0] and 0 < est["blobs"][1]
    for i in np.flatnonzero(new):
        o, ln = int(offs[i]), int(lens[i])
        assert out[64 + o:64 + o + ln].tobytes() == out2[o:o + ln].tobytes(), i
    assert _untouched(np.full(1, SENT_FLAG), offs[~new], lens[~new], kinds[~new], crcs[~new])
    assert len(tw.fused) == len(tw.twin) == before + int(new.sum())
    g.free()
    tw.close()


def test_without_the_flag_it_is_upload_new(held_mix):
    """flags = 0 equals pbsgpu_ring_upload_new_device output for output, with lens = 12 + size and kinds = 0"""
    eng, ring, sid, recs, host = held_mix
    tw = _Twins(eng, recs[1::2])
    for insert in (False, True, True):
        dst2, flags2, offs2, crcs2, st2 = ring.upload_new(tw.twin, sid, recs, insert=insert)
        dst, flags, offs, lens, kinds, crcs, st, est = ring.upload_new2(tw.fused, sid, recs, insert=insert, zstd=False)
        new = flags2 == 0
        assert np.array_equal(flags, flags2) and st == st2 and dst.used == dst2.used and len(tw.fused) == len(tw.twin)
        assert np.array_equal(offs, offs2) and np.array_equal(crcs, crcs2)
        assert np.array_equal(lens[new], recs["size"][new] + 12) and not lens[~new].any() and not kinds.any()
        if dst.used:
            assert dst.download(0, dst.used).tobytes() == dst2.download(0, dst.used).tobytes()
        nnew, nbytes = int(new.sum()), int(recs["size"][new].astype(np.uint64).sum())
        assert est == dict(blobs=[nnew, 0], blob_bytes=[nbytes + 12 * nnew, 0], chunk_bytes=[nbytes, 0], frame_bytes=0,
                           crc_bytes=nbytes)
        dst.free()
        dst2.free()
    assert not new.any()                                                 # the third pass: everything was inserted by the second
    tw.close()


def test_the_set_grows_inside_the_call(held_mix):
    """a set created for one digest takes the whole batch: the call's second synchronisation"""
    eng, ring, sid, recs, host = held_mix
    tw = _Twins(eng, capacity=1)
    tw.check(ring, sid, recs, _single(host, recs))
    assert len(tw.fused) == np.unique(recs["digest"], axis=0).shape[0] == sum(tw.kinds) and min(tw.kinds) > 0
    again, _ = tw.fused.classify(recs, insert=False)
    assert np.all(again == 1)
    tw.close()


def test_refusals_are_decided_before_any_device_work(held_mix):
    """an unknown flag bit, a record not yet polled, a chunk larger than a page, a host destination, a set of another
    engine, a ring without the flag, a record below held()'s first offset; in the contiguous form a destination inside the
    source: sentinels in every output, dst and the set untouched every time. (The last test on the shared ring: it
    releases pages.)"""
    from pbs_plus_amd import RECORD_DTYPE, KnownChunks, PageRing, _lib

    eng, ring, sid, recs, host = held_mix
    tw = _Twins(eng, recs[::2])
    before = len(tw.fused)
    late = recs[-1:].copy()
    late["end"] += 1
    huge = recs[-1:].copy()
    huge["size"] = ring.page_bytes + 1
    g = _guarded(eng, 1 << 20)
    cases = [(recs[:3], 2, _lib.E_INVALID), (recs[:3], 3, _lib.E_INVALID), (recs[:3], 1 << 31, _lib.E_INVALID),
             (np.concatenate([recs[:2], late]), 1, _lib.E_STATE), (huge, 1, _lib.E_INVALID)]
    for batch, zflags, want in cases:
        rc, flags, offs, lens, kinds, crcs, used, st, est = _raw(ring, tw.fused, sid, np.ascontiguousarray(batch), 1, zflags,
                                                                 g.ptr + 64, 1 << 20)
        assert rc == want, (rc, want)
        assert _untouched(flags, offs, lens, kinds, crcs) and used == 123 and len(tw.fused) == before
    assert np.all(g.download() == 0xA5)
    hostbuf = np.zeros(1 << 20, dtype=np.uint8)
    rc, flags, offs, lens, kinds, crcs, used, st, est = _raw(ring, tw.fused, sid, recs[:3], 1, 1, hostbuf.ctypes.data, hostbuf.size)
    assert rc == _lib.E_INVALID and not hostbuf.any() and len(tw.fused) == before and _untouched(flags, offs, lens, kinds, crcs)
    eng2 = _engine(65536)
    other = KnownChunks(eng2)
    assert _raw(ring, other, sid, recs[:3], 1, 1, g.ptr + 64, 1 << 20)[0] == _lib.E_INVALID
    other.close()
    eng2.close()
    eng3 = _engine(65536)
    plain = PageRing(eng3, arena_bytes=64 * (262144 + 256), page_bytes=262144, max_streams=2, sha_cus=8, round_pages=8)  # no HOLD_PAGES
    mine = KnownChunks(eng3)
    assert _raw(plain, mine, plain.open(), recs[:3], 1, 1, g.ptr + 64, 1 << 20)[0] == _lib.E_STATE
    mine.close()
    plain.close()
    eng3.close()
    # the contiguous form: dst inside src, at its first byte, its last byte, and one byte in front of it with room to reach it
    src = eng.alloc(4096)
    chunks = np.array([[0, 100], [100, 50]], dtype=np.uint64)
    two = np.zeros(2, dtype=RECORD_DTYPE)
    two["size"], two["end"] = (100, 50), (100, 150)
    for i in range(2):
        two["digest"][i] = np.frombuffer(hashlib.sha256(b"refusal %d" % i).digest(), np.uint8)
    for ptr, cap, zflags, want in ((src.ptr, 4096, 1, _lib.E_INVALID), (src.ptr + 4095, 4096, 1, _lib.E_INVALID),
                                   (src.ptr - 1, 174, 1, _lib.E_INVALID), (g.ptr + 64, 1 << 20, 4, _lib.E_INVALID)):
        flags = np.full(2, SENT_FLAG, dtype=np.uint8)
        offs = np.full(2, SENT_OFF, dtype=np.uint64)
        lens = np.full(2, SENT_LEN, dtype=np.uint32)
        kinds = np.full(2, SENT_KIND, dtype=np.uint8)
        crcs = np.full(2, SENT_CRC, dtype=np.uint32)
        used, st, enc = C.c_uint64(123), _lib.DedupStats(), _lib.EncodeStats()
        rc = eng._L.pbsgpu_known_upload_new2_device(tw.fused._h, src.ptr, 4096, two.ctypes.data, chunks.ctypes.data, 2, 1, zflags,
                                                    ptr, cap, flags.ctypes.data, offs.ctypes.data, lens.ctypes.data,
                                                    kinds.ctypes.data, crcs.ctypes.data, C.byref(used), C.byref(st), C.byref(enc))
        assert rc == want and _untouched(flags, offs, lens, kinds, crcs) and used.value == 123 and len(tw.fused) == before
    assert np.all(g.download() == 0xA5)
    src.free()
    ring.release(sid, int(recs["end"][recs.size // 2]))
    first, _ = ring.held(sid)
    starts = recs["end"] - recs["size"]
    gone, kept = recs[starts < first], recs[starts >= first]
    assert gone.size and kept.size
    for batch in (np.concatenate([kept[:3], gone[-1:]]), gone[:1]):
        rc, flags, offs, lens, kinds, crcs, used, st, est = _raw(ring, tw.fused, sid, np.ascontiguousarray(batch), 1, 1, g.ptr + 64,
                                                                 1 << 20)
        assert rc == _lib.E_STATE and _untouched(flags, offs, lens, kinds, crcs) and used == 123 and len(tw.fused) == before
    assert np.all(g.download() == 0xA5)
    tw.check(ring, sid, kept, _single(host, kept))                       # what is still held works as ever
    g.free()
    tw.close()


def test_contiguous_form_edge_lengths_at_four_source_alignments(gpu_lib):
    """Text chunks of the lengths around the frame header's and the block's edges at source alignments 0, 1, 3 and 8, half
    of the digests known: KnownChunks.upload_new2 against classify + Engine.blob_encode2 over the new chunks."""
    from pbs_plus_amd import RECORD_DTYPE

    lens_ = (1, 3, 4, 5, 255, 256, 65_791, 65_792, 131_071, 131_072, 131_073, 300_000)
    text = _u8(Z.content_of("text-400000"))
    parts, ranges, pos = [], [], 0
    for al in (0, 1, 3, 8):
        for k, n in enumerate(lens_):
            gap = (-pos) % 16 + al
            parts.append(np.zeros(gap, dtype=np.uint8))
            chunk = text[7 * (k + al):7 * (k + al) + n].copy()
            chunk[0] = 48 + len(ranges)                                  # (48 distinct digests, the one-byte chunks included)
            parts.append(chunk)
            ranges.append((pos + gap, n))
            pos += gap + n
    host = np.concatenate(parts)
    chunks = np.array(ranges, dtype=np.uint64)
    recs = np.zeros(len(ranges), dtype=RECORD_DTYPE)
    recs["size"] = chunks[:, 1]
    recs["end"] = np.cumsum(chunks[:, 1])
    datas = [host[o:o + n].tobytes() for o, n in ranges]
    for i, d in enumerate(datas):
        recs["digest"][i] = np.frombuffer(hashlib.sha256(d).digest(), np.uint8)
    assert np.unique(recs["digest"], axis=0).shape[0] == recs.size
    eng = _engine(4096)
    buf = eng.alloc(host.size)
    buf.upload(host)
    tw = _Twins(eng, recs[1::2])
    for insert in (False, True, True):
        flags2, st2 = tw.twin.classify(recs, insert=insert)
        new = flags2 == 0
        dst, flags, offs, lens, kinds, crcs, st, est = tw.fused.upload_new2(buf, recs, chunks, insert=insert, zstd=True,
                                                                            nbytes=host.size)
        assert np.array_equal(flags, flags2) and st == st2 and len(tw.fused) == len(tw.twin)
        if not new.any():
            assert dst.used == 0 and not offs.any() and not lens.any() and est["blobs"] == [0, 0]
            dst.free()
            continue
        dst2, offs2, lens2, kinds2, crcs2, est2 = eng.blob_encode2(buf, chunks[new], nbytes=host.size, zstd=True)
        assert dst.used == int(offs2[-1]) and est == est2
        assert np.array_equal(offs[new], offs2[:-1]) and np.array_equal(lens[new], lens2)
        assert np.array_equal(kinds[new], kinds2) and np.array_equal(crcs[new], crcs2)
        assert not offs[~new].any() and not lens[~new].any() and not kinds[~new].any() and not crcs[~new].any()
        out, out2 = dst.download(0, dst.used), dst2.download(0, dst.used)
        for i in np.flatnonzero(new):
            o, ln = int(offs[i]), int(lens[i])
            assert out[o:o + ln].tobytes() == out2[o:o + ln].tobytes(), i
        assert est["blobs"][0] >= 6 and est["blobs"][1] >= 12, est      # 1..5 bytes cannot win; text from 255 bytes on does
        _check_blobs(eng, dst, out, offs[new], lens[new], kinds[new], crcs[new], [datas[i] for i in np.flatnonzero(new)],
                     recs["digest"][new])
        dst.free()
        dst2.free()
    assert not new.any()
    tw.close()
    buf.free()
    eng.close()


def test_beside_the_running_services(gpu_lib, O):
    """One stream of 6 MiB of the mix in 64 KiB pages; between pumps, while the services run, polled records go through the
    fused call. Equal to the three-call route every time, and the ring's records still equal the oracle's."""
    from pbs_plus_amd import PageRing

    page = 65536
    eng = _engine(4096)
    host = _mix((6 << 20) + 5, 31)
    jobs = [dict(mode="host", data=host, n=int(host.size))]
    want = _oracle(O, O.new_config(4096), host, None)
    ring = PageRing(eng, hold=True, arena_bytes=160 * (page + 256), page_bytes=page, max_streams=2, sha_cus=16, round_pages=8)
    tw = _Twins(eng, want[::2])
    state = dict(recs=None, sid=None, runs=0)

    def on_records(sid, js, recs):
        ring.release(sid, int(recs["end"][0] - recs["size"][0]))         # what came before this poll has had its turn
        if int(recs["end"][-1]) != host.size and state["recs"] is None:
            state["recs"], state["sid"] = recs[:400].copy(), sid          # not released: still there after the next pump

    def between():
        if state["recs"] is None or ring.stats()["service_launches"] < 1:
            return
        recs, sid = state["recs"], state["sid"]
        tw.check(ring, sid, recs, _single(host, recs))
        state["runs"] += 1
        state["recs"] = None

    got = _drive(eng, ring, jobs, on_records, between=between)
    ring.quiesce()
    print("runs", state["runs"], "kinds", tw.kinds, "known", tw.nknown)
    assert state["runs"] >= 1 and tw.kinds[0] > 0 and tw.kinds[1] > 0 and tw.nknown > 0
    assert got[0].size == want.size and np.array_equal(got[0]["end"], want["end"]) and np.array_equal(got[0]["digest"], want["digest"])
    st = ring.stats()
    assert st["pages_free"] == st["pages_total"], st
    tw.close()
    ring.close()
    eng.close()
