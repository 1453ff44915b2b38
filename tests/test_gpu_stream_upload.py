"""A payload stream that holds its pages until released and frames its new chunks out of them (pbsgpu_stream_hold /
_upload_new2_device / _release / _held / _copy_device).

The reference for every output is the code that existed before: records come from a stream that does not hold, fed by the
same calls; blobs come from KnownChunks.upload_new2 (pbsgpu_known_upload_new2_device) over the same bytes in one device
buffer, with a second set preloaded alike. Everything is compared for equality.

Shape: avg 4 KiB chunker (chunks of at most a page), 64 KiB pages, the small stream ring of test_gpu_ring_partition.py
(0.02 GiB = 326 pages), 1.5 MiB of text, random bytes and repeated stretches: known, compressed and uncompressed kinds all
occur and several chunks lie in two pages."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_enc_inputs as Z  # noqa: E402

pytestmark = pytest.mark.gpu

AVG = 4096
PAGE = 65536
KiB, MiB = 1 << 10, 1 << 20
STEP = 50_000


@pytest.fixture(autouse=True)
def _short_idle_timeout(monkeypatch):
    # a service wave that sees no work gives up after this long: a bug must fail a test, not hang the box
    monkeypatch.setenv("PBSGPU_RING_IDLE_TIMEOUT_S", "5")


def _engine():
    from pbs_plus_amd import Engine, buzhash

    return Engine(buzhash.NewConfig(AVG), device=0, inflight=1, stream_sha_cus=4, stream_express_cus=2, stream_page_bytes=PAGE,
                  stream_ring_gib=0.02)


_CONTENT = {}


def _content():
    """1.5 MiB: text, random bytes, and stretches of both that come again (chunks the set then knows)"""
    if "c" not in _CONTENT:
        u8 = lambda b: np.frombuffer(b, dtype=np.uint8) if isinstance(b, (bytes, bytearray)) else b  # noqa: E731
        text, rand = u8(Z.content_of("text-1000000")), u8(Z.content_of("rand-1000000"))
        parts = [text[:400_000], rand[:300_000], text[100_000:300_000], rand[300_000:500_000], rand[50_000:200_000],
                 text[400_000:650_000]]
        c = np.concatenate(parts)
        _CONTENT["c"] = np.concatenate([c, text[: 3 * MiB // 2 - c.size]]).copy()
        assert _CONTENT["c"].size == 3 * MiB // 2
    return _CONTENT["c"]


def _busy(fn, *a):
    """fn(*a), or None when it answered PBSGPU_E_BUSY"""
    from pbs_plus_amd import _lib

    try:
        fn(*a)
        return True
    except _lib.PbsGpuError as e:
        if e.status != _lib.E_BUSY:
            raise
        return None


def _feed(ps, data, cut_at=None, inject=0, finish=True):
    """the same calls for a holder and a non-holder: STEP bytes per write, a poll behind each, one cut; -> records"""
    got, off = [], 0
    while off < data.size:
        n = min(STEP, data.size - off)
        if cut_at is not None and off < cut_at:
            n = min(n, cut_at - off)
        ps.write(data[off:off + n])
        off += n
        if off == cut_at:
            ps.inject(inject)
        got.append(ps.poll())
    if finish:
        ps.finish()
        got.append(ps.poll())
    return np.concatenate(got)


def _push_and_poll(ps, upto):
    """Small writes gather in the stream's staging buffer: push them into pages (a reservation does that) with the input
    left open, then poll until the records reach `upto`."""
    ps.reserve()
    ps.commit(0)
    got, t0 = [ps.poll()], time.time()
    while not got[-1].size or int(got[-1]["end"][-1]) < upto:
        assert time.time() - t0 < 30
        got.append(ps.poll())
    return np.concatenate(got)


def _same_records(got, want, what):
    assert got.size == want.size, (what, got.size, want.size)
    for f in ("end", "size", "segment", "digest"):
        assert np.array_equal(got[f], want[f]), (what, f)


def _reference_records(eng, data, **kw):
    from pbs_plus_amd import PayloadStream

    ps = PayloadStream(eng)
    recs = _feed(ps, data, **kw)
    ps.close()
    return recs


def _preload(eng, recs):
    """a set that already has every fifth chunk (two alike: one for the stream's call, one for the reference's)"""
    from pbs_plus_amd import KnownChunks

    k = KnownChunks(eng)
    k.add(recs[::5])
    return k


def _blobs(buf, flags, offs, lens):
    """the first lens[i] bytes of the slot of every new record"""
    host = buf.download(0, max(buf.used, 1))
    return [host[int(o):int(o) + int(ln)].tobytes() for f, o, ln in zip(flags, offs, lens) if not f]


def _reference_upload(eng, data, recs, zstd, inject_at=None, inject=0):
    """pbsgpu_known_upload_new2_device over the written bytes in one device buffer"""
    known = _preload(eng, recs)
    src = eng.alloc(data.size)
    src.upload(data)
    start = recs["end"].astype(np.int64) - recs["size"].astype(np.int64)
    if inject_at is not None:
        start = np.where(start >= inject_at + inject, start - inject, start)  # payload position -> written byte
    chunks = np.stack([start, recs["size"].astype(np.int64)], axis=1).astype(np.uint64)
    out = known.upload_new2(src, recs, chunks, insert=True, zstd=zstd, nbytes=data.size)
    res = (out[1:], _blobs(out[0], out[1], out[2], out[3]), out[0].used, len(known))
    out[0].free()
    src.free()
    known.close()
    return res


def _compare_upload(got, got_known_len, want):
    (wflags, woffs, wlens, wkinds, wcrcs, wstats, wenc), wblobs, wused, wlen = want
    buf, flags, offs, lens, kinds, crcs, stats, enc = got
    assert np.array_equal(flags, wflags)
    assert np.array_equal(offs, woffs) and np.array_equal(lens, wlens) and np.array_equal(kinds, wkinds)
    assert np.array_equal(crcs, wcrcs)
    assert buf.used == wused and stats == wstats and enc == wenc and got_known_len == wlen
    blobs = _blobs(buf, flags, offs, lens)
    assert len(blobs) == len(wblobs) and all(a == b for a, b in zip(blobs, wblobs))


def _two_pages(recs, base=0):
    start = recs["end"].astype(np.int64) - recs["size"].astype(np.int64) - base
    return int(np.count_nonzero(start // PAGE != (recs["end"].astype(np.int64) - base - 1) // PAGE))


@pytest.mark.parametrize("zstd", [False, True])
def test_one_section_equals_the_contiguous_call(gpu_lib, zstd):
    from pbs_plus_amd import PayloadStream

    data = _content()
    eng = _engine()
    want_recs = _reference_records(eng, data)
    ps = PayloadStream(eng, hold=True)
    first0, held0, free0 = ps.held()
    assert (first0, held0) == (0, 0) and free0 > 0
    recs = _feed(ps, data)
    _same_records(recs, want_recs, "holder")
    assert _two_pages(recs) >= 3
    want = _reference_upload(eng, data, recs, zstd)
    known = _preload(eng, recs)
    got = ps.upload_new2(known, recs, insert=True, zstd=zstd)
    flags, kinds = got[1], got[4]
    assert flags.any() and not flags.all()                      # known and new
    if zstd:
        assert (kinds[flags == 0] == 1).any() and (kinds[flags == 0] == 0).any()  # compressed and uncompressed
        assert _two_pages(recs[(flags == 0) & (kinds == 1)]) >= 1   # a compressed chunk in two pages
    _compare_upload(got, len(known), want)
    got[0].free()
    first, held, _ = ps.held()
    assert first == 0 and held == (data.size + PAGE - 1) // PAGE
    ps.release(int(recs["end"][-1]))
    assert ps.held() == (data.size, 0, free0)
    known.close()
    ps.close()
    eng.close()


def test_a_cut_with_injected_bytes_and_one_call_over_both_sections(gpu_lib):
    from pbs_plus_amd import PayloadStream, _lib

    data = _content()
    cut_at, inject = 700_001, 123_457
    eng = _engine()
    want_recs = _reference_records(eng, data, cut_at=cut_at, inject=inject)
    ps = PayloadStream(eng, hold=True)
    recs = _feed(ps, data, cut_at=cut_at, inject=inject)
    _same_records(recs, want_recs, "holder with a cut")
    assert set(recs["segment"].tolist()) == {0, 1}
    base1 = cut_at + inject
    assert int(recs["end"][-1]) == data.size + inject
    assert _two_pages(recs[recs["segment"] == 1], base1) >= 2       # page seams of section 1 lie at base1 + k * PAGE
    want = _reference_upload(eng, data, recs, True, inject_at=cut_at, inject=inject)
    known = _preload(eng, recs)
    got = ps.upload_new2(known, recs, insert=True, zstd=True)
    _compare_upload(got, len(known), want)
    got[0].free()
    # the raw bytes: across a page seam of either section, up to a section's last byte
    for pos, ln, w in ((PAGE - 100, 200, PAGE - 100), (base1 + 2 * PAGE - 7, 4099, cut_at + 2 * PAGE - 7),
                       (cut_at - 50, 50, cut_at - 50), (base1, 1, cut_at)):
        buf = ps.copy(pos, ln)
        assert np.array_equal(buf.download(0, ln), data[w:w + ln]), pos
        buf.free()
    # an injected gap has no bytes: inside it, into it, out of it
    dst = eng.alloc(4096)
    L = eng._L
    for pos, ln in ((cut_at + 10, 16), (cut_at - 8, 16), (base1 - 8, 16), (cut_at, 1)):
        assert L.pbsgpu_stream_copy_device(ps._h, pos, ln, dst.ptr) == _lib.E_STATE, pos
    # an unknown section, a size that reaches in front of its section: PBSGPU_E_INVALID
    for field, val in (("segment", 7), ("size", None)):
        bad = recs[recs["segment"] == 1][:2].copy()
        bad[field][0] = val if val is not None else int(bad["end"][0]) - base1 + 1
        with pytest.raises(_lib.PbsGpuError) as e:
            ps.upload_new2(known, bad, insert=False)
        assert e.value.status == _lib.E_INVALID, field
    # a position in the gap counts as the end of the section in front of it: section 0 goes as a whole
    first, held, free = ps.held()
    n0 = (cut_at + PAGE - 1) // PAGE
    ps.release(cut_at + 5)
    assert ps.held() == (base1, held - n0, free + n0)
    dst.free()
    known.close()
    ps.close()
    eng.close()


def test_release_moves_the_watermark_and_gives_the_pages_back(gpu_lib):
    from pbs_plus_amd import PayloadStream, _lib

    data = _content()
    eng = _engine()
    ps = PayloadStream(eng, hold=True)
    _, _, free0 = ps.held()
    assert _feed(ps, data[: 1 * MiB], finish=False).size == 0
    recs = _push_and_poll(ps, 900_000)                  # the input stays open: the last chunks are not cut yet
    assert recs.size > 100
    polled = int(recs["end"][-1])
    npages = (1 * MiB) // PAGE
    first, held, free = ps.held()
    assert first == 0 and held <= npages and held + free <= free0
    L = eng._L
    # beyond the last polled end: PBSGPU_E_INVALID, nothing moves
    assert L.pbsgpu_stream_release(ps._h, polled + 1) == _lib.E_INVALID
    assert ps.held() == (first, held, free)
    i = int(np.searchsorted(recs["end"], 5 * PAGE + 1000))
    mid = int(recs["end"][i])
    ps.release(mid)
    first1, held1, free1 = ps.held()
    assert first1 == mid // PAGE * PAGE and free1 - free == mid // PAGE and held - held1 <= mid // PAGE
    ps.release(mid - 3 * PAGE)                          # a lower value is a no-op
    ps.release(0)
    assert ps.held() == (first1, held1, free1)
    # a record that begins below first_position: PBSGPU_E_STATE, dst and the set unchanged
    below = recs[: i + 3]
    assert int(below["end"][0]) - int(below["size"][0]) < first1 <= int(below["end"][-1]) - int(below["size"][-1])
    known = _preload(eng, recs)
    nknown = len(known)
    dst = eng.alloc(1 * MiB)
    dst.upload(np.full(1 * MiB, 0xA5, dtype=np.uint8))
    with pytest.raises(_lib.PbsGpuError) as e:
        ps.upload_new2(known, below, insert=True, dst=dst)
    assert e.value.status == _lib.E_STATE
    assert len(known) == nknown and np.all(dst.download() == 0xA5)
    # ... a record that was not polled yet: the same
    ahead = recs[-1:].copy()
    ahead["end"] += 1
    with pytest.raises(_lib.PbsGpuError) as e:
        ps.upload_new2(known, ahead, insert=True, dst=dst)
    assert e.value.status == _lib.E_STATE
    # what is still there still uploads, and equals the contiguous call
    rest = recs[i + 3:]
    got = ps.upload_new2(known, rest, insert=True, zstd=True, dst=dst)
    ref = _preload(eng, recs)
    src = eng.alloc(1 * MiB)
    src.upload(data[: 1 * MiB])
    start = rest["end"].astype(np.int64) - rest["size"].astype(np.int64)
    want = ref.upload_new2(src, rest, np.stack([start, rest["size"].astype(np.int64)], axis=1).astype(np.uint64), insert=True,
                           zstd=True, nbytes=1 * MiB)
    _compare_upload(got, len(known), (want[1:], _blobs(want[0], want[1], want[2], want[3]), want[0].used, len(ref)))
    want[0].free()
    src.free()
    ref.close()
    # after the last release the ring has every page again
    ps.finish()
    tail = ps.poll()
    assert tail.size and int(tail["end"][-1]) == 1 * MiB
    ps.release(1 * MiB)
    assert ps.held() == (1 * MiB, 0, free0)
    dst.free()
    known.close()
    ps.close()
    eng.close()


def test_a_full_arena_answers_busy_and_loses_no_byte(gpu_lib):
    """Hold, never release, write until PBSGPU_E_BUSY; then upload, release, write the rest and finish. The rule that
    decides (hold.h: frees_without_release) is proven on the CPU by tests/test_stream_upload_native.py: a call that waits
    here is a bug in the rule."""
    from pbs_plus_amd import PayloadStream

    rng = np.random.default_rng(11)
    data = rng.integers(0, 256, 40 * MiB, dtype=np.uint8)   # twice the arena; a staging buffer takes 32 MiB before it is pushed
    piece = 4 * MiB
    eng = _engine()
    ref = PayloadStream(eng)
    want = []
    for off in range(0, data.size, piece):
        ref.write(data[off:off + piece])
        want.append(ref.poll())
    ref.finish()
    want.append(ref.poll())
    ref.close()
    want = np.concatenate(want)

    ps = PayloadStream(eng, hold=True)
    known = _preload(eng, want)
    got, off, busy, t0 = [], 0, 0, time.time()

    def make_room():
        """what a writer does with PBSGPU_E_BUSY: take the records, frame the new chunks, release"""
        nonlocal busy
        busy += 1
        recs = ps.poll()
        while recs.size == 0:
            assert time.time() - t0 < 60
            recs = ps.poll()
        got.append(recs)
        out = ps.upload_new2(known, recs, insert=True)
        assert out[0].used > 0
        out[0].free()
        before = ps.held()
        ps.release(int(recs["end"][-1]))
        assert ps.held()[2] > before[2]

    while off < data.size:
        assert time.time() - t0 < 60
        w0 = ps.bytes_written()
        ok = _busy(ps.write, data[off:off + piece])
        taken = ps.bytes_written() - w0
        assert taken == min(piece, data.size - off) if ok else 0 <= taken <= piece   # bytes_written names the prefix
        off += taken
        assert ps.position() == off
        if not ok:
            make_room()
    while not _busy(ps.finish):
        assert time.time() - t0 < 60
        make_room()
    got.append(ps.poll())
    assert busy >= 1
    _same_records(np.concatenate(got), want, "holder through a full arena")
    known.close()
    ps.close()
    eng.close()


def test_a_stream_that_does_not_hold_beside_one_that_does(gpu_lib):
    from pbs_plus_amd import PayloadStream, _lib

    data = _content()
    eng = _engine()
    want_recs = _reference_records(eng, data)
    holder = PayloadStream(eng, hold=True)
    _, _, free0 = holder.held()
    assert _feed(holder, data[: 1 * MiB], finish=False).size == 0
    hrecs = _push_and_poll(holder, 900_000)
    assert hrecs.size and holder.held()[1] > 0
    other = PayloadStream(eng)
    recs = _feed(other, data)                       # finishes without any release
    _same_records(recs, want_recs, "beside a holder")
    L = eng._L
    first, pages, free, used = C.c_uint64(7), C.c_uint32(7), C.c_uint32(7), C.c_uint64(7)
    assert L.pbsgpu_stream_held(other._h, C.byref(first), C.byref(pages), C.byref(free)) == _lib.E_STATE
    assert L.pbsgpu_stream_release(other._h, 0) == _lib.E_STATE
    assert L.pbsgpu_stream_copy_device(other._h, 0, 16, None) == _lib.E_INVALID
    dst = eng.alloc(4096)
    assert L.pbsgpu_stream_copy_device(other._h, 0, 16, dst.ptr) == _lib.E_STATE
    assert (first.value, pages.value, free.value) == (7, 7, 7)
    known = _preload(eng, recs)
    with pytest.raises(_lib.PbsGpuError) as e:
        other.upload_new2(known, recs[:4], insert=True, dst=dst)
    assert e.value.status == _lib.E_STATE
    assert L.pbsgpu_stream_hold(other._h) == _lib.E_STATE      # only before the first byte
    other.close()
    assert holder.held()[1] > 0                     # the holder still has its pages ...
    got = holder.upload_new2(known, hrecs[:8], insert=False)
    got[0].free()
    holder.close()                                  # ... and gives everything back when it is destroyed with them
    fresh = PayloadStream(eng, hold=True)           # (the recycled context starts not holding: hold() is accepted again)
    assert fresh.held() == (0, 0, free0)
    fresh.close()
    dst.free()
    known.close()
    eng.close()


def test_busy_calls_happen_entirely_or_not_at_all(gpu_lib):
    """begin_entry (its header), cut and finish on a full arena: PBSGPU_E_BUSY leaves the payload position, the section and
    the entry state as they were; after upload and release the same call goes through, and records and file hashes equal
    those of a stream that does not hold, fed by the same calls. The entry header arrives when 8 bytes are left in the
    staging buffer, so it cannot be taken without a push."""
    from pbs_plus_amd import PayloadStream

    rng = np.random.default_rng(12)
    a, body, b, inject, c = 32 * MiB - 8, 1000, 24 * MiB, 5000, 1 * MiB
    data = rng.integers(0, 256, a + body + b + c, dtype=np.uint8)

    def run(ps, room):
        got, files, busy, t0 = [], [], [0], time.time()

        def call(fn, *args):
            """fn(*args) until it is taken; on PBSGPU_E_BUSY nothing of it has happened"""
            while True:
                pos, w = ps.position(), ps.bytes_written()
                if _busy(fn, *args):
                    return
                assert (ps.position(), ps.bytes_written()) == (pos, w)
                assert time.time() - t0 < 60
                busy[0] += 1
                room(ps, got, t0)

        def write(lo, hi):
            while lo < hi:
                w0 = ps.bytes_written()
                if not _busy(ps.write, data[lo:min(lo + 4 * MiB, hi)]):
                    busy[0] += 1
                    room(ps, got, t0)
                lo += ps.bytes_written() - w0
                assert time.time() - t0 < 60

        write(0, a)
        call(ps.begin_entry, body)
        assert ps.position() == a + 16
        write(a, a + body)
        call(ps.end_entry)
        write(a + body, a + body + b)
        call(ps.inject, inject)
        assert ps.position() == a + 16 + body + b + inject
        write(a + body + b, a + body + b + c)
        call(ps.finish)
        got.append(ps.poll())
        files += ps.poll_files()
        return np.concatenate(got), files, busy[0]

    eng = _engine()
    ref = PayloadStream(eng)
    want, want_files, nbusy = run(ref, None)
    assert nbusy == 0
    ref.close()
    known = _preload(eng, want)

    def room(ps, got, t0):
        recs = ps.poll()
        while recs.size == 0:
            assert time.time() - t0 < 60
            recs = ps.poll()
        got.append(recs)
        ps.upload_new2(known, recs, insert=True)[0].free()
        ps.release(int(recs["end"][-1]))

    ps = PayloadStream(eng, hold=True)
    got, files, nbusy = run(ps, room)
    assert nbusy >= 2
    _same_records(got, want, "entries and a cut through a full arena")
    assert files == want_files and len(files) == 1 and files[0][1] == body
    known.close()
    ps.close()
    eng.close()
