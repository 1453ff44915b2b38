"""The zstd encoder's mode with per-block sequence tables and repeat codes on the GPU: an engine created with
zstd_seq_tables=1 beside a default engine in the same process. pbsgpu_zstd_encode_device must write the frames of
tests/golden/zstd_enc_tables_v1.json (what the CPU build of the same format core writes under sanitizers and libzstd
decodes, tests/test_zstd_encode_tables_native.py), whatever the order of the chunks; the default engine still writes
those of zstd_enc_v1.json. pbsgpu_blob_encode2_device and both fused upload calls of that engine carry the same frames, at
the slots, capacities and verdict rules they always had, and the device's own decoder, which until now met compressed
tables and repeat codes only in a handful of libzstd-made frames, gives every content back."""
import hashlib
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_upload_new2 as U  # noqa: E402
import zstd_enc_tables_inputs as ti  # noqa: E402

zi = ti.zi
pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
OK, BAD_SIZE = 0, 2


@pytest.fixture(autouse=True)
def _short_idle_timeout(monkeypatch):
    monkeypatch.setenv("PBSGPU_RING_IDLE_TIMEOUT_S", "10")


def _tables_engine(avg):
    from pbs_plus_amd import Engine, buzhash

    return Engine(buzhash.NewConfig(avg), device=0, inflight=1, zstd_seq_tables=1)


@pytest.fixture(scope="module")
def world(gpu_lib):
    """(engine with the option, default engine, cases, device buffer of all contents 0-6 bytes apart, their ranges)"""
    from pbs_plus_amd import Engine, buzhash

    eng1 = _tables_engine(4096)
    eng0 = Engine(buzhash.NewConfig(4096), device=0)
    cases = ti.cases()
    rng = np.random.default_rng(10)
    parts, ranges, pos = [], [], 0
    for _, data in cases:
        gap = int(rng.integers(0, 7))
        parts.append(bytes(gap) + data)
        ranges.append((pos + gap, len(data)))
        pos += gap + len(data)
    host = np.frombuffer(b"".join(parts), np.uint8)
    dev = eng1.alloc(host.size)
    dev.upload(host)
    yield eng1, eng0, cases, dev, np.array(ranges, dtype=np.uint64)
    dev.free()
    eng0.close()
    eng1.close()


def _encode(eng, dev, ranges, rooms):
    """one call with room i of rooms[i] bytes between guards of a pattern, which are checked here:
    (status, frame lengths, [the room's bytes], dst, out). The caller frees dst."""
    out, pos = [], GUARD
    for r in rooms:
        out.append((pos, r))
        pos += r + GUARD
    dst = eng.alloc(pos)
    dst.upload(np.full(pos, FILL, np.uint8))
    out = np.array(out, dtype=np.uint64).reshape(-1, 2)
    _, status, flen, _ = eng.zstd_encode(dev, ranges, out=out, dst=dst)
    got = dst.download(0, pos)
    at = 0
    for o, r in out:
        assert np.all(got[at:int(o)] == FILL), "guard in front of room at %d" % o
        at = int(o + r)
    assert np.all(got[at:] == FILL), "guard behind the last room"
    return status, flen, [got[int(o):int(o + r)] for o, r in out], dst, out


@pytest.fixture(scope="module")
def first(world):
    """every case in one call on the engine with the option: (status, frame lengths, frames as bytes, dst, out)"""
    eng1, _, cases, dev, ranges = world
    status, flen, rooms, dst, out = _encode(eng1, dev, ranges, [zi.bound(len(d)) for _, d in cases])
    frames = [rooms[i][:int(flen[i])].tobytes() for i in range(len(cases))]
    yield status, flen, frames, dst, out
    dst.free()


def test_every_frame_is_the_golden_one_of_the_mode(world, first):
    _, _, cases, _, _ = world
    status, flen, frames, _, _ = first
    golden = ti.golden()
    assert np.all(status == OK), [cases[i][0] for i in np.flatnonzero(status != OK)]
    for (name, data), frame in zip(cases, frames):
        assert 0 < len(frame) <= zi.bound(len(data)), name
        assert [len(frame), hashlib.sha256(frame).hexdigest()] == golden[name], name


def test_the_frames_do_not_depend_on_order_or_neighbours(world, first):
    eng1, _, cases, dev, ranges = world
    _, _, frames, _, _ = first
    n = len(cases)
    rev = np.arange(n)[::-1]
    status, flen, rooms, dst, _ = _encode(eng1, dev, ranges[rev], [zi.bound(len(cases[i][1])) for i in rev])
    dst.free()
    assert np.all(status == OK)
    for k, i in enumerate(rev):
        assert rooms[k][:int(flen[k])].tobytes() == frames[i], cases[i][0]
    for name in ("text-300000", "touch-300000", "seqs-2", "zeros-0"):
        i = [c[0] for c in cases].index(name)
        status, flen, rooms, dst, _ = _encode(eng1, dev, ranges[i:i + 1], [zi.bound(len(cases[i][1]))])
        dst.free()
        assert status[0] == OK and rooms[0][:int(flen[0])].tobytes() == frames[i], name


def test_a_default_engine_beside_it_writes_the_frames_it_always_wrote(world, first):
    _, eng0, cases, dev, ranges = world
    base = zi.cases()
    golden = zi.golden()
    n = len(base)
    assert [c[0] for c in cases[:n]] == [c[0] for c in base]
    status, flen, rooms, dst, _ = _encode(eng0, dev, ranges[:n], [zi.bound(len(d)) for _, d in base])
    dst.free()
    assert np.all(status == OK)
    shorter = 0
    for k, (name, _) in enumerate(base):
        frame = rooms[k][:int(flen[k])].tobytes()
        assert [len(frame), hashlib.sha256(frame).hexdigest()] == golden[name], name
        assert len(first[2][k]) <= len(frame), name
        shorter += len(first[2][k]) < len(frame)
    assert shorter >= 20  # two engines, two settings


def test_the_device_decoder_gives_the_contents_back(world, first):
    eng1, _, cases, _, _ = world
    status, flen, frames, dst, out = first
    fr = np.stack([out[:, 0], flen], axis=1)
    sizes = np.array([len(d) for _, d in cases], dtype=np.uint64)
    ends = np.cumsum(sizes)
    back, st, decoded, _ = eng1.zstd_decode(dst, fr, out=np.stack([ends - sizes, sizes], axis=1))
    try:
        got = back.download(0, max(int(ends[-1]), 1))
    finally:
        back.free()
    assert np.all(st == OK) and np.array_equal(decoded, sizes)
    assert got[:int(ends[-1])].tobytes() == b"".join(d for _, d in cases)


def test_blobs_carry_the_golden_frames_in_the_uncompressed_layouts_slots(world, first):
    """kinds, lens and CRCs against a host recomputation from the frames (which are the golden ones); the blobs through
    blob_decode2 with zstd back to the contents (U._check_blobs), the frames against zstd_encode on the same engine"""
    eng1, _, cases, dev, ranges = world
    _, _, frames, _, _ = first
    pick = [i for i, (_, d) in enumerate(cases) if len(d)]
    datas = [cases[i][1] for i in pick]
    dst, offs, lens, kinds, crcs, est = eng1.blob_encode2(dev, ranges[pick], zstd=True)
    try:
        out = dst.download(0, int(offs[-1]))
        sizes = np.array([len(d) for d in datas], dtype=np.uint64)
        assert np.array_equal(offs, np.concatenate([[0], np.cumsum(sizes + 12)]).astype(np.uint64))
        for k, i in enumerate(pick):
            wins = len(frames[i]) < len(datas[k])
            payload = frames[i] if wins else datas[k]
            assert (int(kinds[k]), int(lens[k]), int(crcs[k])) == (int(wins), 12 + len(payload), zlib.crc32(payload)), cases[i][0]
            assert out[int(offs[k]) + 12:int(offs[k]) + int(lens[k])].tobytes() == payload, cases[i][0]
        assert est["blobs"] == [int((kinds == 0).sum()), int((kinds == 1).sum())] and est["blobs"][1] >= 40
        digests = np.stack([np.frombuffer(hashlib.sha256(d).digest(), np.uint8) for d in datas])
        U._check_blobs(eng1, dst, out, offs[:-1], lens, kinds, crcs, datas, digests)
    finally:
        dst.free()


def test_a_room_one_byte_short_is_refused_and_nothing_is_written_outside(world, first):
    eng1, _, cases, dev, ranges = world
    _, _, frames, _, _ = first
    names = [c[0] for c in cases]
    pick = [names.index(n) for n in ("text-4096", "mixed-300000", "rand-255", "touch-131073", "byte-5", "records-20000")]
    rooms = [zi.bound(len(cases[i][1])) for i in pick]
    rooms[1] = len(frames[pick[1]]) - 1  # one byte short
    rooms[3] = len(frames[pick[3]]) - 1
    rooms[5] = 0
    status, flen, got, dst, _ = _encode(eng1, dev, ranges[pick], rooms)  # (checks the guards around every room)
    dst.free()
    assert list(status) == [OK, BAD_SIZE, OK, BAD_SIZE, OK, BAD_SIZE]
    assert flen[1] == 0 and flen[3] == 0 and flen[5] == 0
    for k in (0, 2, 4):
        assert got[k][:int(flen[k])].tobytes() == frames[pick[k]], names[pick[k]]


@pytest.fixture(scope="module")
def held(gpu_lib):
    """a holding ring of the engine with the option: 1 MiB of the mix at NewConfig(4096) in 64 KiB pages, cuts asked for
    around the seams, nothing released"""
    page, n = 65536, 1 << 20
    host = U._mix(n, 7)
    mp = pytest.MonkeyPatch()
    mp.setattr(U, "_engine", _tables_engine)
    mp.setenv("PBSGPU_RING_IDLE_TIMEOUT_S", "10")
    try:
        eng, ring, sid, recs = U._held(4096, page, 64, host, U._seam_suggestions(n, page, 1024))
    finally:
        mp.undo()
    yield eng, ring, sid, recs, host
    ring.close_stream(sid)
    ring.close()
    eng.close()


def test_the_ring_call_with_half_the_records_known_and_chunks_in_two_pages(held):
    """U._Twins.check: the fused call against classify + copy + blob_encode2 on the same engine, every compressed frame
    against zstd_encode of the chunk's bytes on the same engine, every blob back through blob_decode2"""
    from pbs_plus_amd import Engine, buzhash

    eng, ring, sid, recs, host = held
    tw = U._Twins(eng, recs[::2])
    flags = tw.check(ring, sid, recs, U._single(host, recs), insert=True)
    print("kinds", tw.kinds, "known", tw.nknown, "in two pages", len(tw.firsts))
    assert tw.kinds[0] >= 10 and tw.kinds[1] >= 10 and tw.nknown >= recs.size // 2 and len(tw.firsts) >= 4
    # the option is what made these frames: a default engine needs more bytes for the same new chunks
    new = np.flatnonzero(flags == 0)
    ends, sizes = recs["end"].astype(np.uint64)[new], recs["size"].astype(np.uint64)[new]
    eng0 = Engine(buzhash.NewConfig(4096), device=0)
    buf0, buf1 = eng0.alloc(host.size), eng.alloc(host.size)
    try:
        totals = []
        for e, b in ((eng0, buf0), (eng, buf1)):
            b.upload(host)
            d, offs, lens, kinds, crcs, est = e.blob_encode2(b, np.stack([ends - sizes, sizes], axis=1), nbytes=host.size, zstd=True)
            d.free()
            totals.append(est["frame_bytes"])
        print("frame bytes, default and with the option", totals)
        assert totals[1] < totals[0]
    finally:
        buf0.free()
        buf1.free()
        eng0.close()
        tw.close()


def test_a_destination_too_small_leaves_it_and_the_set_untouched(held):
    from pbs_plus_amd import _lib

    eng, ring, sid, recs, host = held
    tw = U._Twins(eng, recs[1::2])
    want_flags, want_st = tw.twin.classify(recs, insert=False)
    new = want_flags == 0
    needed = int(recs["size"][new].astype(np.uint64).sum()) + 12 * int(new.sum())
    before = len(tw.fused)
    g = U._guarded(eng, needed)
    rc, flags, offs, lens, kinds, crcs, used, st, est = U._raw(ring, tw.fused, sid, recs, 1, 1, g.ptr + 64, needed - 1)
    assert rc == _lib.E_CAPACITY and used == needed
    assert np.all(g.download() == 0xA5)
    assert len(tw.fused) == before and np.array_equal(flags, want_flags) and st == want_st
    assert U._untouched(np.full(1, U.SENT_FLAG), offs, lens, kinds, crcs) and est["blobs"] == [0, 0]
    rc, flags, offs, lens, kinds, crcs, used, st, est = U._raw(ring, tw.fused, sid, recs, 1, 1, g.ptr + 64, needed)
    assert rc == 0 and used == needed and np.array_equal(flags, want_flags)
    out = g.download()
    assert np.all(out[:64] == 0xA5) and np.all(out[64 + needed:] == 0xA5)
    assert est["blobs"][1] > 0 and len(tw.fused) == before + int(new.sum())
    g.free()
    tw.close()


def test_the_contiguous_call_against_blob_encode2_of_the_same_engine(gpu_lib):
    """chunks of the crafted contents and of text at the lengths around a block's edge, half of the digests known"""
    from pbs_plus_amd import RECORD_DTYPE

    names = ("touch-131072", "touch-131073", "touch-300000", "records-20000", "text-131073", "text-4096", "rand-255", "ofrle",
             "llrle", "seqs-2", "text-5", "mixed-300000")
    parts, ranges, pos = [], [], 0
    for k, name in enumerate(names):
        gap = (-pos) % 16 + (0, 1, 3, 8)[k % 4]
        chunk = np.frombuffer(ti.content_of(name), np.uint8)
        parts += [np.zeros(gap, dtype=np.uint8), chunk]
        ranges.append((pos + gap, chunk.size))
        pos += gap + chunk.size
    host = np.concatenate(parts)
    chunks = np.array(ranges, dtype=np.uint64)
    recs = np.zeros(len(ranges), dtype=RECORD_DTYPE)
    recs["size"] = chunks[:, 1]
    recs["end"] = np.cumsum(chunks[:, 1])
    datas = [host[o:o + n].tobytes() for o, n in ranges]
    for i, d in enumerate(datas):
        recs["digest"][i] = np.frombuffer(hashlib.sha256(d).digest(), np.uint8)
    eng = _tables_engine(4096)
    buf = eng.alloc(host.size)
    buf.upload(host)
    tw = U._Twins(eng, recs[1::2])
    try:
        flags2, st2 = tw.twin.classify(recs, insert=True)
        new = flags2 == 0
        assert new.sum() == len(names) // 2
        dst, flags, offs, lens, kinds, crcs, st, est = tw.fused.upload_new2(buf, recs, chunks, insert=True, zstd=True, nbytes=host.size)
        dst2, offs2, lens2, kinds2, crcs2, est2 = eng.blob_encode2(buf, chunks[new], nbytes=host.size, zstd=True)
        try:
            assert np.array_equal(flags, flags2) and st == st2 and len(tw.fused) == len(tw.twin)
            assert dst.used == int(offs2[-1]) and est == est2
            assert np.array_equal(offs[new], offs2[:-1]) and np.array_equal(lens[new], lens2)
            assert np.array_equal(kinds[new], kinds2) and np.array_equal(crcs[new], crcs2)
            assert not offs[~new].any() and not lens[~new].any() and not kinds[~new].any() and not crcs[~new].any()
            out, out2 = dst.download(0, dst.used), dst2.download(0, dst.used)
            golden = ti.golden()
            for i in np.flatnonzero(new):
                o, ln = int(offs[i]), int(lens[i])
                assert out[o:o + ln].tobytes() == out2[o:o + ln].tobytes(), names[i]
                if kinds[i]:
                    frame = out[o + 12:o + ln].tobytes()
                    assert [len(frame), hashlib.sha256(frame).hexdigest()] == golden[names[i]], names[i]
            assert est["blobs"][1] >= 4
            U._check_blobs(eng, dst, out, offs[new], lens[new], kinds[new], crcs[new], [datas[i] for i in np.flatnonzero(new)],
                           recs["digest"][new])
        finally:
            dst.free()
            dst2.free()
    finally:
        tw.close()
        buf.free()
        eng.close()
