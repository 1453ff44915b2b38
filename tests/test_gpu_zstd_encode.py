"""zstd frames written on the GPU (pbsgpu_zstd_encode_device, Engine.zstd_encode): every case of tests/zstd_enc_inputs.py in
one call, the chunks 0-6 bytes apart in the source, each room exactly zstd_encode_bound(n) between guards of 64 bytes of
a pattern. The frames must be the ones of tests/golden/zstd_enc_v1.json, byte for byte what the CPU build of the same
format core writes under sanitizers and what libzstd decodes there (tests/test_zstd_encode_native.py); here the device's
own decoder gives the contents back. Nothing here needs libzstd or a compiler."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_enc_inputs as zi  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
OK, BAD_SIZE = 0, 2


@pytest.fixture(scope="module")
def world():
    """(engine, cases, device buffer of all contents 0-6 bytes apart, their ranges)"""
    from pbs_plus_amd import Engine, buzhash

    eng = Engine(buzhash.NewConfig(4096), device=0)
    cases = zi.cases()
    rng = np.random.default_rng(9)
    parts, ranges, pos = [], [], 0
    for _, data in cases:
        gap = int(rng.integers(0, 7))
        parts.append(bytes(gap) + data)
        ranges.append((pos + gap, len(data)))
        pos += gap + len(data)
    host = np.frombuffer(b"".join(parts), np.uint8)
    dev = eng.alloc(host.size)
    dev.upload(host)
    yield eng, cases, dev, np.array(ranges, dtype=np.uint64)
    dev.free()
    eng.close()


def _encode(eng, dev, ranges, rooms):
    """one call with room i of rooms[i] bytes between guards: (status, frame lengths, [the room's bytes], dst, out); the
    guards are checked here. The caller frees dst."""
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
    """every case in one call: (status, frame lengths, frames as bytes)"""
    eng, cases, dev, ranges = world
    status, flen, rooms, dst, out = _encode(eng, dev, ranges, [zi.bound(len(d)) for _, d in cases])
    frames = [rooms[i][:int(flen[i])].tobytes() for i in range(len(cases))]
    yield status, flen, frames, dst, out
    dst.free()


def test_every_frame_is_the_golden_one(world, first):
    eng, cases, dev, ranges = world
    status, flen, frames, _, _ = first
    golden = zi.golden()
    assert np.all(status == OK), [cases[i][0] for i in np.flatnonzero(status != OK)]
    for (name, data), frame in zip(cases, frames):
        assert 0 < len(frame) <= zi.bound(len(data)), name
        assert [len(frame), hashlib.sha256(frame).hexdigest()] == golden[name], name


def test_the_device_decoder_gives_the_contents_back(world, first):
    eng, cases, dev, ranges = world
    status, flen, frames, dst, out = first
    fr = np.stack([out[:, 0], flen], axis=1)
    sizes = np.array([len(d) for _, d in cases], dtype=np.uint64)
    ends = np.cumsum(sizes)
    back, st, decoded, _ = eng.zstd_decode(dst, fr, out=np.stack([ends - sizes, sizes], axis=1))
    try:
        got = back.download(0, max(int(ends[-1]), 1))
    finally:
        back.free()
    assert np.all(st == OK) and np.array_equal(decoded, sizes)
    assert got[:int(ends[-1])].tobytes() == b"".join(d for _, d in cases)


def test_the_output_does_not_depend_on_the_grid_or_on_neighbours(world, first):
    eng, cases, dev, ranges = world
    _, _, frames, _, _ = first
    n = len(cases)
    rev = np.arange(n)[::-1]
    status, flen, rooms, dst, _ = _encode(eng, dev, ranges[rev], [zi.bound(len(cases[i][1])) for i in rev])
    dst.free()
    assert np.all(status == OK)
    for k, i in enumerate(rev):
        assert rooms[k][:int(flen[k])].tobytes() == frames[i], cases[i][0]
    for name in ("text-300000", "zeros-0"):
        i = [c[0] for c in cases].index(name)
        status, flen, rooms, dst, _ = _encode(eng, dev, ranges[i:i + 1], [zi.bound(len(cases[i][1]))])
        dst.free()
        assert status[0] == OK and rooms[0][:int(flen[0])].tobytes() == frames[i], name


def test_rooms_too_small_are_refused_and_the_others_unaffected(world, first):
    eng, cases, dev, ranges = world
    _, _, frames, _, _ = first
    names = [c[0] for c in cases]
    pick = [names.index(n) for n in ("text-4096", "mixed-300000", "rand-255", "text10-131073", "byte-5", "many-65792")]
    rooms = [zi.bound(len(cases[i][1])) for i in pick]
    rooms[1] = len(frames[pick[1]]) - 1  # one byte short
    rooms[3] = 0
    status, flen, got, dst, _ = _encode(eng, dev, ranges[pick], rooms)
    dst.free()
    assert list(status) == [OK, BAD_SIZE, OK, BAD_SIZE, OK, OK]
    assert flen[1] == 0 and flen[3] == 0
    for k in (0, 2, 4, 5):
        assert got[k][:int(flen[k])].tobytes() == frames[pick[k]], names[pick[k]]


def test_no_chunks_is_ok(world):
    eng, cases, dev, ranges = world
    dst, status, flen, out = eng.zstd_encode(dev, np.zeros((0, 2), np.uint64))
    dst.free()
    assert status.size == 0 and flen.size == 0
