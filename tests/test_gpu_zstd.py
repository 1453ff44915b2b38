"""zstd frames decoded on the GPU (pbsgpu_zstd_decode_device, Engine.zstd_decode) against the golden frames of
tests/golden/zstd_v1*.npz: nothing here needs libzstd. Every destination lies between two guards of 64 bytes and is
pre-filled with the guard pattern, so a byte stored outside a frame's room is seen. The malformed frames are the
hand-assembled ones (three truncations of a raw-block frame among them), three truncations of a compressed fixture and
three single-byte mutations, each with the status that the sanitizer run of the
same format core recorded for it (tests/test_zstd_core_native.py); the fuzz corpus itself stays on the CPU."""
import hashlib
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
BAD_ROOM = 4096  # what a frame nobody may accept gets to write into


class _View:
    """a window of a device allocation: what zstd_decode needs of a destination"""

    def __init__(self, ptr, nbytes):
        self.ptr, self.nbytes = ptr, nbytes


class _Guarded:
    """one allocation that serves as the guarded destination of many calls"""

    def __init__(self, eng, cap):
        self.eng, self.buf = eng, eng.alloc(cap + 2 * GUARD)

    def run(self, data, frames, out, need):
        """decode into dst[0, need) behind the front guard; (the need bytes, status, decoded)"""
        total = need + 2 * GUARD
        assert total <= self.buf.nbytes
        self.buf.upload(np.full(total, FILL, np.uint8))
        # the capacity reaches over the guard behind: room that no `out` names and that must not be used
        view = _View(self.buf.ptr + GUARD, need + GUARD)
        try:
            _, status, decoded, _ = self.eng.zstd_decode(data, frames, out=out, dst=view)
        finally:
            got = self.buf.download(0, total)
            assert np.all(got[:GUARD] == FILL), "guard in front of dst"
            assert np.all(got[GUARD + need:] == FILL), "guard behind dst"
        return got[GUARD:GUARD + need], status, decoded

    def free(self):
        self.buf.free()


@pytest.fixture(scope="module")
def world():
    """(engine, cases, device buffer of all frames 0-6 bytes apart, frame ranges, guarded destination)"""
    from pbs_plus_amd import Engine, buzhash

    eng = Engine(buzhash.NewConfig(4096), device=0)
    cases = zstd_inputs.cases()
    extra = [dict(name="mutated-%d" % k, frame=zstd_inputs.mutated(next(c for c in cases if c["name"] == name)["frame"], at, xor),
                  status=status, length=decoded, crc=crc, content=None, room=next(c for c in cases if c["name"] == name)["length"])
             for k, (name, at, xor, status, decoded, crc) in enumerate(zstd_inputs.MUTATIONS)]
    extra += [dict(name="cut-%d" % k, frame=next(c for c in cases if c["name"] == name)["frame"][:length], status=status, length=0,
                   content=None, room=next(c for c in cases if c["name"] == name)["length"])
              for k, (name, length, status) in enumerate(zstd_inputs.CUTS)]
    allc = cases + extra
    rng = np.random.default_rng(7)
    parts, ranges, pos = [], [], 0
    for c in allc:
        gap = int(rng.integers(0, 7))
        parts.append(bytes(gap) + c["frame"])
        ranges.append((pos + gap, len(c["frame"])))
        pos += gap + len(c["frame"])
    host = np.frombuffer(b"".join(parts), np.uint8)
    dev = eng.alloc(host.size)
    dev.upload(host)
    room = sum(_room(c) + 7 for c in allc)
    g = _Guarded(eng, room)
    yield eng, allc, dev, np.array(ranges, dtype=np.uint64), g
    g.free()
    dev.free()
    eng.close()


def _room(c):
    if "room" in c:  # a mutated frame gets the room it had in the sanitizer run: its case's
        return c["room"]
    return c["length"] if c["status"] == 0 else BAD_ROOM


def _check(c, status, decoded, got):
    assert status == c["status"], (c["name"], status)
    if c["status"] != 0:
        assert decoded == 0, c["name"]
        return
    assert decoded == c["length"], (c["name"], decoded)
    if c["content"] is None:  # a mutated frame that still decodes: the sanitizer run recorded what to
        assert zlib.crc32(got.tobytes()) == c["crc"], c["name"]
        return
    assert hashlib.sha256(got.tobytes()).digest() == c["sha256"], c["name"]
    assert got.tobytes() == c["content"], c["name"]


NAMES = [c["name"] for c in zstd_inputs.golden().load()]


@pytest.mark.parametrize("name", [n for n in NAMES if not n.startswith("bad-")])
def test_every_fixture_decodes_bit_exact_alone(world, name):
    eng, allc, dev, ranges, g = world
    i = [c["name"] for c in allc].index(name)
    c = allc[i]
    got, status, decoded = g.run(dev, ranges[i:i + 1], [(0, c["length"])], c["length"])
    _check(c, int(status[0]), int(decoded[0]), got)


def test_all_fixtures_in_one_call_with_scrambled_destinations(world):
    eng, allc, dev, ranges, g = world
    rng = np.random.default_rng(11)
    order = rng.permutation(len(allc))
    out, pos = np.zeros((len(allc), 2), dtype=np.uint64), 0
    for i in order:  # frame i's room lies where the permutation puts it, 1-7 untouchable bytes behind it
        out[i] = (pos, _room(allc[i]))
        pos += _room(allc[i]) + int(rng.integers(1, 8))
    got, status, decoded = g.run(dev, ranges, out, pos)
    used = np.zeros(pos, dtype=bool)
    for i, c in enumerate(allc):
        a, n = int(out[i, 0]), int(out[i, 1])
        used[a:a + n] = True
        _check(c, int(status[i]), int(decoded[i]), got[a:a + n])
    assert np.all(got[~used] == FILL), "bytes between the rooms"


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("bad-")] + ["mutated-%d" % k for k in range(len(zstd_inputs.MUTATIONS))] + ["cut-%d" % k for k in range(len(zstd_inputs.CUTS))])
def test_malformed_frames_report_their_status_inside_their_room(world, name):
    eng, allc, dev, ranges, g = world
    i = [c["name"] for c in allc].index(name)
    c = allc[i]
    got, status, decoded = g.run(dev, ranges[i:i + 1], [(0, _room(c))], _room(c))
    _check(c, int(status[0]), int(decoded[0]), got)


def test_a_room_one_byte_too_small_and_no_frames_at_all(world):
    eng, allc, dev, ranges, g = world
    i = [c["name"] for c in allc].index("text-60000-level1")
    got, status, decoded = g.run(dev, ranges[i:i + 1], [(0, allc[i]["length"] - 1)], allc[i]["length"] - 1)
    assert int(status[0]) == zstd_inputs.BAD_SIZE and int(decoded[0]) == 0
    _, status, decoded, _ = eng.zstd_decode(dev, np.zeros((0, 2), np.uint64), out=np.zeros((0, 2), np.uint64), dst=_View(g.buf.ptr, 16))
    assert status.size == 0 and decoded.size == 0


def test_the_default_form_sizes_and_allocates_by_itself(world):
    """out=None lays the frames out back to back by their declared content sizes (one read-back of the headers), dst=None
    allocates; a frame that declares no size is a ValueError before anything is decoded"""
    eng, allc, dev, ranges, g = world
    names = [c["name"] for c in allc]
    pick = [names.index(n) for n in ("text-3", "mixed-1048576-level3", "text-0", "bad-magic", "hand-fcs8", "text-131073", "bad-truncated-3")]
    dst, status, decoded, out = eng.zstd_decode(dev, ranges[pick])
    try:
        want = [allc[i]["length"] for i in pick]
        assert out[:, 1].tolist() == want and out[:, 0].tolist() == [sum(want[:k]) for k in range(len(pick))]
        assert dst.nbytes >= sum(want)
        got = dst.download(0, sum(want))
        for k, i in enumerate(pick):
            a = int(out[k, 0])
            _check(allc[i], int(status[k]), int(decoded[k]), got[a:a + want[k]])
    finally:
        dst.free()
    with pytest.raises(ValueError):
        eng.zstd_decode(dev, ranges[[names.index("text-3"), names.index("text-50000-nosize")]])
    dst, status, decoded, out = eng.zstd_decode(dev, np.zeros((0, 2), np.uint64))
    assert status.size == 0 and out.shape == (0, 2)
    dst.free()


def test_argument_checks_that_need_the_device(world):
    from pbs_plus_amd import PbsGpuError, _lib

    eng, allc, dev, ranges, g = world
    i = [c["name"] for c in allc].index("hand-raw-block")
    fr = ranges[i:i + 1]
    before = g.buf.download(0, 256).copy()

    def bad(**kw):
        args = dict(data=dev, frames=fr, out=[(0, 78)], dst=_View(g.buf.ptr, 256))
        args.update(kw)
        with pytest.raises(PbsGpuError) as e:
            eng.zstd_decode(**args)
        assert e.value.status == _lib.E_INVALID

    bad(out=[(200, 78)])                                       # a room outside dst_cap
    bad(frames=[(dev.nbytes - 10, 78)])                        # a frame outside src
    bad(frames=np.concatenate([fr, fr]), out=[(0, 78), (77, 78)])  # rooms that overlap
    bad(dst=_View(dev.ptr + 8, 256))                           # a destination inside the source
    host = np.zeros(256, np.uint8)
    bad(dst=_View(host.ctypes.data, 256))                      # a host pointer
    assert np.array_equal(g.buf.download(0, 256), before)
