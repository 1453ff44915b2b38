"""The zstd content checksum and whole streams on the GPU (pbsgpu_xxh64_many_device, pbsgpu_zstd_decode2_device,
pbsgpu_zstd_encode2_device) against tests/golden/zstd_checksum_v1.json and the `xxhash` module: nothing here needs libzstd.
Every destination is pre-filled with a guard pattern and every room lies between two guards of 64 bytes, so a byte stored
outside a room is seen. The cases are those of the sanitizer run of the same format cores
(tests/test_zstd_checksum_native.py); the fuzz corpus itself stays on the CPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_checksum_inputs as zi  # noqa: E402
import zstd_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5


@pytest.fixture(scope="module")
def eng():
    from pbs_plus_amd import Engine, buzhash

    e = Engine(buzhash.NewConfig(4096), device=0)
    yield e
    e.close()


def _run(eng, call, items):
    """items = [(source bytes, room)]: the sources 0-6 bytes apart in one device buffer, every room between two guards in
    another that is pre-filled with the pattern; call(src, ranges, out, dst) -> (status, lengths). Returns per item
    (status, length, the room's bytes) after checking that every byte outside the rooms is still the pattern."""
    rng = np.random.default_rng(len(items))
    parts, ranges, pos = [], [], 0
    for data, _ in items:
        gap = int(rng.integers(0, 7))
        parts.append(bytes(gap) + data)
        ranges.append((pos + gap, len(data)))
        pos += gap + len(data)
    host = np.frombuffer(b"".join(parts) + bytes(16), np.uint8)
    out, at = [], GUARD
    for _, room in items:
        out.append((at, room))
        at += room + GUARD
    src, dst = eng.alloc(host.size), eng.alloc(at)
    try:
        src.upload(host)
        dst.upload(np.full(at, FILL, np.uint8))
        status, lens = call(src, np.array(ranges, dtype=np.uint64).reshape(-1, 2), np.array(out, dtype=np.uint64).reshape(-1, 2), dst)
        got = dst.download(0, at)
    finally:
        src.free()
        dst.free()
    keep = np.ones(at, dtype=bool)
    for o, room in out:
        keep[o:o + room] = False
    assert np.all(got[keep] == FILL), "a byte outside every room was written"
    return [(int(status[i]), int(lens[i]), got[o:o + room].tobytes()) for i, (o, room) in enumerate(out)]


def _decode2(eng, **kw):
    def call(src, ranges, out, dst):
        _, status, decoded, _ = eng.zstd_decode2(src, ranges, out=out, dst=dst, **kw)
        return status, decoded
    return call


def _decode(eng):
    def call(src, ranges, out, dst):
        _, status, decoded, _ = eng.zstd_decode(src, ranges, out=out, dst=dst)
        return status, decoded
    return call


# ---- 1. xxh64_many against xxhash --------------------------------------------------------------------------------------
def test_xxh64_many_matches_xxhash(eng):
    import xxhash

    rng = np.random.default_rng(64)
    n = (1 << 20) + 5 + 4200 + 9
    host = rng.integers(0, 256, size=n, dtype=np.uint8)
    dev = eng.alloc(n)
    try:
        dev.upload(host)
        data = host.tobytes()
        for seed in zi.XXH_SEEDS:
            # every length class at every alignment; one long range; ranges that overlap one another
            segs = [(base + 13 * k, ln) for k, ln in enumerate(zi.XXH_LENGTHS) for base in range(8)]
            segs += [(3, (1 << 20) + 5), (100, 4000), (150, 4000), (100, 4000), (0, 0), (n, 0), (n - 1, 1)]
            got = eng.xxh64_many(dev, segs, seed=seed)
            for (o, ln), h in zip(segs, got):
                assert int(h) == xxhash.xxh64(data[o:o + ln], seed=seed).intdigest(), (o, ln, seed)
        # 67 ranges in one call: four full waves of sixteen and a ragged fifth; lengths that differ inside a wave
        segs = [(int(rng.integers(0, 3000)), int(rng.integers(0, 1500))) for _ in range(67)]
        got = eng.xxh64_many(dev, segs)
        assert [int(h) for h in got] == [xxhash.xxh64(data[o:o + ln]).intdigest() for o, ln in segs]
        # a device pointer at an odd address
        odd = eng.xxh64_many(dev.ptr + 1, [(0, 4097), (6, 33), (7, 8)], nbytes=n - 1)
        assert [int(h) for h in odd] == [xxhash.xxh64(data[1 + o:1 + o + ln]).intdigest() for o, ln in ((0, 4097), (6, 33), (7, 8))]
        assert eng.xxh64_many(dev, []).size == 0
    finally:
        dev.free()


# ---- 2. flags = 0 is the old call ----------------------------------------------------------------------------------------
def test_decode2_without_flags_is_decode(eng):
    cases = zstd_inputs.cases()
    assert len(cases) >= 30 and {c["status"] for c in cases} == {0, 1, 2, 3}
    items = [(c["frame"], c["length"] if c["status"] == 0 else 4096) for c in cases]
    old = _run(eng, _decode(eng), items)
    new = _run(eng, _decode2(eng), items)
    for c, a, b in zip(cases, old, new):
        assert a[:2] == b[:2] == (c["status"], c["length"] if c["status"] == 0 else 0), (c["name"], a[:2], b[:2])
        assert a[2] == b[2], c["name"]  # every byte of the room, decoded or not
        if c["status"] == 0:
            assert a[2] == c["content"], c["name"]


# ---- 3. F_CHECKSUM ---------------------------------------------------------------------------------------------------------
def test_checksum_is_verified_where_the_old_call_says_ok(eng):
    good, bad = zi.frames(), zi.flipped()
    items = [(f["frame"], f["length"]) for f in good] + [(c["frame"], c["length"]) for c in bad]
    res = _run(eng, _decode2(eng, checksum=True), items)
    for f, (status, decoded, room) in zip(good, res):
        assert (status, decoded) == (zi.OK, f["length"]) and room == f["content"], f["name"]
    for c, (status, decoded, _) in zip(bad, res[len(good):]):
        assert (status, decoded) == (zi.BAD_CHECKSUM, 0), c["name"]
    # the same frames through the call that verifies nothing: OK, to bytes nobody vouches for
    for call in (_decode(eng), _decode2(eng)):
        for c, (status, decoded, _) in zip(bad, _run(eng, call, items)[len(good):]):
            assert (status, decoded) == (zi.OK, c["length"]), c["name"]
    # a frame without a checksum is unaffected by the flag
    plain = [c for c in zstd_inputs.cases() if c["status"] == 0 and not c["info"][4] and len(c["frame"]) <= 30_000][:8]
    for c, (status, decoded, room) in zip(plain, _run(eng, _decode2(eng, checksum=True), [(c["frame"], c["length"]) for c in plain])):
        assert (status, decoded) == (zi.OK, c["length"]) and room == c["content"], c["name"]


# ---- 4. F_STREAM -----------------------------------------------------------------------------------------------------------
def test_streams_decode_as_zstd_decompress_does_it(eng):
    streams = zi.streams()
    items = [(s["stream"], s["room"]) for s in streams]
    res = _run(eng, _decode2(eng, checksum=True, stream=True), items)
    for s, (status, decoded, room) in zip(streams, res):
        assert status == s["status"], (s["name"], status)
        assert decoded == len(s["content"]), s["name"]
        if status == zi.OK:
            assert room == s["content"], s["name"]
    by = {s["name"]: r for s, r in zip(streams, res)}
    assert by["skip-alone"][:2] == (zi.OK, 0) and by["empty"][:2] == (zi.OK, 0)
    # without F_CHECKSUM a stream's bad checksum goes unseen; without F_STREAM a stream is what it always was
    two = next(s for s in streams if s["name"] == "two")
    bad = next(s for s in streams if s["name"] == "second-bad-checksum")
    (status, decoded, room), = _run(eng, _decode2(eng, stream=True), [(bad["stream"], bad["room"])])
    assert (status, decoded) == (zi.OK, len(two["content"])) and room[:decoded] == two["content"]
    for call in (_decode2(eng, checksum=True), _decode(eng)):
        (status, decoded, _), = _run(eng, call, [(two["stream"], two["room"])])
        assert (status, decoded) == (zi.UNSUPPORTED, 0)
    (status, decoded, _), = _run(eng, _decode2(eng, stream=True), [(two["stream"], two["room"] - 1)])
    assert (status, decoded) == (zi.BAD_SIZE, 0)


def test_every_workgroup_takes_a_second_and_a_third_segment(eng):
    """3 x grid + 1 small segments (the grid is four workgroups per CU): every workgroup decodes a second and a third segment
    with a State and a walk that the one before has used, and what it used them for differs from segment to segment"""
    grid = 256 * 4  # an MI355X has 256 CUs; with fewer (a partition) every workgroup takes more segments still
    kinds = [s for s in zi.streams() if len(s["stream"]) <= 4000]
    kinds += [dict(name=f["name"], stream=f["frame"], status=zi.OK, content=f["content"], room=f["length"])
              for f in zi.frames() if len(f["frame"]) <= 2000]
    kinds += [dict(name=c["name"], stream=c["frame"], status=zi.BAD_CHECKSUM, content=b"", room=c["length"])
              for c in zi.flipped() if len(c["frame"]) <= 2000]
    assert len(kinds) >= 12 and {k["status"] for k in kinds} >= {zi.OK, zi.BAD_CHECKSUM, zi.BAD_FRAME}
    n = 3 * grid + 1
    order = [kinds[(7 * i + i // len(kinds)) % len(kinds)] for i in range(n)]
    res = _run(eng, _decode2(eng, checksum=True, stream=True), [(k["stream"], k["room"]) for k in order])
    for i, (k, (status, decoded, room)) in enumerate(zip(order, res)):
        assert (status, decoded) == (k["status"], len(k["content"])), (i, k["name"], status, decoded)
        if status == zi.OK:
            assert room[:decoded] == k["content"], (i, k["name"])


# ---- 5. encode2 with the flag ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [{}, {"zstd_seq_tables": 1}, {"zstd_window_log": 17}], ids=["default", "tables", "window17"])
def test_encode2_writes_the_checksum(options):
    import xxhash
    from pbs_plus_amd import Engine, buzhash, zstd_encode_bound, zstd_encode_bound2

    e = Engine(buzhash.NewConfig(4096), device=0, options=options) if options else Engine(buzhash.NewConfig(4096), device=0)
    try:
        contents = [zi.enc_content(name, n) for name, n in zi.ENC_CONTENTS]

        def encode(**kw):
            def call(src, ranges, out, dst):
                fn = e.zstd_encode2 if kw else e.zstd_encode
                _, status, flen, _ = fn(src, ranges, out=out, dst=dst, **kw)
                return status, flen
            return call

        plain = _run(e, encode(), [(c, zstd_encode_bound(len(c))) for c in contents])
        same = _run(e, encode(checksum=False), [(c, zstd_encode_bound(len(c))) for c in contents])
        summed = _run(e, encode(checksum=True), [(c, zstd_encode_bound2(len(c), True)) for c in contents])
        frames = []
        for c, p, q, s in zip(contents, plain, same, summed):
            assert p[0] == q[0] == s[0] == zi.OK, len(c)
            old = p[2][:p[1]]
            assert q[1] == p[1] and q[2] == p[2], len(c)  # flags = 0 is the old call
            want = old[:4] + bytes([old[4] | 4]) + old[5:] + (xxhash.xxh64(c).intdigest() & 0xFFFFFFFF).to_bytes(4, "little")
            assert not old[4] & 4 and s[1] == p[1] + 4 and s[2][:s[1]] == want, len(c)
            frames.append(want)
        back = _run(e, _decode2(e, checksum=True), [(f, len(c)) for f, c in zip(frames, contents)])
        for c, (status, decoded, room) in zip(contents, back):
            assert (status, decoded) == (zi.OK, len(c)) and room == c, len(c)
        # a room one byte short of the bound: random content and the empty frame need all of it
        tight = [c for c, (name, n) in zip(contents, zi.ENC_CONTENTS) if n == 0 or name == "rand"]
        assert len(tight) == 3
        for c, (status, flen, _) in zip(tight, _run(e, encode(checksum=True), [(c, zstd_encode_bound2(len(c), True) - 1) for c in tight])):
            assert (status, flen) == (zi.BAD_SIZE, 0), len(c)
    finally:
        e.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_dst_untouched(eng):
    from pbs_plus_amd import PbsGpuError, _lib

    f = zi.frame("lowsym-3000-level1")
    host = np.frombuffer(f["frame"] + bytes(64), np.uint8)
    src, dst = eng.alloc(host.size), eng.alloc(8192)
    try:
        src.upload(host)
        dst.upload(np.full(8192, FILL, np.uint8))
        fr = np.array([[0, len(f["frame"])], [0, len(f["frame"])]], dtype=np.uint64)
        out = np.array([[0, 3000], [4000, 3000]], dtype=np.uint64)
        status, lens = np.full(2, 9, np.uint8), np.full(2, 9, np.uint64)
        L = eng._L

        def dec(flags, sp=src.ptr, dp=dst.ptr, o=out):
            return L.pbsgpu_zstd_decode2_device(eng._h, sp, src.nbytes, fr.ctypes.data, 2, o.ctypes.data, dp, 8192, status.ctypes.data,
                                                lens.ctypes.data, flags)

        def enc(flags, sp=src.ptr, dp=dst.ptr, o=out):
            return L.pbsgpu_zstd_encode2_device(eng._h, sp, src.nbytes, fr.ctypes.data, 2, o.ctypes.data, dp, 8192, status.ctypes.data,
                                                lens.ctypes.data, flags)

        overlap = np.array([[0, 3000], [2999, 3000]], dtype=np.uint64)
        for fn, ok in ((dec, (0, 1, 2, 3)), (enc, (0, 1))):
            for flags in (4, 8, 0x80000000) + ((2, 3) if fn is enc else ()):
                assert fn(flags) == _lib.E_INVALID
            for flags in ok:
                assert fn(flags, sp=host.ctypes.data) == _lib.E_INVALID   # a host pointer for the source
                assert fn(flags, dp=host.ctypes.data) == _lib.E_INVALID   # ... and for the destination
                assert fn(flags, o=overlap) == _lib.E_INVALID             # rooms that share a byte
                assert fn(flags, dp=src.ptr) == _lib.E_INVALID            # a destination inside the source
        hashes = np.full(2, 9, np.uint64)
        assert L.pbsgpu_xxh64_many_device(eng._h, host.ctypes.data, host.size, fr.ctypes.data, 2, 0, hashes.ctypes.data) == _lib.E_INVALID
        assert np.all(status == 9) and np.all(lens == 9) and np.all(hashes == 9)
        assert np.all(dst.download(0, 8192) == FILL)
        with pytest.raises(ValueError):
            eng.zstd_decode2(src, fr, stream=True)  # a stream's room comes from the caller
        assert issubclass(PbsGpuError, Exception)
    finally:
        src.free()
        dst.free()
