"""Blobs whose kind the device decides (pbsgpu_blob_encode2_device, Engine.blob_encode2): 40 chunks of mixed kinds and
sizes. Without the flag the call is pbsgpu_blob_encode_device output for output. With it a chunk is a compressed blob
exactly where the golden frame (tests/golden/zstd_enc_v1.json) is shorter than the chunk, every blob is magic + CRC-32 of
its payload + payload in the slot the uncompressed layout gives it, nothing outside the slots is written, the statistics
add up, and pbsgpu_blob_decode2_device restores the source bytes from these blobs."""
import hashlib
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_enc_inputs as zi  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
NAMES = ["%s-%d" % (k, n) for k in ("text", "many", "rand", "byte", "period3", "zeros", "text10") for n in (1, 5, 255, 65_792, 131_073)]
NAMES += ["mixed-4096", "mixed-300000", "text-4096", "seqs-128", "cap"]


class _View:
    def __init__(self, ptr, nbytes):
        self.ptr, self.nbytes = ptr, nbytes


@pytest.fixture(scope="module")
def world():
    """(engine, [(name, content)], device source, chunk ranges, guarded destination buffer, total of the slots)"""
    from pbs_plus_amd import Engine, buzhash

    eng = Engine(buzhash.NewConfig(4096), device=0)
    by_name = dict(zi.cases())
    cases = [(n, by_name[n]) for n in NAMES]
    assert len(cases) == 40
    rng = np.random.default_rng(10)
    parts, ranges, pos = [], [], 0
    for _, data in cases:
        gap = int(rng.integers(0, 7))
        parts.append(bytes(gap) + data)
        ranges.append((pos + gap, len(data)))
        pos += gap + len(data)
    host = np.frombuffer(b"".join(parts), np.uint8)
    dev = eng.alloc(host.size)
    dev.upload(host)
    total = sum(12 + len(d) for _, d in cases)
    buf = eng.alloc(total + 2 * GUARD)
    yield eng, cases, dev, np.array(ranges, dtype=np.uint64), buf, total
    buf.free()
    dev.free()
    eng.close()


def _run(world, zstd, cap=None):
    """blob_encode2 into the guarded buffer: (the slots' bytes, offsets, lens, kinds, crcs, stats)"""
    eng, cases, dev, ranges, buf, total = world
    buf.upload(np.full(total + 2 * GUARD, FILL, np.uint8))
    view = _View(buf.ptr + GUARD, total if cap is None else cap)
    try:
        _, offs, lens, kinds, crcs, stats = eng.blob_encode2(dev, ranges, dst=view, zstd=zstd)
    finally:
        got = buf.download(0, total + 2 * GUARD)
        assert np.all(got[:GUARD] == FILL) and np.all(got[GUARD + total:] == FILL), "guards around dst"
    return got[GUARD:GUARD + total], offs, lens, kinds, crcs, stats


def test_without_the_flag_it_is_blob_encode(world):
    eng, cases, dev, ranges, buf, total = world
    old, offs_old, crcs_old = eng.blob_encode(dev, ranges)
    try:
        want = old.download(0, total)
    finally:
        old.free()
    got, offs, lens, kinds, crcs, stats = _run(world, zstd=False)
    assert np.array_equal(got, want) and np.array_equal(offs, offs_old) and np.array_equal(crcs, crcs_old)
    assert np.array_equal(lens, 12 + ranges[:, 1]) and np.all(kinds == 0)
    assert stats["blobs"] == [40, 0] and stats["blob_bytes"] == [total, 0] and stats["frame_bytes"] == 0
    assert stats["crc_bytes"] == total - 12 * 40


def test_with_the_flag_the_device_decides_the_kind(world):
    from pbs_plus_amd import blob_magic

    eng, cases, dev, ranges, buf, total = world
    golden = zi.golden()
    got, offs, lens, kinds, crcs, stats = _run(world, zstd=True)
    assert int(offs[0]) == 0 and int(offs[-1]) == total
    want_stats = dict(blobs=[0, 0], blob_bytes=[0, 0], chunk_bytes=[0, 0], frame_bytes=0, crc_bytes=0)
    for i, (name, data) in enumerate(cases):
        flen, sha = golden[name]
        k = 1 if flen < len(data) else 0
        assert kinds[i] == k, name
        assert int(offs[i + 1] - offs[i]) == 12 + len(data)
        blob = got[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes()
        payload = blob[12:]
        assert blob[:8] == blob_magic(k) and int.from_bytes(blob[8:12], "little") == zlib.crc32(payload) == crcs[i], name
        if k:
            assert len(payload) == flen and hashlib.sha256(payload).hexdigest() == sha, name
        else:
            assert payload == data, name
        want_stats["blobs"][k] += 1
        want_stats["blob_bytes"][k] += len(blob)
        want_stats["chunk_bytes"][k] += len(data)
        want_stats["frame_bytes"] += len(payload) if k else 0
        want_stats["crc_bytes"] += len(payload)
    assert stats == want_stats
    assert 0 < want_stats["blobs"][0] < 40  # both kinds occur


def test_blob_decode2_restores_the_source_from_these_blobs(world):
    from pbs_plus_amd import RECORD_DTYPE

    eng, cases, dev, ranges, buf, total = world
    got, offs, lens, kinds, crcs, stats = _run(world, zstd=True)
    blobs = np.stack([GUARD + offs[:-1], lens.astype(np.uint64)], axis=1)
    idx = np.zeros(len(cases), dtype=RECORD_DTYPE)
    sizes = np.array([len(d) for _, d in cases], dtype=np.uint64)
    idx["size"] = sizes
    idx["end"] = np.cumsum(sizes)
    idx["digest"] = [np.frombuffer(hashlib.sha256(d).digest(), np.uint8) for _, d in cases]
    blob_of = np.arange(len(cases), dtype=np.uint32)
    out, status, st = eng.blob_decode2(buf, blobs, idx, blob_of, 0, int(idx["end"][-1]), True, zstd=True)
    try:
        back = out.download(0, int(idx["end"][-1]))
    finally:
        out.free()
    assert np.all(status == 0), [cases[i][0] for i in np.flatnonzero(status)]
    assert back.tobytes() == b"".join(d for _, d in cases)


def test_a_destination_one_byte_short_is_refused(world):
    from pbs_plus_amd import PbsGpuError, _lib

    eng, cases, dev, ranges, buf, total = world
    for zstd in (False, True):
        with pytest.raises(PbsGpuError) as e:
            _run(world, zstd=zstd, cap=total - 1)
        assert e.value.status == _lib.E_CAPACITY
