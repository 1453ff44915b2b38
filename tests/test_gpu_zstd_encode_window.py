"""The zstd encoder's long-range match finder on the GPU: engines created with zstd_window_log = 17 and 19, each without
and with zstd_seq_tables, beside a default engine in the same process. pbsgpu_zstd_encode_device must write the frames of
tests/golden/zstd_enc_window_v1.json (what the CPU build of the same format core writes under sanitizers and libzstd
decodes, tests/test_zstd_encode_window_native.py) for contents with far repeats and for those crafted for the window's
edges, whatever the order of the chunks and with each chunk alone; the default engine still writes the frames of
zstd_enc_v1.json; and the blobs of pbsgpu_blob_encode2_device come back through the device's decoder to chunks with the
SHA-256 of what went in."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_upload_new2 as U  # noqa: E402
import test_gpu_zstd_encode_tables as T  # noqa: E402
import zstd_enc_window_inputs as wi  # noqa: E402

zi = wi.zi
pytestmark = pytest.mark.gpu
OK = 0


@pytest.fixture(scope="module")
def world(gpu_lib):
    """({mode: engine}, default engine, [(name, content)] of the subset, device buffer of the contents 0-6 bytes apart,
    their ranges)"""
    from pbs_plus_amd import Engine, buzhash

    engines = {m: Engine(buzhash.NewConfig(4096), device=0, inflight=1, zstd_window_log=m[0], zstd_seq_tables=m[1])
               for m in wi.WINDOW_MODES}
    eng0 = Engine(buzhash.NewConfig(4096), device=0)
    cases = [(name, wi.content_of(name)) for name in wi.GPU_SUBSET]
    rng = np.random.default_rng(10)
    parts, ranges, pos = [], [], 0
    for _, data in cases:
        gap = int(rng.integers(0, 7))
        parts.append(bytes(gap) + data)
        ranges.append((pos + gap, len(data)))
        pos += gap + len(data)
    host = np.frombuffer(b"".join(parts), np.uint8)
    dev = eng0.alloc(host.size)
    dev.upload(host)
    yield engines, eng0, cases, dev, np.array(ranges, dtype=np.uint64)
    dev.free()
    eng0.close()
    for e in engines.values():
        e.close()


def _frames(eng, dev, ranges, cases, order):
    """one call over the chunks in `order`, rooms of the bound between guards (T._encode checks them): {case index: frame}"""
    status, flen, rooms, dst, _ = T._encode(eng, dev, ranges[order], [zi.bound(len(cases[i][1])) for i in order])
    dst.free()
    assert np.all(status == OK), [cases[order[k]][0] for k in np.flatnonzero(status != OK)]
    return {int(i): rooms[k][:int(flen[k])].tobytes() for k, i in enumerate(order)}


@pytest.mark.parametrize("mode", wi.WINDOW_MODES, ids=[wi.KEY[m] for m in wi.WINDOW_MODES])
def test_golden_frames_in_any_order_and_alone(world, mode):
    engines, _, cases, dev, ranges = world
    eng, golden, n = engines[mode], wi.golden(), len(cases)
    first = _frames(eng, dev, ranges, cases, np.arange(n))
    for i, (name, data) in enumerate(cases):
        assert 0 < len(first[i]) <= zi.bound(len(data)), name
        assert [len(first[i]), hashlib.sha256(first[i]).hexdigest()] == golden[name][wi.KEY[mode]], name
    perm = np.random.default_rng(3).permutation(n)
    assert _frames(eng, dev, ranges, cases, perm) == first
    for i in range(n):
        assert _frames(eng, dev, ranges, cases, np.array([i])) == {i: first[i]}, cases[i][0]


def test_a_default_engine_beside_them_writes_the_frames_it_always_wrote(world):
    engines, eng0, cases, dev, ranges = world
    golden = zi.golden()
    pick = np.array([i for i, (name, _) in enumerate(cases) if name in golden])
    assert pick.size >= 4
    frames = _frames(eng0, dev, ranges, cases, pick)
    for i in pick:
        assert [len(frames[i]), hashlib.sha256(frames[i]).hexdigest()] == golden[cases[i][0]], cases[i][0]
    # and the option is what made the others: the far repeats cost the default engine more bytes
    i = [c[0] for c in cases].index("period70000-300000")
    assert 2 * wi.golden()["period70000-300000"]["w17-t0"][0] < len(frames[i])


@pytest.mark.parametrize("mode", wi.WINDOW_MODES, ids=[wi.KEY[m] for m in wi.WINDOW_MODES])
def test_blobs_come_back_through_the_device_decoder(world, mode):
    """blob_encode2(zstd) on the window engine: a compressed blob's frame is zstd_encode's of the same bytes on the same
    engine and strictly shorter than the chunk, and blob_decode2 gives chunks with the SHA-256 of the contents"""
    engines, _, cases, dev, ranges = world
    eng, golden = engines[mode], wi.golden()
    datas = [d for _, d in cases]
    dst, offs, lens, kinds, crcs, est = eng.blob_encode2(dev, ranges, zstd=True)
    try:
        out = dst.download(0, int(offs[-1]))
        for k, (name, data) in enumerate(cases):
            wins = golden[name][wi.KEY[mode]][0] < len(data)  # "compressed only if strictly shorter than the chunk"
            assert (int(kinds[k]), int(lens[k])) == (int(wins), 12 + (golden[name][wi.KEY[mode]][0] if wins else len(data))), name
        assert est["blobs"][1] >= len(cases) - 2
        digests = np.stack([np.frombuffer(hashlib.sha256(d).digest(), np.uint8) for d in datas])
        U._check_blobs(eng, dst, out, offs[:-1], lens, kinds, crcs, datas, digests)
    finally:
        dst.free()
