"""Keyed chunk digests on the device, SHA-256(content || id_key): the whole-range hash with a key
(pbsgpu_sha256_keyed_many_*) and the batch path with every record's digest keyed (pbsgpu_submit_*_keyed), on each form of the
SHA-256 kernels (pairs, single wave, express) and in the dense and the sparse selection. Every expectation is exact:
hashlib.sha256(content + id_key). The references are computed once per module."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu

KEY_A = bytes((7 * i + 3) & 0xFF for i in range(32))
KEY_B = bytes((11 * i + 5) & 0xFF for i in range(32))
MIB = 1 << 20


@pytest.fixture(scope="module")
def ranges():
    """(the 6 MB buffer, the segments, {key: the keyed digests of the checked segments}, the checked indices)"""
    from oracle import oracle as O

    blob = O.fill(6_000_000, 22, 0)
    segs = [(a, l) for a in range(4) for l in range(131)]
    # long and short chunks at odd offsets; 1 MiB + 23 and + 24: both parities of the tail block on a long chunk
    at = 1
    for l in (0, 1, 3, 4095, 65535, 65536, 65537, MIB + 23, MIB + 24):
        segs.append((at, l))
        at += l + 2 - (l & 1)  # stays odd
    assert at < 6_000_000 and all(o & 1 for o, _ in segs[4 * 131:])
    special = len(segs)
    rng = np.random.default_rng(3)
    segs += [(int(o), int(l)) for o, l in zip(rng.integers(0, 5_000_000, 30000), rng.integers(0, 200, 30000))]
    checked = list(range(special)) + list(range(special, len(segs), 97))
    raw = blob.tobytes()
    want = {k: {i: hashlib.sha256(raw[segs[i][0]:segs[i][0] + segs[i][1]] + k).digest() for i in checked} for k in (KEY_A, KEY_B, b"")}
    return blob, segs, want, checked


@pytest.mark.parametrize("dense_pct", [1, 0xFFFFFFFF])
@pytest.mark.parametrize("form", [0, 1, 2])
def test_keyed_many_equals_hashlib_on_every_form(ranges, form, dense_pct):
    from pbs_plus_amd import Engine, IdKey, buzhash

    blob, segs, want, checked = ranges
    with Engine(buzhash.NewConfig(4096), sha_form=form, sha_dense_pct=dense_pct) as eng:
        buf = eng.alloc(blob.size + 16)
        ka, kb = IdKey(eng, KEY_A), IdKey(eng, KEY_B)
        try:
            buf.upload(blob)
            for key, raw in ((ka, KEY_A), (kb, KEY_B)):
                dig = eng.sha256_keyed_many(key, buf, segs, nbytes=blob.size)
                assert dig.shape == (len(segs), 32)
                bad = [(i, segs[i]) for i in checked if bytes(dig[i]) != want[raw][i]]
                assert not bad, (form, dense_pct, bad[:8])
            # the host entry point, and the plain call over the same segments: unchanged
            host = eng.sha256_keyed_many(ka, blob, segs[:4 * 131 + 9])
            assert all(bytes(host[i]) == want[KEY_A][i] for i in range(4 * 131 + 9))
            plain = eng.sha256_many(buf, segs, nbytes=blob.size)
            bad = [(i, segs[i]) for i in checked if bytes(plain[i]) != want[b""][i]]
            assert not bad, (form, dense_pct, bad[:8])
        finally:
            ka.close()
            kb.close()
            buf.free()
    # two keys, two digests; and neither is the plain one (the empty range included: the digest of the key alone)
    for i in checked[:4 * 131 + 9]:
        assert len({want[KEY_A][i], want[KEY_B][i], want[b""][i]}) == 3, i


def test_a_key_of_another_engine_is_refused():
    from pbs_plus_amd import Engine, IdKey, PbsGpuError, _lib, buzhash

    with Engine(buzhash.NewConfig(4096)) as eng, Engine(buzhash.NewConfig(4096)) as other:
        with IdKey(other, KEY_A) as foreign, IdKey(eng, KEY_A) as own:
            data = np.arange(100000, dtype=np.uint32).view(np.uint8)
            with pytest.raises(PbsGpuError) as ei:
                eng.sha256_keyed_many(foreign, data, [(0, 100)])
            assert ei.value.status == _lib.E_INVALID
            with pytest.raises(PbsGpuError) as ei:
                eng.submit(data, id_key=foreign)
            assert ei.value.status == _lib.E_INVALID
            assert bytes(eng.sha256_keyed_many(own, data, [(0, 100)])[0]) == hashlib.sha256(data[:100].tobytes() + KEY_A).digest()
        with pytest.raises(ValueError):
            IdKey(eng, KEY_A[:31])
        with IdKey(eng, KEY_A) as k:
            assert repr(k) == "IdKey(<32 bytes>)"  # (never the key)


CASES = ((4096, 3_000_001, 3), (4 << 20, 80 << 20, 0))


@pytest.fixture(scope="module")
def streams():
    """per case: (data, the oracle's records, the keyed digest of every oracle chunk)"""
    from oracle import oracle as O

    out = {}
    for avg, n, kind in CASES:
        data = O.fill(n, 21, kind)
        recs = O.chunk_and_digest(O.new_config(avg), data)
        raw = data.tobytes()
        keyed = [hashlib.sha256(raw[int(r["end"]) - int(r["size"]):int(r["end"])] + KEY_A).digest() for r in recs]
        out[avg] = (data, recs, keyed)
    return out


def same_cuts(got, want):
    return len(got) == len(want) and all(np.array_equal(got[f], want[f]) for f in ("end", "size", "segment"))


@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("avg", [c[0] for c in CASES])
def test_the_batch_path_with_a_key(streams, avg, form):
    from pbs_plus_amd import Engine, IdKey, buzhash

    data, want, keyed = streams[avg]
    with Engine(buzhash.NewConfig(avg), sha_form=form) as eng, IdKey(eng, KEY_A) as key:
        got = eng.chunk_and_digest(data, id_key=key)
        assert same_cuts(got, want), (len(got), len(want))
        bad = [i for i in range(len(got)) if bytes(got["digest"][i]) != keyed[i]]
        assert not bad, (avg, form, bad[:8])
        if avg != 4096:
            return
        # a plain and a keyed ticket in flight together on one engine: each gets its own digests
        tk, tp = eng.submit(data, id_key=key), eng.submit(data)
        plain, again = eng.collect(tp), eng.collect(tk)
        assert same_cuts(plain, want) and np.array_equal(plain["digest"], want["digest"])
        assert same_cuts(again, want) and all(bytes(again["digest"][i]) == keyed[i] for i in range(len(again)))


def test_the_batch_path_with_a_key_and_segments(streams):
    from oracle import oracle as O
    from pbs_plus_amd import Engine, IdKey, buzhash

    data = streams[4096][0]
    segs = [(0, 700_001), (700_004, 1_299_996), (2_000_003, 999_998)]
    want = O.chunk_and_digest(O.new_config(4096), data, segs)
    raw = data.tobytes()
    with Engine(buzhash.NewConfig(4096)) as eng, IdKey(eng, KEY_A) as key:
        buf = eng.alloc(data.size + 16)
        try:
            buf.upload(data)
            got = eng.chunk_and_digest(buf, segments=segs, nbytes=data.size, id_key=key)
        finally:
            buf.free()
    assert same_cuts(got, want), (len(got), len(want))
    for r in got:
        lo = segs[int(r["segment"])][0] + int(r["end"]) - int(r["size"])
        assert bytes(r["digest"]) == hashlib.sha256(raw[lo:lo + int(r["size"])] + KEY_A).digest(), r
