"""The device-resident known-chunk set (pbsgpu_known_*, KnownChunks) on the GPU, bit-exact against a sequential Python
`set` model: the PBS client's known_chunks rule — upload the first occurrence of a digest the server lacks, reference
every later one."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from known_inputs import records as _recs, set_model as _model  # noqa: E402

pytestmark = pytest.mark.gpu


def _engine(avg=4096):
    from pbs_plus_amd import Engine, buzhash

    return Engine(buzhash.NewConfig(avg), device=0)


def _digest_set(recs):
    return {d.tobytes() for d in recs["digest"]}


def _rand(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def test_model_parity_on_a_mixed_batch():
    from pbs_plus_amd import KnownChunks

    rng = np.random.default_rng(11)
    eng = _engine()
    base = _recs(_rand(rng, 200_000), seed=1)
    k = KnownChunks(eng)
    k.add(base)
    assert len(k) == 200_000
    n = 300_000
    fresh = _rand(rng, 150_000)
    parts = [base["digest"][rng.integers(0, base.size, 90_000)],          # ~30 % from the set
             fresh[rng.integers(0, fresh.shape[0], 60_000)],              # ~20 % repeated within the batch
             fresh]                                                        # fresh (first occurrences among them)
    dig = np.concatenate(parts)[rng.permutation(n)]
    batch = _recs(dig, seed=2)
    want, wst, after = _model(_digest_set(base), batch)
    got, st = k.classify(batch, insert=True)
    assert np.array_equal(got, want)
    assert st == wst, (st, wst)
    assert 0.3 < wst["nunique"] / n < 0.6
    assert len(k) == len(after)
    k.close()
    eng.close()


def test_insert_0_leaves_the_set_unchanged():
    from pbs_plus_amd import KnownChunks

    rng = np.random.default_rng(12)
    eng = _engine()
    base = _recs(_rand(rng, 50_000))
    k = KnownChunks(eng, capacity=1000)
    k.add(base)
    dig = np.concatenate([base["digest"][:20_000], _rand(rng, 30_000)])
    dig = np.concatenate([dig, dig[::7]])
    batch = _recs(dig[rng.permutation(dig.shape[0])])
    want, wst, _ = _model(_digest_set(base), batch, insert=False)
    f1, s1 = k.classify(batch, insert=False)
    assert len(k) == 50_000
    f2, s2 = k.classify(batch, insert=False)
    assert len(k) == 50_000
    assert np.array_equal(f1, want) and np.array_equal(f2, want) and s1 == wst and s2 == wst
    # stats only (no flags) through the same path
    none, s3 = k.classify(batch, insert=False, want_flags=False)
    assert none is None and s3 == wst
    k.close()
    eng.close()


def _crafted(rng):
    fams = []
    a = _rand(rng, 512)
    a[:, :8] = rng.integers(0, 256, 8, dtype=np.uint8)            # 512 sharing bytes 0..7
    fams.append(a)
    b = _rand(rng, 512)
    b[:, :16] = rng.integers(0, 256, 16, dtype=np.uint8)          # 512 sharing bytes 0..15
    fams.append(b)
    p = _rand(rng, 64)
    q = p.copy()
    q[:, 31] ^= rng.integers(1, 256, 64, dtype=np.uint8)          # pairs differing only in byte 31
    fams.append(np.concatenate([p, q]))
    z = np.zeros((2, 32), dtype=np.uint8)
    z[1] = 0xFF                                                    # all-zero, all-0xFF
    fams.append(z)
    t = np.zeros((3, 32), dtype=np.uint8)
    t[0, 0] = 1                                                    # tag collides with the zero digest's (0 -> 1)
    t[1, 31] = 1
    t[2, 8:16] = 0xFF
    fams.append(t)
    return np.concatenate(fams)


def test_crafted_digests_as_set_content_and_as_queries():
    from pbs_plus_amd import KnownChunks

    rng = np.random.default_rng(13)
    eng = _engine()
    crafted = _crafted(rng)
    m = crafted.shape[0]
    for trial in range(3):
        perm = rng.permutation(m)
        content = crafted[perm[: m // 2]] if trial < 2 else crafted[:0]
        k = KnownChunks(eng, capacity=16)
        if content.shape[0]:
            k.add(_recs(content))
        # queries: everything, some of it twice, in a shuffled order
        q = np.concatenate([crafted, crafted[rng.integers(0, m, m // 3)]])
        batch = _recs(q[rng.permutation(q.shape[0])])
        init = _digest_set(_recs(content)) if content.shape[0] else set()
        for insert in (False, True):
            want, wst, after = _model(init, batch, insert=insert)
            got, st = k.classify(batch, insert=insert)
            assert np.array_equal(got, want), (trial, insert)
            assert st == wst
            assert len(k) == len(after)
        # after the insert everything is known
        got, st = k.classify(_recs(crafted), insert=False)
        assert got.all() and st["nunique"] == 0
        k.close()
    eng.close()


def test_growth_from_a_small_table():
    from pbs_plus_amd import KnownChunks

    rng = np.random.default_rng(14)
    eng = _engine()
    k = KnownChunks(eng, capacity=1024)
    sizes = [1, 7, 4096, 1 << 20] * 3
    batches = [_rand(rng, s) for s in sizes]
    total = 0
    for b in batches:
        k.add(_recs(b))
        total += b.shape[0]
        assert len(k) == total
    alld = np.concatenate(batches)
    assert np.unique(alld, axis=0).shape[0] == total                 # (random 32-byte digests: no accidental repeats)
    k.add(_recs(alld[::5]))                                           # idempotent
    assert len(k) == total
    got, st = k.classify(_recs(alld), insert=False)
    assert got.all() and st["nunique"] == 0 and st["nrecords"] == total
    fresh = _rand(rng, 100_000)
    got, st = k.classify(_recs(fresh), insert=False)
    assert not got.any() and st["nunique"] == 100_000
    assert len(k) == total
    k.close()
    eng.close()


def test_host_and_device_variants_agree():
    from pbs_plus_amd import KnownChunks

    rng = np.random.default_rng(15)
    eng = _engine()
    base = _recs(_rand(rng, 40_000))
    dig = np.concatenate([base["digest"][:15_000], _rand(rng, 25_000)])
    dig = np.concatenate([dig, dig[::3]])
    batch = _recs(dig[rng.permutation(dig.shape[0])])
    buf = eng.alloc(batch.nbytes)
    buf.upload(batch.view(np.uint8))
    kh, kd = KnownChunks(eng), KnownChunks(eng)
    kh.add(base)
    bb = eng.alloc(base.nbytes)
    bb.upload(base.view(np.uint8))
    kd.add_device(bb.ptr, base.size)
    assert len(kh) == len(kd) == base.size
    want, wst, after = _model(_digest_set(base), batch)
    for insert in (False, True, False):
        before = len(kh)
        fh, sh = kh.classify(batch, insert=insert)
        fd, sd = kd.classify_device(buf.ptr, batch.size, insert=insert)
        assert np.array_equal(fh, fd) and sh == sd
        assert len(kh) == len(kd)
        if before == base.size:
            assert np.array_equal(fh, want) and sh == wst
        else:                                        # after the insert: everything is known
            assert fh.all()
    assert len(kh) == len(after)
    buf.free()
    bb.free()
    kh.close()
    kd.close()
    eng.close()


def test_batch_dedup_is_classify_against_an_empty_set():
    """Engine.dedup / dedup_device (pbsgpu_dedup_*) give the flags and stats of classify(insert=False) on a fresh set,
    and of the sequential model."""
    from pbs_plus_amd import KnownChunks

    rng = np.random.default_rng(17)
    eng = _engine()
    pre = _rand(rng, 40)
    pre[:, :8] = pre[0, :8]                                        # 40 records sharing one 8-byte prefix ...
    pre[[9, 17, 33]] = pre[[2, 5, 2]]                              # ... with repeated digests among them
    n = 1 << 20
    root = np.arange(n)
    rep = rng.random(n) < 0.4                                      # ~40 % repeat a random earlier record
    rep[0] = False
    root[rep] = (rng.random(n) * np.arange(n)).astype(np.int64)[rep]
    while not np.array_equal(root[root], root):
        root = root[root]
    k = KnownChunks(eng)
    for batch in (_recs(_rand(rng, 0)), _recs(_rand(rng, 1)), _recs(pre), _recs(_rand(rng, n)[root], seed=3)):
        want, wst, _ = _model(set(), batch, insert=False)
        dup, st = eng.dedup(batch)
        assert np.array_equal(dup, want) and st == wst, batch.size
        buf = eng.alloc(batch.nbytes) if batch.size else None
        if buf:
            buf.upload(batch.view(np.uint8))
        dptr = buf.ptr if buf else 0
        dup_d, st_d = eng.dedup_device(dptr, batch.size)
        assert np.array_equal(dup_d, want) and st_d == wst, batch.size
        none, st_n = eng.dedup_device(dptr, batch.size, want_flags=False)
        assert none is None and st_n == wst
        kf, kst = k.classify(batch, insert=False)
        assert np.array_equal(kf, want) and kst == wst, batch.size
        if buf:
            kf, kst = k.classify_device(buf.ptr, batch.size, insert=False)
            assert np.array_equal(kf, want) and kst == wst, batch.size
            buf.free()
        if batch.size == 40:
            assert wst["nunique"] == 37
        if batch.size == n:
            assert 0.35 < 1 - wst["nunique"] / n < 0.45, wst
    assert len(k) == 0
    k.close()
    eng.close()


def test_add_didx_loads_an_index_and_rejects_bad_images():
    from pbs_plus_amd import KnownChunks, PbsGpuError

    rng = np.random.default_rng(16)
    eng = _engine()
    recs = _recs(_rand(rng, 5000))
    blob = eng.didx_encode(recs)
    k = KnownChunks(eng)
    k.add_didx(blob)
    assert len(k) == 5000
    got, _ = k.classify(recs, insert=False)
    assert got.all()
    for bad in (b"\0" * 8 + blob[8:], blob[:-3], blob[:100]):
        with pytest.raises(PbsGpuError) as ei:
            k.add_didx(bad)
        assert ei.value.status == -1
    assert len(k) == 5000
    k.add_didx(blob[:4096])                                      # an empty index
    assert len(k) == 5000
    k.close()
    eng.close()


def _ring_ingest(ring, rows, nbytes, on_batch=None, timeout_s=240.0):
    """Feed one piece-table stream through the ring; on_batch(records) is called for every polled batch."""
    sid = ring.open()
    left, first, got, fin = nbytes, True, [], False
    quota = 16 * ring.page_bytes
    t0 = time.time()
    while not fin:
        assert time.time() - t0 < timeout_s, ring.stats()
        if left:
            want = min(left, quota)
            left -= ring.fill_pieces(sid, np.array(rows, dtype=np.uint64) if first else None, want, final=(want == left))
            first = False
        ring.pump()
        recs, fin = ring.poll(sid, cap=1 << 15)
        if recs.size:
            recs = recs.copy()
            got.append(recs)
            if on_batch is not None:
                on_batch(recs)
    ring.close_stream(sid)
    return np.concatenate(got)


def test_incremental_backup_through_the_ring():
    """The scenario the set exists for: a base stream's index is loaded from its .didx, an edited stream is chunked through
    the page ring, and every polled batch is classified WHILE the ring's service runs — exact against the model, most
    bytes known, and no call waits for the service to go idle."""
    from pbs_plus_amd import KnownChunks, PageRing

    eng = _engine(64 << 10)
    page = 262144
    ring = PageRing(eng, arena_bytes=64 * (page + 256), page_bytes=page, max_streams=2, sha_cus=16, round_pages=8)
    n = 256 << 20
    seed_base, seed_new = 4242, 99
    base = _ring_ingest(ring, [(0, n, 0, seed_base)], n)
    assert base.size > 2000 and int(base["end"][-1]) == n
    k = KnownChunks(eng)
    k.add_didx(eng.didx_encode(base))
    base_set = _digest_set(base)
    assert len(k) == len(base_set)
    # the edited stream: the base with 8 rewritten extents (offsets and lengths multiples of 16)
    rng = np.random.default_rng(17)
    cuts = sorted(int(x) * 16 for x in rng.choice(n // 16 - 4096, 8, replace=False))
    rows, pos, npos = [], 0, 0
    for c in cuts:
        if c < pos:
            continue
        ln = int(rng.integers(1, 256)) * 16
        rows.append((pos, c - pos, pos, seed_base))
        rows.append((c, ln, npos, seed_new))
        npos += ln
        pos = c + ln
    rows.append((pos, n - pos, pos, seed_base))
    rows = [r for r in rows if r[1] > 0]
    flags, times, batches = [], [], []

    def classify(recs):
        t0 = time.perf_counter()
        f, st = k.classify(recs, insert=True)
        times.append(time.perf_counter() - t0)
        assert st["nrecords"] == recs.size
        flags.append(f)
        batches.append(recs)

    edited = _ring_ingest(ring, rows, n, on_batch=classify)
    assert ring.stats()["service_launches"] >= 1
    ring.quiesce()
    got = np.concatenate(flags)
    want, wst, after = _model(base_set, edited)
    assert np.array_equal(got, want)
    sizes = edited["size"].astype(np.uint64)
    assert sizes[got == 1].sum() >= 0.95 * n, (int(sizes[got == 1].sum()), n)
    assert len(k) == len(after)
    assert max(times) < 1.0, times
    assert len(times) >= 2
    ring.close()
    k.close()
    eng.close()


def test_lifetime_two_sets_and_a_closed_engine():
    from pbs_plus_amd import KnownChunks

    rng = np.random.default_rng(18)
    eng = _engine()
    a, b = _recs(_rand(rng, 1000)), _recs(_rand(rng, 1000))
    ka, kb = KnownChunks(eng), KnownChunks(eng)
    ka.add(a)
    kb.add(b)
    fa, _ = ka.classify(b, insert=False)
    fb, _ = kb.classify(a, insert=False)
    assert not fa.any() and not fb.any() and len(ka) == len(kb) == 1000
    eng.close()                                   # the sets keep the engine alive
    f, st = ka.classify(np.concatenate([a, b]), insert=True)
    assert f[:1000].all() and not f[1000:].any() and st["nunique"] == 1000
    assert len(ka) == 2000 and len(kb) == 1000
    ka.close()
    f, _ = kb.classify(b, insert=False)
    assert f.all()
    kb.close()
