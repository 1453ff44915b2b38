"""The known-chunk set (pbs_plus_amd/csrc/known.hip) on digests crafted to collide: one home slot (a long probe chain, its
wrap from the last slot to slot 0, hundreds of threads of one launch claiming slots of one chain, the rehash of such a
chain), one sort key (runs of several distinct digests with their repeats interleaved, at both ends of the sorted array
and across 256-thread blocks), equal tag AND home AND key (the 32-byte compare decides alone), the exact load boundary,
and the fused classify-and-frame call on such input.

Every flag, every stats field and every len() is exact against the sequential `set` rule (known_inputs.set_model).
tests/known_inputs.py builds the inputs by inverting the set's hash; tests/test_known_inputs.py proves without a GPU, on
the C++ hash and on a model of the table, that each scenario reaches the path named here."""
import ctypes as C
import hashlib
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import known_inputs as K  # noqa: E402
from known_inputs import digest_set, records, set_model  # noqa: E402

pytestmark = pytest.mark.gpu
MAGIC = hashlib.sha256(b"Proxmox Backup uncompressed blob v1.0").digest()[:8]


@pytest.fixture
def eng(gpu_lib):
    from pbs_plus_amd import Engine, buzhash

    e = Engine(buzhash.NewConfig(4096), device=0)
    yield e
    e.close()


def _small_set(eng, content=None):
    """KnownChunks(capacity=16): a table of 1 024 slots"""
    from pbs_plus_amd import KnownChunks

    k = KnownChunks(eng, capacity=16)
    if content is not None and content.shape[0]:
        k.add(records(content))
    return k


def _classify(k, have, digests, insert, what=""):
    """classify on the host path, exact against the model started from `have`; returns (flags, the set afterwards)"""
    recs = records(digests)
    want, wst, after = set_model(have, recs, insert=insert)
    got, st = k.classify(recs, insert=insert)
    assert np.array_equal(got, want), (what, int((got != want).sum()), np.nonzero(got != want)[0][:8])
    assert st == wst, (what, st, wst)
    assert len(k) == len(after), (what, len(k), len(after))
    return got, after


@pytest.mark.parametrize("H", [K.HOME_LAST, K.HOME_FIRST, K.HOME_MID], ids=["last", "first", "mid"])
def test_one_home_a_wrapped_chain_and_its_growth(eng, H):
    """a. 400 threads of one add claim slots of one chain; absent queries walk all 400 slots (for HOME_LAST: across the
    table's end); the next 400 grow the table inside classify and the chain is rehashed; a set filled one record per call
    answers the same."""
    sc = K.scenario_one_home(H)
    a, b, c = sc["a"], sc["b"], sc["c"]
    k = _small_set(eng)
    k.add(records(a))
    assert len(k) == 400
    have = digest_set(a)
    f_ab, have = _classify(k, have, sc["q_ab"], False, "a and b against a")
    f_b, have = _classify(k, have, b, True, "b inserted: growth")
    assert not f_b.any() and len(k) == 800
    f_all, have = _classify(k, have, sc["q_all"], False, "all against a and b")
    in_c = np.array([bytes(d) not in have for d in sc["q_all"]])
    assert f_all[~in_c].all() and int((f_all[in_c] == 0).sum()) == 400      # c: new in its first occurrences only
    # the same content, the first 40 one record per call: the answers do not depend on the order of insertion
    k2 = _small_set(eng)
    for i in range(40):
        k2.add(records(a[i:i + 1]))
        assert len(k2) == i + 1
    k2.add(records(a[40:]))
    assert len(k2) == 400
    g_ab, _ = _classify(k2, digest_set(a), sc["q_ab"], False, "second set: a and b against a")
    assert np.array_equal(g_ab, f_ab)
    g_b, have2 = _classify(k2, digest_set(a), b, True, "second set: b inserted")
    g_all, _ = _classify(k2, have2, sc["q_all"], False, "second set: all")
    assert np.array_equal(g_all, f_all)
    # ... and c goes in as well (a second growth, of an 800-long chain), after which everything is known
    _, have = _classify(k, have, sc["q_all"], True, "c inserted: second growth")
    assert len(k) == 1200
    f, _ = _classify(k, have, sc["q_all"], False, "everything known")
    assert f.all()
    k.close()
    k2.close()


@pytest.mark.parametrize("shuffle_seed", [0, 1, 2])
def test_one_sort_key_first_occurrence_rule(eng, shuffle_seed):
    """b. Runs of about a thousand records under one sort key (0, 0xFFFFFFFF and one in between), 400 distinct digests
    each, repeats interleaved: through the batch dedup, classify on both paths, and add_didx (stride 40)."""
    sc = K.scenario_one_key(shuffle_seed=shuffle_seed)
    recs = records(sc["batch"], seed=shuffle_seed)
    # the batch dedup: nothing known beforehand
    want, wst, _ = set_model(set(), recs, insert=False)
    dup, st = eng.dedup(recs)
    assert np.array_equal(dup, want) and st == wst
    buf = eng.alloc(recs.nbytes)
    buf.upload(recs.view(np.uint8))
    dup_d, st_d = eng.dedup_device(buf.ptr, recs.size)
    assert np.array_equal(dup_d, want) and st_d == wst
    # classify, host and device records, on sets preloaded with every third distinct digest
    pre = digest_set(sc["preload"])
    kh, kd = _small_set(eng, sc["preload"]), _small_set(eng, sc["preload"])
    assert len(kh) == len(kd) == len(pre) == 567
    have = pre
    for insert in (False, True):
        want, wst, after = set_model(have, recs, insert=insert)
        fh, sh = kh.classify(recs, insert=insert)
        fd, sd = kd.classify_device(buf.ptr, recs.size, insert=insert)
        assert np.array_equal(fh, want) and sh == wst, insert
        assert np.array_equal(fd, want) and sd == wst, insert
        assert len(kh) == len(kd) == len(after), insert
        have = after
    assert len(kh) == 1700
    f, st = kh.classify(recs, insert=False)
    assert f.all() and st["nunique"] == 0
    # a .didx image of the same records: the 40-byte entries go through the same lookup, sort, mark and insert
    kx = _small_set(eng)
    kx.add_didx(eng.didx_encode(recs))
    assert len(kx) == 1700
    f, _ = kx.classify(records(sc["distinct"]), insert=False)
    assert f.all()
    f, st = kx.classify(records(K.random_digests(np.random.default_rng(9), 64)), insert=False)
    assert not f.any() and st["nunique"] == 64
    buf.free()
    for k in (kh, kd, kx):
        k.close()


def test_equal_tag_home_and_key(eng):
    """c. Digests that agree in tag, home slot and sort key and differ only in bytes 8..31 (a quarter of them only in bytes
    16..31), and the w0 = 0 / w0 = 1 families of one home that share the stored tag 1: half of them in the set, all of them
    queried, some twice."""
    sc = K.scenario_equal_tag_home_key()
    k = _small_set(eng, sc["content"])
    have = digest_set(sc["content"])
    assert len(k) == 350
    for insert in (False, True):
        _, have = _classify(k, have, sc["queries"], insert, insert)
    assert len(k) == 700
    f, _ = _classify(k, have, sc["all"], False, "afterwards")
    assert f.all()
    k.close()


def test_load_boundary_on_one_chain(eng):
    """d. 511 digests of the last slot's home, then the 512th (count == slots / 2: the table stays), an absent digest of
    that home (a walk over 512 occupied slots to the one empty slot behind them), then the 513th (the table grows)."""
    sc = K.scenario_load_boundary()
    absent = sc["absent"]
    k = _small_set(eng)
    k.add(records(sc["first"]))
    have = digest_set(sc["first"])
    inserted = sc["first"]

    def check(step):
        assert len(k) == len(have), step
        f, _ = _classify(k, have, np.concatenate([inserted, absent]), False, step)
        assert f[:-1].all() and f[-1] == 0, step

    check("511")
    f, have = _classify(k, have, sc["d512"], True, "the 512th")
    assert f[0] == 0 and len(k) == 512
    inserted = np.concatenate([inserted, sc["d512"]])
    check("512")
    f, _ = _classify(k, have, absent, False, "absent at the boundary")
    assert f[0] == 0
    f, have = _classify(k, have, sc["d513"], True, "the 513th")
    assert f[0] == 0 and len(k) == 513
    inserted = np.concatenate([inserted, sc["d513"]])
    check("513")
    k.close()


def _fused_raw(k, src, recs, chunks, insert, dptr, cap):
    """pbsgpu_known_upload_new_device with its outputs pre-set: (status, flags, offsets, crcs, used, stats)"""
    from pbs_plus_amd import _lib

    n = int(recs.size)
    segs = np.ascontiguousarray(chunks, dtype=np.uint64).reshape(-1, 2)
    flags = np.full(n, 9, dtype=np.uint8)
    offs = np.full(n, 7, dtype=np.uint64)
    crcs = np.full(n, 9, dtype=np.uint32)
    used, st = C.c_uint64(123), _lib.DedupStats()
    rc = k._L.pbsgpu_known_upload_new_device(k._h, src.ptr, src.nbytes, recs.ctypes.data, segs.ctypes.data, n, int(insert),
                                             dptr, cap, flags.ctypes.data, offs.ctypes.data, crcs.ctypes.data,
                                             C.byref(used), C.byref(st))
    return rc, flags, offs, crcs, int(used.value), {f: int(getattr(st, f)) for f, _ in _lib.DedupStats._fields_}


def test_fused_call_on_crafted_digests(eng):
    """e. KnownChunks.upload_new on 1 500 records whose digests are two one-home one-key families with repeats (a third
    preloaded), over random 0 to 3 000-byte ranges of a 1 MiB buffer: flags, stats and len() against the model; offsets,
    CRCs and blob bytes against zlib and against classify + Engine.blob_encode on a twin; then E_CAPACITY one byte short."""
    from pbs_plus_amd import _lib

    sc = K.scenario_fused()
    chunks, n = sc["chunks"], sc["batch"].shape[0]
    host = np.random.default_rng(sc["data_seed"]).integers(0, 256, sc["nbytes"], dtype=np.uint8)
    src = eng.alloc(sc["nbytes"])
    src.upload(host)
    recs = records(sc["batch"], sizes=chunks[:, 1].astype(np.uint32))
    pre = digest_set(sc["preload"])
    want, wst, after = set_model(pre, recs, insert=True)
    new = want == 0
    assert int(new.sum()) == 500
    # the model blob
    blob, want_offs, want_crcs = bytearray(), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    for i in np.nonzero(new)[0]:
        o, m = int(chunks[i, 0]), int(chunks[i, 1])
        data = host[o:o + m].tobytes()
        want_offs[i], want_crcs[i] = len(blob), zlib.crc32(data)
        blob += MAGIC + zlib.crc32(data).to_bytes(4, "little") + data
    needed = len(blob)
    assert needed == int(chunks[new, 1].sum()) + 12 * 500
    fused, twin, short = (_small_set(eng, sc["preload"]) for _ in range(3))
    # insert = False first: the same flags, the set as it was
    w0, wst0, _ = set_model(pre, recs, insert=False)
    dst, flags, offs, crcs, st = fused.upload_new(src, recs, chunks, insert=False)
    assert np.array_equal(flags, w0) and st == wst0 and len(fused) == 250 and dst.used == needed
    assert dst.download(0, needed).tobytes() == bytes(blob)
    dst.free()
    dst, flags, offs, crcs, st = fused.upload_new(src, recs, chunks, insert=True)
    assert np.array_equal(flags, want) and st == wst, int((flags != want).sum())
    assert len(fused) == len(after) == 750
    assert dst.used == needed
    assert np.array_equal(offs[new], want_offs[new]) and np.array_equal(crcs[new], want_crcs[new])
    assert not offs[~new].any() and not crcs[~new].any()
    out = dst.download(0, needed).tobytes()
    assert out == bytes(blob)
    # the two-call path on the twin
    f2, st2 = twin.classify(recs, insert=True)
    dst2, offs2, crcs2 = eng.blob_encode(src, chunks[f2 == 0])
    assert np.array_equal(f2, flags) and st2 == st and len(twin) == len(fused)
    assert int(offs2[-1]) == needed and np.array_equal(offs2[:-1], offs[new]) and np.array_equal(crcs2, crcs[new])
    assert dst2.download(0, needed).tobytes() == out
    dst.free()
    dst2.free()
    f, st = fused.classify(recs, insert=False)
    assert f.all() and st["nunique"] == 0
    # one byte short on a fresh twin: E_CAPACITY, the size needed, valid flags and stats, nothing inserted
    before, _ = short.classify(recs, insert=False)
    assert np.array_equal(before, w0)
    g = eng.alloc(needed + 128)
    g.upload(np.full(needed + 128, 0xA5, dtype=np.uint8))
    rc, flags, offs, crcs, used, st = _fused_raw(short, src, recs, chunks, True, g.ptr + 64, needed - 1)
    assert rc == _lib.E_CAPACITY and used == needed
    assert len(short) == 250
    assert np.array_equal(flags, w0) and st == wst0
    assert np.all(offs == 7) and np.all(crcs == 9)
    assert np.all(g.download() == 0xA5)
    again, st_again = short.classify(recs, insert=False)              # (the table may have grown; its content has not changed)
    assert np.array_equal(again, before) and st_again == wst0 and len(short) == 250
    rc, flags, offs, crcs, used, st = _fused_raw(short, src, recs, chunks, True, g.ptr + 64, needed)
    assert rc == 0 and used == needed and np.array_equal(flags, want) and st == wst and len(short) == 750
    got = g.download()
    assert got[64:64 + needed].tobytes() == bytes(blob) and np.all(got[:64] == 0xA5) and np.all(got[64 + needed:] == 0xA5)
    g.free()
    src.free()
    for k in (fused, twin, short):
        k.close()
