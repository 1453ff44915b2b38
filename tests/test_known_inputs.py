"""The crafted inputs of tests/test_gpu_known_collisions.py, without a GPU (tests/known_inputs.py):
- the inverse of the mix;
- every family those tests use, hashed by the C++ of pbs_plus_amd/csrc/known_hash.h (tests/native/test_known_hash.cpp, built
  with ASan + UBSan): home, key and tag equal the Python port's and the claimed equalities hold, so the inputs are bound to
  the hash the kernels run — change the mix and this fails, rather than the GPU tests quietly turning random;
- every scenario replayed on TableModel: the chain, the probe length, the growth step and the run length it claims.
These are conditions on the INPUTS, checked against the model, never against the library."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import known_inputs as K  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scenarios():
    out = [("one_home_%s" % n, K.scenario_one_home(H)) for n, H in (("last", K.HOME_LAST), ("first", K.HOME_FIRST),
                                                                   ("mid", K.HOME_MID))]
    out += [("one_key", K.scenario_one_key()), ("equal_tag_home_key", K.scenario_equal_tag_home_key()),
            ("load_boundary", K.scenario_load_boundary()), ("fused", K.scenario_fused())]
    return out


def test_unmix_inverts_mix():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.integers(0, 1 << 64, 10_000, dtype=np.uint64),
                        np.array([0, 1, 1 << 63, (1 << 64) - 1], dtype=np.uint64)])
    assert np.array_equal(K.unmix(K.mix(x)), x)
    assert np.array_equal(K.mix(K.unmix(x)), x)
    # splitmix64's first output for seed 0 is the finaliser of its increment
    assert int(K.mix(0)) == 0 and int(K.mix(0x9E3779B97F4A7C15)) == 0xE220A8397B1DCDAF
    assert int(K.unmix(K.mix((1 << 64) - 1))) == (1 << 64) - 1


def test_home_constants():
    assert K.HOME_LAST & 0xFFFFFF == 0xFFFFFF and K.HOME_FIRST & 0xFFFFFF == 0
    assert K.HOME_MID & 0xFFFFFF == 512


@pytest.fixture(scope="module")
def hash_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("known_hash") / "test_known_hash")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
             "-Werror"]
    subprocess.run(["g++", *flags, os.path.join(ROOT, "tests", "native", "test_known_hash.cpp"), "-o", exe], check=True)
    return exe


def _native(exe, digests):
    """(home, key, tag) of every digest as the C++ computes them"""
    d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
    text = "".join(bytes(x).hex() + "\n" for x in d)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == "known-hash-ok" and len(lines) == d.shape[0] + 1
    cols = [ln.split() for ln in lines[:-1]]
    return (np.array([int(c[0], 16) for c in cols], dtype=np.uint64), np.array([int(c[1], 16) for c in cols], dtype=np.uint32),
            np.array([int(c[2], 16) for c in cols], dtype=np.uint64))


def test_port_equals_the_native_hash_on_plain_digests(hash_driver):
    rng = np.random.default_rng(2)
    d = K.random_digests(rng, 2000)
    d[0] = 0
    d[1] = 0xFF
    d[2, :8] = 0                                                     # tag 0 -> 1
    d[3] = np.arange(32)                                             # byte order: word 0 = 0x0706050403020100
    h, k, t = _native(hash_driver, d)
    assert np.array_equal(h, K.home(d)) and np.array_equal(k, K.key(d)) and np.array_equal(t, K.tag(d))
    assert int(t[0]) == 1 and int(t[2]) == 1 and int(t[3]) == 0x0706050403020100


def test_every_family_holds_its_claims_under_the_native_hash(hash_driver):
    nfam = 0
    for sname, sc in _scenarios():
        for fname, d, claims in sc["families"]:
            name = sname + "/" + fname
            h, k, t = _native(hash_driver, d)
            assert np.array_equal(h, K.home(d)) and np.array_equal(k, K.key(d)) and np.array_equal(t, K.tag(d)), name
            assert np.unique(d, axis=0).shape[0] == d.shape[0], name
            w = K.words(d)
            if "home" in claims:
                assert np.all(h == np.uint64(claims["home"])), name
            else:                                                    # spread: (nearly) every digest a home slot of its own
                assert np.unique(h & np.uint64(1023)).size > d.shape[0] // 2, name
            if "key" in claims:
                assert np.all(k == np.uint32(claims["key"])), name
            if "w0" in claims:
                assert np.all(w[:, 0] == np.uint64(claims["w0"])), name
                assert np.unique(k).size == 1 and np.unique(t).size == 1, name
                assert int(t[0]) == (claims["w0"] or 1), name
                assert np.unique(d[:, 8:], axis=0).shape[0] == d.shape[0], name      # bytes 8..31 alone tell them apart
            if "w1" in claims:
                assert np.all(w[:, 1] == np.uint64(claims["w1"])), name
                assert np.unique(d[:, :16], axis=0).shape[0] == 1, name
            nfam += 1
    assert nfam == 3 + 6 + 4 + 1 + 2
    # the w0 = 0 and w0 = 1 families of one home: different digests and keys, one stored tag
    fam = dict((f[0], f) for f in K.scenario_equal_tag_home_key()["families"])
    assert np.all(K.tag(fam["tag_zero"][1]) == 1) and np.all(K.tag(fam["tag_one"][1]) == 1)
    assert fam["tag_zero"][2]["home"] == fam["tag_one"][2]["home"]


# ---- the scenarios on the table's model ----

def _chain(start, n, slots):
    return {(start + i) & (slots - 1) for i in range(n)}


@pytest.mark.parametrize("H", [K.HOME_LAST, K.HOME_FIRST, K.HOME_MID], ids=["last", "first", "mid"])
def test_scenario_one_home_on_the_model(H):
    sc = K.scenario_one_home(H)
    t = K.TableModel.for_capacity(16)
    assert t.slots == 1024
    assert not t.insert(sc["a"]) and t.count == 400
    start = H & 1023
    assert t.occupied() == _chain(start, 400, 1024)
    if H == K.HOME_LAST:
        assert t.occupied() == {1023} | set(range(399))              # the last slot, then slot 0 onwards
    assert max(t.probe(d)[1] for d in sc["a"]) == 400
    for d in sc["b"][:5]:
        assert t.probe(d) == (False, 401)                            # absent: the whole chain, then the empty slot
    assert len(K.digest_set(sc["q_ab"])) == 800 and sc["q_ab"].shape[0] == 1067
    assert t.insert(sc["b"]) and t.slots == 2048 and t.count == 800 and t.growths == 1
    assert t.occupied() == _chain(H & 2047, 800, 2048)
    if H == K.HOME_LAST:
        assert {2047, 0, 798} <= t.occupied()                        # the rehashed chain wraps again
    assert sc["q_all"].shape[0] == 1350 and len(K.digest_set(sc["q_all"])) == 1200
    assert t.insert(sc["c"]) and t.slots == 4096 and t.count == 1200
    assert t.occupied() == _chain(H & 4095, 1200, 4096)


@pytest.mark.parametrize("shuffle_seed", [0, 1, 2])
def test_scenario_one_key_on_the_model(shuffle_seed):
    sc = K.scenario_one_key(shuffle_seed=shuffle_seed)
    batch = sc["batch"]
    n = batch.shape[0]
    assert 2800 <= n <= 4000
    keys = K.key(batch)
    order = np.argsort(keys, kind="stable")                          # the device's stable sort
    skeys, sdig = keys[order], batch[order]
    assert sc["keys"][:2] == [0, 0xFFFFFFFF]
    for Kv, want_len in zip(sc["keys"], sc["run_lengths"]):
        pos = np.nonzero(skeys == np.uint32(Kv))[0]
        assert pos.size == want_len and 800 <= want_len <= 1200      # the run length is the stated one
        assert pos[-1] - pos[0] + 1 == pos.size                      # contiguous
        if Kv == 0:
            assert pos[0] == 0                                       # the walk's q > 0 bound
        if Kv == 0xFFFFFFFF:
            assert pos[-1] == n - 1
        assert pos[0] // 256 != pos[-1] // 256                       # crosses a 256-thread block
        run = [bytes(d) for d in sdig[pos]]
        assert len(set(run)) == 400
        # how far the mark walk goes: a first occurrence walks to the run's start, a repeat to its nearest earlier copy
        last, far, behind_other = {}, 0, 0
        for j, b in enumerate(run):
            if b in last:
                far = max(far, j - last[b])
                behind_other += j - last[b] > 1                      # A B A: a different digest in between
            else:
                far = max(far, j)
            last[b] = j
        assert far >= 256 and behind_other >= 300, (far, behind_other)
    # the random digests hold no run of their own kind worth the name (that is what the suite had before)
    assert n - sum(sc["run_lengths"]) == 500
    assert sc["distinct"].shape[0] == 1700 and len(K.digest_set(sc["distinct"])) == 1700
    t = K.TableModel.for_capacity(16)
    assert t.insert(sc["preload"]) and t.count == 567                # 567 > 512: the preload itself grows the table
    t.insert(batch)
    assert t.count == 1700


def test_scenario_equal_tag_home_key_on_the_model():
    sc = K.scenario_equal_tag_home_key()
    assert sc["all"].shape[0] == 700 and len(K.digest_set(sc["all"])) == 700
    assert sc["content"].shape[0] == 350 and sc["queries"].shape[0] == 700 + 233
    t = K.TableModel.for_capacity(16)
    assert not t.insert(sc["content"])
    in_set = K.digest_set(sc["content"])
    # a stored digest and an absent one that agree in tag, home and key: only the 32-byte compare tells them apart
    fam = dict((f[0], f[1]) for f in sc["families"])
    for name in ("w0", "w0_w1"):
        have = [d for d in fam[name] if bytes(d) in in_set]
        lack = [d for d in fam[name] if bytes(d) not in in_set]
        assert len(have) >= 30 and len(lack) >= 30, name
        assert t.probe(lack[0])[1] > len(have)                       # walks past every stored one of its kind
    # in the batch's sorted order, the w0 families form one run of equal keys holding many distinct digests
    k = K.key(sc["queries"])
    assert (k == K.key(fam["w0"][:1])[0]).sum() >= 400
    t.insert(sc["queries"])
    assert t.count == 700


def test_scenario_load_boundary_on_the_model():
    sc = K.scenario_load_boundary()
    t = K.TableModel.for_capacity(16)
    assert not t.insert(sc["first"]) and t.count == 511
    assert not t.insert(sc["d512"]) and t.count == 512 == t.slots // 2 and t.slots == 1024    # at the limit: no growth
    assert t.occupied() == {1023} | set(range(511))
    assert t.probe(sc["absent"][0]) == (False, 513)                  # 512 occupied slots, then the empty one
    assert t.insert(sc["d513"]) and t.count == 513 and t.slots == 2048                        # one more: growth
    assert t.probe(sc["absent"][0]) == (False, 514)


def test_scenario_fused_on_the_model():
    sc = K.scenario_fused()
    assert sc["batch"].shape[0] == 1500 and sc["distinct"].shape[0] == 750 == len(K.digest_set(sc["batch"]))
    ch = sc["chunks"]
    assert ch.shape == (1500, 2) and int(ch[:, 1].max()) == 3000 and int(ch[:, 1].min()) == 0
    assert np.all(ch[:, 0] + ch[:, 1] <= sc["nbytes"])
    t = K.TableModel.for_capacity(16)
    assert not t.insert(sc["preload"]) and t.count == 250
    assert t.insert(sc["batch"]) and t.count == 750 and t.slots == 2048       # the table grows inside the fused call
    for _, d, claims in sc["families"]:
        assert (K.key(sc["batch"]) == np.uint32(claims["key"])).sum() >= 500  # two long runs of one key each
