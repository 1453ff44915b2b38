"""AES-256-GCM on the GPU (pbsgpu_aes_key_*, pbsgpu_aes_gcm_many_device) in both directions against
tests/golden/aes_gcm_v1.json (libcrypto's tags and ciphertext CRCs) and, for messages the file does not hold, against
libcrypto where it loads and the pure-Python GCM of tests/aes_inputs.py where it does not. Every destination is pre-filled
with a guard pattern and every room lies between guards, so a byte stored outside a room is seen; rooms begin at odd
offsets and sources at every residue mod 16."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aes_inputs as ai  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 67  # odd: the rooms' offsets take every parity and residue
FILL = 0xA5


@pytest.fixture(scope="module")
def eng():
    from pbs_plus_amd import Engine, buzhash

    e = Engine(buzhash.NewConfig(4096), device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def keys(eng):
    from pbs_plus_amd import AesKey

    made = {}

    def get(key):
        if key not in made:
            made[key] = AesKey(eng, key)
        return made[key]

    yield get
    for k in made.values():
        k.close()


def ref_encrypt(key, iv, plain):
    return ai.libcrypto_encrypt(key, iv, plain) if ai.libcrypto() is not None else ai.gcm_encrypt(key, iv, plain)


def run(eng, key, items, encrypt, slack=0):
    """items = [(input bytes, iv, tag or None, source residue mod 16 or None)]: the inputs in one device buffer at the
    wanted residues, every room (length + slack bytes) between guards in another that is pre-filled with the pattern.
    Returns per item (status, tag, the room's bytes) after checking that every byte outside the rooms' first `length`
    bytes is still the pattern."""
    buf, ranges = bytearray(), []
    for data, _, _, residue in items:
        pad = 0 if residue is None else (residue - len(buf)) % 16
        buf += bytes(pad)
        ranges.append((len(buf), len(data)))
        buf += data
    host = np.frombuffer(bytes(buf) + bytes(16), np.uint8)
    out, at = [], GUARD
    for i, (data, _, _, _) in enumerate(items):
        out.append((at, len(data) + slack))
        at += len(data) + slack + GUARD + i % 3
    src, dst = eng.alloc(host.size), eng.alloc(at)
    try:
        src.upload(host)
        dst.upload(np.full(at, FILL, np.uint8))
        tags = None if encrypt else [t for _, _, t, _ in items]
        _, status, tags, _ = eng.aes_gcm_many(key, src, np.array(ranges, dtype=np.uint64).reshape(-1, 2), [iv for _, iv, _, _ in items],
                                              tags=tags, out=np.array(out, dtype=np.uint64).reshape(-1, 2), dst=dst, encrypt=encrypt)
        got = dst.download(0, at)
    finally:
        src.free()
        dst.free()
    keep = np.ones(at, dtype=bool)
    for (o, _), (data, _, _, _) in zip(out, items):
        keep[o:o + len(data)] = False
    assert np.all(got[keep] == FILL), "a byte outside a message's output was written"
    return [(int(status[i]), tags[i].tobytes(), got[o:o + len(items[i][0])].tobytes()) for i, (o, _) in enumerate(out)]


def groups():
    """the golden cases the call takes (IVs of 12 and 16 bytes), by (key, IV length)"""
    g = {}
    for c in ai.golden():
        if len(c["iv"]) in (12, 16):
            g.setdefault((c["key"], len(c["iv"])), []).append(c)
    return g


@pytest.fixture(scope="module")
def ciphertexts(eng, keys):
    """every golden case encrypted on the device, checked against the file: {name: ciphertext}. The decrypt tests start
    from these bytes, which the recorded CRC vouches for."""
    out = {}
    for (key, _), cs in groups().items():
        res = run(eng, keys(key), [(ai.pattern(c["length"], c["seed"]), c["iv"], None, 12) for c in cs], encrypt=True)
        for c, (status, tag, ct) in zip(cs, res):
            assert status == ai.OK and tag == c["tag"], c["name"]
            assert zlib.crc32(ct) == c["crc"], c["name"]
            out[c["name"]] = ct
    return out


def test_encrypt_matches_the_golden_file(ciphertexts):
    names = set(ciphertexts)
    assert {"len-%d" % n for n in ai.LENGTHS} <= names and {"iv12-len-%d" % n for n in ai.LENGTHS if n >= 50} <= names
    assert {"zero-key", "wrap-first-piece", "wrap-at-boundary", "wrap-third-piece", "wrap-short"} <= names
    assert ciphertexts["zero-key"].hex() == "cea7403d4d606b6e074ec5d3baf39d18"


def test_decrypt_matches_the_golden_file(eng, keys, ciphertexts):
    for (key, _), cs in groups().items():
        res = run(eng, keys(key), [(ciphertexts[c["name"]], c["iv"], c["tag"], (5 * i) % 16) for i, c in enumerate(cs)], encrypt=False,
                  slack=3)
        for c, (status, _, plain) in zip(cs, res):
            assert status == ai.OK, c["name"]
            assert plain == ai.pattern(c["length"], c["seed"]), c["name"]


def test_the_counter_wraps_where_the_cases_say():
    """the crafted IVs put the wrap in the first piece, on a piece boundary and in the third piece"""
    g = {c["name"]: c for c in ai.golden()}
    for name, before in (("wrap-first-piece", 100), ("wrap-at-boundary", 4096), ("wrap-third-piece", 2 * 4096 + 1000), ("wrap-short", 1)):
        c = g[name]
        assert ai.j0_of(c["key"], c["iv"]) & 0xFFFFFFFF == 0xFFFFFFFF - before, name
        assert before < -(-c["length"] // 16), name  # the wrap lies inside the message


@pytest.mark.parametrize("name", ["len-1025", "len-65537"])
def test_every_source_residue_and_odd_output_offsets(eng, keys, ciphertexts, name):
    c = next(x for x in ai.golden() if x["name"] == name)
    plain = ai.pattern(c["length"], c["seed"])
    enc = run(eng, keys(c["key"]), [(plain, c["iv"], None, r) for r in range(16)], encrypt=True)
    for r, (status, tag, ct) in enumerate(enc):
        assert status == ai.OK and tag == c["tag"] and ct == ciphertexts[name], r
    dec = run(eng, keys(c["key"]), [(ciphertexts[name], c["iv"], c["tag"], r) for r in range(16)], encrypt=False, slack=1)
    for r, (status, _, got) in enumerate(dec):
        assert status == ai.OK and got == plain, r


def test_a_batch_of_300_mixed_messages(eng, keys):
    """about 300 messages in one call, zero length included, each with its own IV: short ones against the reference GCM,
    long ones from the golden file's cases of the same key"""
    rng = np.random.default_rng(300)
    key = ai.key_of(1)
    lens = [0, 0, 1, 15, 16, 17, 31, 32, 33, 48] + [int(n) for n in rng.integers(0, 65, 250)] + [int(n) for n in rng.integers(65, 1100, 20)]
    items, want = [], []
    for i, n in enumerate(lens):
        plain, iv = ai.pattern(n, 5000 + i), ai.pattern(16, 6000 + i)
        ct, tag = ref_encrypt(key, iv, plain)
        items.append((plain, iv, None, None))
        want.append((ct, tag))
    long_cases = [c for c in ai.golden() if c["key"] == key and len(c["iv"]) == 16 and c["length"] >= 1023]
    for c in long_cases:
        items.insert(len(items) // 2, (ai.pattern(c["length"], c["seed"]), c["iv"], None, None))
        want.insert(len(want) // 2, (None, c["tag"]))
    assert len(items) >= 290 and len({iv for _, iv, _, _ in items}) == len(items)
    enc = run(eng, keys(key), items, encrypt=True)
    for i, ((status, tag, ct), (wct, wtag)) in enumerate(zip(enc, want)):
        assert status == ai.OK and tag == wtag, (i, len(items[i][0]))
        assert wct is None or ct == wct, (i, len(items[i][0]))
    dec = run(eng, keys(key), [(ct, items[i][1], tag, None) for i, (_, tag, ct) in enumerate(enc)], encrypt=False, slack=2)
    for i, (status, _, plain) in enumerate(dec):
        assert status == ai.OK and plain == items[i][0], (i, len(items[i][0]))


def test_a_bad_tag_zeroes_its_own_output_and_nothing_else(eng, keys, ciphertexts):
    g = {c["name"]: c for c in ai.golden()}
    names = ["len-33", "len-1025", "len-65537", "len-17", "len-131077", "len-4097", "len-16"]
    cs = [g[n] for n in names]
    key = cs[0]["key"]
    assert all(c["key"] == key for c in cs)

    def flip(b, at):
        b = bytearray(b)
        b[at] ^= 0x10
        return bytes(b)

    items = [(ciphertexts[c["name"]], c["iv"], c["tag"], None) for c in cs]
    items[0] = (flip(items[0][0], 32), items[0][1], items[0][2], None)      # a ciphertext byte, in the partial block
    items[1] = (items[1][0], items[1][1], flip(items[1][2], 15), None)      # a tag byte
    items[2] = (items[2][0], flip(items[2][1], 7), items[2][2], None)       # an IV byte
    items[4] = (flip(items[4][0], 70000), items[4][1], items[4][2], None)   # a ciphertext byte in the second piece
    res = run(eng, keys(key), items, encrypt=False, slack=5)  # (run: the slack behind a zeroed output is still the pattern)
    for i, (c, (status, _, got)) in enumerate(zip(cs, res)):
        if i in (0, 1, 2, 4):
            assert status == ai.BAD_TAG and got == bytes(c["length"]), c["name"]
        else:
            assert status == ai.OK and got == ai.pattern(c["length"], c["seed"]), c["name"]


def test_two_keys_on_one_engine_do_not_mix(eng, keys):
    a, b = ai.key_of(1), ai.key_of(2)
    plain, iv = ai.pattern(1000, 77), ai.pattern(16, 78)
    (sa, ta, ca), = run(eng, keys(a), [(plain, iv, None, None)], encrypt=True)
    (sb, tb, cb), = run(eng, keys(b), [(plain, iv, None, None)], encrypt=True)
    assert (ca, ta) == ref_encrypt(a, iv, plain) and (cb, tb) == ref_encrypt(b, iv, plain) and ca != cb and ta != tb
    (s1, _, p1), = run(eng, keys(a), [(ca, iv, ta, None)], encrypt=False)
    (s2, _, p2), = run(eng, keys(b), [(ca, iv, ta, None)], encrypt=False)
    (s3, _, p3), = run(eng, keys(b), [(cb, iv, tb, None)], encrypt=False)
    assert (s1, p1) == (ai.OK, plain) and (s2, p2) == (ai.BAD_TAG, bytes(1000)) and (s3, p3) == (ai.OK, plain)


def test_encrypting_twice_gives_identical_bytes_and_decrypts_back(eng, keys):
    key = keys(ai.key_of(3))
    items = [(ai.pattern(n, 900 + n), ai.pattern(16, 901 + n), None, None) for n in (0, 5, 4096, 70001)]
    one, two = run(eng, key, items, encrypt=True), run(eng, key, items, encrypt=True)
    assert one == two
    back = run(eng, key, [(ct, items[i][1], tag, None) for i, (_, tag, ct) in enumerate(one)], encrypt=False)
    assert [(s, p) for s, _, p in back] == [(ai.OK, it[0]) for it in items]


def test_refusals_that_need_a_device(eng, keys):
    from pbs_plus_amd import _lib

    L, key = _lib.lib(), keys(ai.key_of(1))
    src, dst = eng.alloc(4096), eng.alloc(4096)
    try:
        dst.upload(np.full(4096, FILL, np.uint8))
        seg = np.array([[0, 100]], dtype=np.uint64)
        iv, tag, status = np.zeros(16, np.uint8), np.zeros(16, np.uint8), np.full(1, 9, np.uint8)
        hostbuf = np.zeros(4096, np.uint8)

        def call(sp=src.ptr, dp=dst.ptr, o=seg, n=4096, ivl=16, flags=0):
            return L.pbsgpu_aes_gcm_many_device(key._h, sp, n, seg.ctypes.data, 1, iv.ctypes.data, ivl, tag.ctypes.data, o.ctypes.data, dp,
                                                4096, status.ctypes.data, flags)

        E = _lib.E_INVALID
        assert call(sp=hostbuf.ctypes.data) == E and call(dp=hostbuf.ctypes.data) == E     # host pointers
        assert call(sp=dst.ptr) == E                                                       # the output inside the source
        assert call(o=np.array([[0, 99]], dtype=np.uint64)) == E                           # a room shorter than its message
        assert call(ivl=8) == E and call(ivl=60) == E and call(flags=2) == E and call(n=99) == E
        assert status[0] == 9 and np.all(dst.download(0, 4096) == FILL)
        assert call() == _lib.OK and status[0] == ai.BAD_TAG and np.all(dst.download(0, 100) == 0)  # (a zero tag over zero bytes)
        assert np.all(dst.download(100, 3996) == FILL)
    finally:
        src.free()
        dst.free()
