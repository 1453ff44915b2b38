"""Inputs of the AES-256-GCM tests: the cases, a seeded byte pattern, a small pure-Python AES-256-GCM (slow: short
messages only; it needs no library), IVs crafted for a wanted pre-counter block, and the golden file
(tests/golden/aes_gcm_v1.json, made by tests/golden/make_aes_golden.py with libcrypto)."""
import ctypes
import ctypes.util
import functools
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "aes_gcm_v1.json")
ZEROS = 0xFFFFFFFF  # the seed of an all-zero pattern
PIECE = 65536
OK, BAD_TAG = 0, 1

# the lengths the GPU test runs: around a block, around one stride of a piece's lanes (256 blocks), around a wave's
# (1 024 bytes), around a piece, and 2, 3 and 5 pieces with odd tails
LENGTHS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 65535, 65536, 65537, 2 * 65536 + 5, 3 * 65536 - 16, 5 * 65536 + 33)


def pattern(n, seed):
    """n bytes that depend on every bit of the index (tests/native/test_aes_gcm.cpp makes the same)"""
    if seed == ZEROS:
        return bytes(n)
    i = np.arange(n, dtype=np.uint64)
    x = ((i + np.uint64(seed * 7919)) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    return (((x >> np.uint64(24)) ^ (x >> np.uint64(9))) & np.uint64(0xFF)).astype(np.uint8).tobytes()


# ---- GF(2^128) in GCM's bit order, blocks as big-endian integers ----

R = 0xE1 << 120
ONE = 1 << 127


def gf_mul(x, y):
    z = 0
    for i in range(127, -1, -1):
        if x >> i & 1:
            z ^= y
        y = (y >> 1) ^ (R if y & 1 else 0)
    return z


def gf_pow(x, n):
    r = ONE
    while n:
        if n & 1:
            r = gf_mul(r, x)
        x = gf_mul(x, x)
        n >>= 1
    return r


def gf_inv(x):
    return gf_pow(x, (1 << 128) - 2)


# ---- AES-256, forward ----

@functools.lru_cache(maxsize=None)
def _sbox():
    s = [0] * 256
    p = q = 1
    while True:
        p = (p ^ (p << 1) ^ (0x1B if p & 0x80 else 0)) & 0xFF
        q ^= q << 1
        q ^= q << 2
        q ^= q << 4
        q &= 0xFF
        if q & 0x80:
            q ^= 0x09
        x = q ^ ((q << 1 | q >> 7) & 0xFF) ^ ((q << 2 | q >> 6) & 0xFF) ^ ((q << 3 | q >> 5) & 0xFF) ^ ((q << 4 | q >> 4) & 0xFF)
        s[p] = x ^ 0x63
        if p == 1:
            break
    s[0] = 0x63
    return tuple(s)


def _xt(b):
    return ((b << 1) ^ (0x1B if b & 0x80 else 0)) & 0xFF


@functools.lru_cache(maxsize=16)
def _round_keys(key):
    s = _sbox()
    w = [list(key[4 * i:4 * i + 4]) for i in range(8)]
    rcon = 1
    for i in range(8, 60):
        t = list(w[i - 1])
        if i % 8 == 0:
            t = [s[b] for b in t[1:] + t[:1]]
            t[0] ^= rcon
            rcon = _xt(rcon)
        elif i % 8 == 4:
            t = [s[b] for b in t]
        w.append([a ^ b for a, b in zip(w[i - 8], t)])
    return tuple(bytes(sum(w[4 * r:4 * r + 4], [])) for r in range(15))


def aes_encrypt_block(key, block):
    s, rk = _sbox(), _round_keys(bytes(key))
    st = [a ^ b for a, b in zip(block, rk[0])]
    for r in range(1, 15):
        st = [s[b] for b in st]
        st = [st[(i + 4 * (i % 4)) % 16] for i in range(16)]  # ShiftRows on the column-major state
        if r < 14:
            out = []
            for c in range(4):
                a = st[4 * c:4 * c + 4]
                out += [_xt(a[i]) ^ _xt(a[(i + 1) % 4]) ^ a[(i + 1) % 4] ^ a[(i + 2) % 4] ^ a[(i + 3) % 4] for i in range(4)]
            st = out
        st = [a ^ b for a, b in zip(st, rk[r])]
    return bytes(st)


# ---- GCM, AAD empty ----

def _int(b):
    return int.from_bytes(b, "big")


def hash_key(key):
    return _int(aes_encrypt_block(key, bytes(16)))


def ghash(h, data, lenblock):
    y = 0
    for i in range(0, len(data), 16):
        y = gf_mul(y ^ _int(data[i:i + 16].ljust(16, b"\0")), h)
    return gf_mul(y ^ lenblock, h)


def j0_of(key, iv):
    if len(iv) == 12:
        return _int(iv) << 32 | 1
    return ghash(hash_key(key), iv, len(iv) * 8)


def gcm_encrypt(key, iv, plain):
    """(ciphertext, tag)"""
    j0 = j0_of(key, iv)
    out = bytearray()
    for k in range(0, len(plain), 16):
        ctr = (j0 & ~0xFFFFFFFF) | ((j0 + 1 + k // 16) & 0xFFFFFFFF)
        ks = aes_encrypt_block(key, ctr.to_bytes(16, "big"))
        out += bytes(a ^ b for a, b in zip(plain[k:k + 16], ks))
    s = ghash(hash_key(key), bytes(out), len(out) * 8)
    return bytes(out), (s ^ _int(aes_encrypt_block(key, j0.to_bytes(16, "big")))).to_bytes(16, "big")


def craft_iv(key, j0):
    """the 16-byte IV whose pre-counter block is j0: J0 = IV * H^2 ^ [128] * H, so IV = (J0 ^ [128] * H) * H^-2"""
    h = hash_key(key)
    iv = gf_mul(j0 ^ gf_mul(128, h), gf_inv(gf_mul(h, h)))
    assert j0_of(key, iv.to_bytes(16, "big")) == j0
    return iv.to_bytes(16, "big")


# ---- the cases: (name, key, iv, length, seed) ----

def key_of(k):
    return bytes(32) if k == 0 else pattern(32, 2000 + k)


def wrap_iv(key, blocks_before_wrap, salt):
    """an IV whose counter's low word passes 2^32 - 1 after that many blocks of the message"""
    top = _int(pattern(12, 3000 + salt))
    return craft_iv(key, top << 32 | ((1 << 32) - 1 - blocks_before_wrap))


def cases():
    out = [("zero-key", bytes(32), bytes(12), 16, ZEROS)]  # C = cea7403d..., T = d0d1c8a7...
    for n in range(50):
        out.append(("len-%d" % n, key_of(1), pattern(16, 100 + n), n, n))
    for ivn in (8, 12, 60):
        for n in (0, 1, 16, 33):
            out.append(("iv%d-len-%d" % (ivn, n), key_of(2), pattern(ivn, 200 + n), n, 300 + n))
    for n in LENGTHS:
        if n >= 50:
            out.append(("len-%d" % n, key_of(1), pattern(16, 100 + n), n, n))
            out.append(("iv12-len-%d" % n, key_of(2), pattern(12, 100 + n), n, n + 1))
    # the counter's low word wraps in the first piece, exactly at a piece boundary, and in the third piece
    k = key_of(3)
    out.append(("wrap-first-piece", k, wrap_iv(k, 100, 1), 5 * PIECE + 33, 401))
    out.append(("wrap-at-boundary", k, wrap_iv(k, 4096, 2), 3 * PIECE - 16, 402))  # block 0 of piece 1 has counter 0
    out.append(("wrap-third-piece", k, wrap_iv(k, 2 * 4096 + 1000, 3), 5 * PIECE + 33, 403))
    out.append(("wrap-short", k, wrap_iv(k, 1, 4), 33, 404))  # J0 ends in 0xFFFFFFFE
    return out


@functools.lru_cache(maxsize=1)
def golden():
    """the recorded cases: dicts with name, key, iv, length, seed, tag, crc (of the ciphertext)"""
    g = json.load(open(GOLDEN))
    keys = [bytes.fromhex(k) for k in g["keys"]]
    return [dict(name=name, key=keys[k], iv=bytes.fromhex(iv), length=n, seed=seed, tag=bytes.fromhex(tag), crc=crc)
            for name, k, iv, n, seed, tag, crc in g["cases"]]


# ---- libcrypto, where it loads ----

@functools.lru_cache(maxsize=1)
def libcrypto():
    for name in ("libcrypto.so.3", ctypes.util.find_library("crypto")):
        try:
            lib = ctypes.CDLL(name)
            lib.EVP_CIPHER_CTX_new.restype = ctypes.c_void_p
            lib.EVP_aes_256_gcm.restype = ctypes.c_void_p
            return lib
        except (OSError, TypeError, AttributeError):
            continue
    return None


def libcrypto_encrypt(key, iv, plain):
    """(ciphertext, tag) by EVP_aes_256_gcm"""
    lib, vp = libcrypto(), ctypes.c_void_p
    ctx = vp(lib.EVP_CIPHER_CTX_new())
    try:
        assert lib.EVP_EncryptInit_ex(ctx, vp(lib.EVP_aes_256_gcm()), None, None, None) == 1
        assert lib.EVP_CIPHER_CTX_ctrl(ctx, 0x9, len(iv), None) == 1  # EVP_CTRL_GCM_SET_IVLEN
        assert lib.EVP_EncryptInit_ex(ctx, None, None, bytes(key), bytes(iv)) == 1
        out, n = ctypes.create_string_buffer(len(plain) + 16), ctypes.c_int(0)
        if plain:
            assert lib.EVP_EncryptUpdate(ctx, out, ctypes.byref(n), bytes(plain), len(plain)) == 1
        done = n.value
        assert lib.EVP_EncryptFinal_ex(ctx, ctypes.byref(out, done), ctypes.byref(n)) == 1
        tag = ctypes.create_string_buffer(16)
        assert lib.EVP_CIPHER_CTX_ctrl(ctx, 0x10, 16, tag) == 1  # EVP_CTRL_GCM_GET_TAG
        return out.raw[:done + n.value], tag.raw
    finally:
        lib.EVP_CIPHER_CTX_free(ctx)
