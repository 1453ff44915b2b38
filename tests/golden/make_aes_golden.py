"""Writes tests/golden/aes_gcm_v1.json: the cases of tests/aes_inputs.py encrypted by libcrypto's EVP_aes_256_gcm
(through ctypes; EVP_CTRL_GCM_SET_IVLEN sets the IV's length). Per case: name, key (an index into "keys"), IV, length,
pattern seed, tag and the CRC-32 of the ciphertext; the content is regenerated from the pattern. The short cases are
checked against the pure-Python GCM on the way. No test needs libcrypto to run.

    python tests/golden/make_aes_golden.py
"""
import json
import os
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aes_inputs as ai  # noqa: E402


def main():
    assert ai.libcrypto() is not None, "libcrypto does not load here"
    keys, rows = [], []
    for name, key, iv, n, seed in ai.cases():
        plain = ai.pattern(n, seed)
        ct, tag = ai.libcrypto_encrypt(key, iv, plain)
        assert len(ct) == n
        if n <= 64:
            assert (ct, tag) == ai.gcm_encrypt(key, iv, plain), name
        if key.hex() not in keys:
            keys.append(key.hex())
        rows.append([name, keys.index(key.hex()), iv.hex(), n, seed, tag.hex(), zlib.crc32(ct)])
    zero = rows[0]
    assert zero[0] == "zero-key" and zero[5] == "d0d1c8a799996bf0265b98b5d48ab919"
    with open(ai.GOLDEN, "w") as f:
        f.write('{"format": "aes-256-gcm, empty AAD; cases: name, key, iv, length, pattern seed, tag, crc32(ciphertext)",\n "keys": ')
        f.write(json.dumps(keys) + ',\n "cases": [\n  ')
        f.write(",\n  ".join(json.dumps(r) for r in rows))
        f.write("\n ]}\n")
    print("%d cases, %d bytes" % (len(rows), os.path.getsize(ai.GOLDEN)))


if __name__ == "__main__":
    main()
