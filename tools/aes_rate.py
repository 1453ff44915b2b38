"""Rate of AES-256-GCM on the device (pbsgpu_aes_gcm_many_device, and pbsgpu_blob_decode3_device over encrypted blobs of the
same chunks), in GB/s of payload, beside what it is measured against:

* EVP_aes_256_gcm of the same ciphertext on 16 host threads, where libcrypto loads (ctypes releases the GIL); the host's
  tags are compared with the device's on the way, so the run is a check as well;
* blob_decode of the same chunks stored as uncompressed blobs, without digests: what a restore costs when nothing is
  encrypted.

The chunks: `--chunks` of seeded sizes between 64 KiB and 4 MiB (4 096 by default, about 8 GiB), filled on the device,
encrypted there with 16-byte IVs, then decrypted. Each figure is the median of `--reps` synchronous calls timed with a host
clock after one warm-up call, with the fastest and the slowest beside it: the spread is what a difference has to be read
against. Prints one JSON line.

    python tools/aes_rate.py [--chunks 4096] [--reps 5] [--host-chunks 512]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _spread(fn, reps):
    """[fastest, median, slowest] of reps calls after one warm-up, in seconds"""
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts), statistics.median(ts), max(ts)


def _put(res, name, total, ts):
    res[name + "_ms"] = [round(t * 1e3, 3) for t in ts]
    res[name + "_GBps"] = round(total / ts[1] / 1e9, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-chunks", type=int, default=512, help="chunks the host decrypts (their bytes are downloaded)")
    a = ap.parse_args()
    import aes_inputs as ai
    from pbs_plus_amd import RECORD_DTYPE, AesKey, Engine, buzhash

    rng = np.random.default_rng(4096)
    sizes = rng.integers(64 << 10, (4 << 20) + 1, a.chunks).astype(np.uint64)
    ends = np.cumsum(sizes)
    segs = np.stack([ends - sizes, sizes], axis=1)
    total = int(ends[-1])
    key_bytes = ai.pattern(32, 9001)
    ivs = np.frombuffer(ai.pattern(16 * a.chunks, 9002), np.uint8).reshape(-1, 16)
    eng = Engine(buzhash.NewConfig(4 << 20), device=0)
    key = AesKey(eng, key_bytes)
    plain, cipher, back = eng.alloc(total), eng.alloc(total), eng.alloc(total)
    eng.fill(plain.ptr, total, 7, 0)
    res = {"chunks": a.chunks, "payload_bytes": total, "reps": a.reps}

    _, status, tags, _ = eng.aes_gcm_many(key, plain, segs, ivs, out=segs, dst=cipher, encrypt=True)
    assert not status.any()
    _put(res, "encrypt", total, _spread(lambda: eng.aes_gcm_many(key, plain, segs, ivs, out=segs, dst=cipher, encrypt=True), a.reps))
    _, status, _, _ = eng.aes_gcm_many(key, cipher, segs, ivs, tags=tags, out=segs, dst=back)
    assert not status.any()
    for i in (0, a.chunks // 2, a.chunks - 1):  # decrypt(encrypt(x)) = x on the first, a middle and the last chunk
        o, n = int(segs[i, 0]), int(segs[i, 1])
        assert np.array_equal(plain.download(o, n), back.download(o, n)), i
    _put(res, "decrypt", total, _spread(lambda: eng.aes_gcm_many(key, cipher, segs, ivs, tags=tags, out=segs, dst=back), a.reps))

    # the same chunks as uncompressed blobs, restored without digests
    blobs, offs, _ = eng.blob_encode(plain, segs)
    idx = np.zeros(a.chunks, dtype=RECORD_DTYPE)
    idx["size"] = sizes
    idx["end"] = ends
    ranges = np.stack([offs[:-1], offs[1:] - offs[:-1]], axis=1)
    _, status, _ = eng.blob_decode(blobs, ranges, idx, None, None, None, False, dst=back)
    assert not status.any()
    _put(res, "blob_decode_plain", total, _spread(lambda: eng.blob_decode(blobs, ranges, idx, None, None, None, False, dst=back), a.reps))
    blobs.free()

    # the same chunks as encrypted blobs (magic | CRC | IV | tag | ciphertext), restored with the key: encrypted straight into
    # the blobs' layout, IVs and tags written behind the headers, the CRCs taken on the device
    from pbs_plus_amd import blob_magic

    blens = sizes + np.uint64(44)
    boffs = np.cumsum(blens) - blens
    eblobs = eng.alloc(int(blens.sum()))
    where = np.stack([boffs + np.uint64(44), sizes], axis=1)
    _, status, etags, _ = eng.aes_gcm_many(key, plain, segs, ivs, out=where, dst=eblobs, encrypt=True)
    assert not status.any() and np.array_equal(etags, tags)
    for i in range(a.chunks):
        eblobs.upload(np.concatenate([ivs[i], etags[i]]), int(boffs[i]) + 12)
    crcs = eng.crc32_many(eblobs, where)  # (the CRC covers what follows the 44-byte header)
    magic = np.frombuffer(blob_magic(2), np.uint8)
    for i in range(a.chunks):
        eblobs.upload(np.concatenate([magic, np.frombuffer(int(crcs[i]).to_bytes(4, "little"), np.uint8)]), int(boffs[i]))
    eranges = np.stack([boffs, blens], axis=1)
    fn = lambda: eng.blob_decode3(eblobs, eranges, idx, None, None, None, False, dst=back, zstd=False, key=key)  # noqa: E731
    _, status, st = fn()
    assert not status.any() and st["aes_bytes"] == total, (status[status != 0][:4], st)
    for i in (0, a.chunks // 2, a.chunks - 1):
        o, n = int(segs[i, 0]), int(segs[i, 1])
        assert np.array_equal(plain.download(o, n), back.download(o, n)), i
    _put(res, "blob_decode3_encrypted", total, _spread(fn, a.reps))
    eblobs.free()

    # the host: EVP_aes_256_gcm decrypting a share of the same ciphertext on 16 threads
    lib = ai.libcrypto()
    if lib is None:
        res["host16"] = "libcrypto does not load here"
    else:
        nh = min(a.host_chunks, a.chunks)
        host = [cipher.download(int(segs[i, 0]), int(segs[i, 1])) for i in range(nh)]
        hbytes = int(sizes[:nh].sum())
        vp = C.c_void_p
        lib.EVP_CIPHER_CTX_new.restype = vp
        lib.EVP_aes_256_gcm.restype = vp
        cipher_t = vp(lib.EVP_aes_256_gcm())
        outs = [np.empty(4 << 20, np.uint8) for _ in range(16)]

        def part(k):
            ctx, n = vp(lib.EVP_CIPHER_CTX_new()), C.c_int(0)
            good = 0
            for i in range(k, nh, 16):
                lib.EVP_DecryptInit_ex(ctx, cipher_t, None, None, None)
                lib.EVP_CIPHER_CTX_ctrl(ctx, 0x9, 16, None)  # EVP_CTRL_GCM_SET_IVLEN
                lib.EVP_DecryptInit_ex(ctx, None, None, key_bytes, ivs[i].tobytes())
                lib.EVP_DecryptUpdate(ctx, vp(outs[k].ctypes.data), C.byref(n), vp(host[i].ctypes.data), host[i].size)
                lib.EVP_CIPHER_CTX_ctrl(ctx, 0x11, 16, tags[i].tobytes())  # EVP_CTRL_GCM_SET_TAG: the DEVICE's tag
                good += lib.EVP_DecryptFinal_ex(ctx, vp(outs[k].ctypes.data), C.byref(n)) == 1
            lib.EVP_CIPHER_CTX_free(ctx)
            return good

        pool16 = ThreadPoolExecutor(16)
        assert sum(pool16.map(part, range(16))) == nh, "libcrypto refuses a tag the device wrote"
        _put(res, "host16_decrypt", hbytes, _spread(lambda: list(pool16.map(part, range(16))), a.reps))
        res["host16_bytes"] = hbytes
    print(json.dumps(res), flush=True)
    key.close()
    for b in (plain, cipher, back):
        b.free()
    eng.close()


if __name__ == "__main__":
    main()
