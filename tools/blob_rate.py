"""Rates of the data-blob calls (pbsgpu_crc32_* / pbsgpu_blob_*) on one GPU, in GB/s of chunk bytes:

* crc32_many on device bytes and on host bytes (the host variant moves the bytes through pinned staging first);
* blob_encode_device (one pass: the CRC and the copy into the blobs);
* blob_verify_device with sizes and digests (CRC + SHA-256), beside sha256_many_device over the same chunks;
* the read side: blob_decode_device of the whole stream of those blobs, with and without the digest check, beside the
  composition it replaces, blob_verify_device (sizes + digests) followed by pbsgpu_gather_device of the same chunks
  (--no-decode leaves the decode leg out: the composition alone, for a build that has no blob_decode).

Two batches of device-resident chunks: fixed 4 MiB chunks (NewConfig(4 << 20)'s average) and chunks of 1-7 KiB, 4 KiB on
average (NewConfig(4096)). The corpus is written on the device by the engine's fill kernel. Each figure is the median of
a few synchronous calls timed with a host clock, after one warm-up call.

    python tools/blob_rate.py [--big-gib 2] [--small-mib 256] [--reps 5] [--no-decode]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _median_s(fn, reps):
    fn()  # warm-up (first-use allocation of the leased work buffers)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big-gib", type=float, default=2.0, help="corpus of the 4 MiB-chunk batch")
    ap.add_argument("--small-mib", type=int, default=256, help="corpus of the 4 KiB-average batch")
    ap.add_argument("--host-gib", type=float, default=1.0, help="bytes of the host-variant CRC batch")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-decode", action="store_true", help="skip blob_decode (a build without it): the composition only")
    a = ap.parse_args()

    from pbs_plus_amd import Engine, _lib, buzhash
    from pbs_plus_amd.engine import _segs

    eng = Engine(buzhash.NewConfig(4 << 20), device=0)
    L = _lib.lib()
    rng = np.random.default_rng(7)
    big = int(a.big_gib * (1 << 30)) // (4 << 20) * (4 << 20)
    small = a.small_mib << 20
    batches = []
    # 4 MiB chunks, each at a 16-byte-unaligned offset (+5: the loads and the blob stores are never dword-aligned)
    n4 = big // (4 << 20) - 1
    batches.append(("4MiB", big, [(i * (4 << 20) + 5, 4 << 20) for i in range(n4)]))
    lens = rng.integers(1024, 7169, small // 4096)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    keep = offs + lens <= small
    batches.append(("4KiB-avg", small, list(zip(offs[keep].tolist(), lens[keep].tolist()))))
    rows = []
    for name, nbytes, chunks in batches:
        src = eng.alloc(nbytes)
        eng.fill(src.ptr, nbytes, seed=0xB10B, kind=0)
        data = sum(n for _, n in chunks)
        segs, n = _segs(chunks)
        out32 = np.zeros(n, dtype=np.uint32)
        digs = np.zeros((n, 32), dtype=np.uint8)
        t_crc = _median_s(lambda: _lib.check(L.pbsgpu_crc32_many_device(eng._h, src.ptr, nbytes, segs, n, out32.ctypes.data),
                                             "crc32_many_device"), a.reps)
        total = C.c_uint64()
        _lib.check(L.pbsgpu_blob_encoded_size(segs, n, C.byref(total)), "blob_encoded_size")
        dst = eng.alloc(total.value)
        offs_out = np.zeros(n + 1, dtype=np.uint64)

        def encode():
            _lib.check(L.pbsgpu_blob_encode_device(eng._h, src.ptr, nbytes, segs, n, dst.ptr, dst.nbytes, C.byref(total),
                                                   offs_out.ctypes.data, out32.ctypes.data), "blob_encode_device")

        t_enc = _median_s(encode, a.reps)
        _lib.check(L.pbsgpu_sha256_many_device(eng._h, src.ptr, nbytes, segs, n, digs.ctypes.data), "sha256_many_device")
        t_sha = _median_s(lambda: _lib.check(L.pbsgpu_sha256_many_device(eng._h, src.ptr, nbytes, segs, n, digs.ctypes.data),
                                             "sha256_many_device"), a.reps)
        blobs = np.stack([offs_out[:-1], offs_out[1:] - offs_out[:-1]], axis=1)
        sizes = np.array([c for _, c in chunks], dtype=np.uint32)
        status, st = eng.blob_verify(dst, blobs, digs, sizes)
        assert st["ok"] == n, st
        t_ver = _median_s(lambda: eng.blob_verify(dst, blobs, digs, sizes), max(1, a.reps // 2))
        # the read side: the stream is the chunks back to back, entry i in blob i
        idx = np.zeros(n, dtype=_lib.RECORD_DTYPE)
        idx["size"] = sizes
        idx["end"] = np.cumsum(sizes.astype(np.uint64))
        idx["digest"] = digs
        back = eng.alloc(data)
        items = np.stack([blobs[:, 0] + 12, idx["end"] - sizes, sizes.astype(np.uint64)], axis=1)

        def compose():
            status, _ = eng.blob_verify(dst, blobs, digs, sizes)
            eng.gather(dst, back, items)
            return status

        assert not compose().any()
        t_cmp = _median_s(compose, a.reps)
        dec = {}
        if not a.no_decode:
            for key, chk in (("decode", True), ("decode_nodigest", False)):
                _, status, dst_st = eng.blob_decode(dst, blobs, idx, check_digest=chk, dst=back)
                assert dst_st["ok"] == n and dst_st["out_bytes"] == data, dst_st
                dec[key] = _median_s(lambda: eng.blob_decode(dst, blobs, idx, check_digest=chk, dst=back), a.reps)
        back.free()
        row = {"batch": name, "chunks": n, "bytes": data,
               "crc_device_GBps": data / t_crc / 1e9, "encode_GBps": data / t_enc / 1e9,
               "verify_device_GBps": data / t_ver / 1e9, "sha256_many_GBps": data / t_sha / 1e9,
               "verify_then_gather_GBps": data / t_cmp / 1e9,
               "ms": {"crc": t_crc * 1e3, "encode": t_enc * 1e3, "verify": t_ver * 1e3, "sha256_many": t_sha * 1e3,
                      "verify_then_gather": t_cmp * 1e3}}
        for key, t in dec.items():
            row[key + "_GBps"] = data / t / 1e9
            row["ms"][key] = t * 1e3
        rows.append(row)
        print(json.dumps(row), flush=True)
        dst.free()
        src.free()
    # host bytes: the CRC of the 4 MiB batch with the bytes on the host (pinned staging + H2D in the call)
    hb = int(a.host_gib * (1 << 30)) // (4 << 20) * (4 << 20)
    host = rng.integers(0, 256, hb, dtype=np.uint8)
    chunks = [(i * (4 << 20), 4 << 20) for i in range(hb // (4 << 20))]
    hsegs, hn = _segs(chunks)
    hout = np.zeros(hn, dtype=np.uint32)
    t_host = _median_s(lambda: _lib.check(L.pbsgpu_crc32_many_host(eng._h, host.ctypes.data, hb, hsegs, hn, hout.ctypes.data),
                                          "crc32_many_host"), max(1, a.reps // 2))
    h2d = eng.h2d_bandwidth(1 << 30)
    row = {"batch": "4MiB-host", "chunks": len(chunks), "bytes": hb, "crc_host_GBps": hb / t_host / 1e9, "h2d_GBps": h2d}
    rows.append(row)
    print(json.dumps(row), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
