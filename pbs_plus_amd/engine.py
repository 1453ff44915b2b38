"""Engine / PayloadStream / Chunker — thin object wrappers over the C ABI.

Device memory: ``Engine`` accepts raw device pointers (ints), anything exposing
``data_ptr()``/``numel()``/``element_size()`` (a CUDA/HIP torch tensor) or host
buffers (bytes / numpy); torch is plumbing only and is never imported here.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import RECORD_DTYPE, Segment, check
from .buzhash import Config


def _segs(segments):
    """[(offset, length)] or an (n, 2) uint64 array -> (pointer-compatible object, n).
    pbsgpu_segment is two little-endian u64, i.e. exactly one row of such an array."""
    if segments is None:
        return None, 0
    n = len(segments)
    if n == 0:
        return None, 0
    a = np.ascontiguousarray(segments, dtype=np.uint64).reshape(n, 2)
    return a.ctypes.data_as(C.POINTER(Segment)), n


def _host_view(data) -> np.ndarray:
    a = data if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _is_device_tensor(x) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda") and bool(x.is_cuda)


class DeviceBuffer:
    """Library-owned device allocation (for callers without torch)."""

    def __init__(self, eng: "Engine", nbytes: int):
        self._eng = eng
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(eng._L.pbsgpu_device_alloc(eng._h, self.nbytes, C.byref(p)), "device_alloc")
        self.ptr = p.value

    def free(self):
        if self.ptr:
            check(self._eng._L.pbsgpu_device_free(self._eng._h, self.ptr), "device_free")
            self.ptr = None

    def upload(self, data, offset: int = 0):
        a = _host_view(data)
        assert offset + a.size <= self.nbytes
        check(self._eng._L.pbsgpu_memcpy_h2d(self._eng._h, self.ptr + offset, a.ctypes.data, a.size), "memcpy_h2d")

    def download(self, offset: int = 0, nbytes: int | None = None) -> np.ndarray:
        n = self.nbytes - offset if nbytes is None else nbytes
        out = np.empty(n, dtype=np.uint8)
        check(self._eng._L.pbsgpu_memcpy_d2h(self._eng._h, out.ctypes.data, self.ptr + offset, n), "memcpy_d2h")
        return out


class Engine:
    """One engine per (process, GPU). Stands where backupproxy's session owns the
    chunker + hasher built from the buzhash.Config (commit_orchestrate.go:137-149)."""

    def __init__(self, config: Config, device: int = 0, inflight: int = 2, **options):
        """`options`: fields of pbsgpu_engine_options by name (sha_form=2, stream_ring_gib=8.0, zstd_seq_tables=1,
        zstd_window_log=17, ...); none = the defaults."""
        self._L = _lib.lib()
        self.config = config
        h = C.c_void_p()
        if options:
            o = _lib.EngineOptions()
            o.inflight = int(inflight)
            for k, v in options.items():
                setattr(o, k, v)
            check(self._L.pbsgpu_engine_create_opt(int(device), C.byref(config._c), C.byref(o), C.byref(h)), "engine_create_opt")
        else:
            check(self._L.pbsgpu_engine_create(int(device), C.byref(config._c), int(inflight), C.byref(h)),
                  "engine_create")
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._L.pbsgpu_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_suggested_feed(self, feed_bytes: int = 1, absolute_grid: bool = False) -> None:
        """Reader buffer size the suggested-boundary rule emulates (1 = byte-serial, 0 = everything at once)."""
        check(self._L.pbsgpu_engine_set_suggested_feed(self._h, int(feed_bytes), int(absolute_grid)), "set_suggested_feed")

    # ---- device memory helpers -------------------------------------------------------------
    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def fill(self, dptr: int, nbytes: int, seed: int, kind: int = 0, stream_off: int = 0) -> None:
        check(self._L.pbsgpu_fill_device(self._h, dptr, stream_off, nbytes, seed, kind), "fill_device")

    @staticmethod
    def _dev(data, nbytes=None):
        if isinstance(data, DeviceBuffer):
            return data.ptr, data.nbytes if nbytes is None else nbytes
        if _is_device_tensor(data):
            return data.data_ptr(), data.numel() * data.element_size() if nbytes is None else nbytes
        if isinstance(data, int):
            assert nbytes is not None
            return data, nbytes
        return None, None

    # ---- batch path ------------------------------------------------------------------------------
    def submit(self, data, segments=None, nbytes: int | None = None, suggested=None, id_key=None) -> int:
        """Enqueue cut + digest of every segment; returns a ticket. `suggested` = one ascending list of suggested
        boundaries per segment (relative to the segment start; payload-chunker rule, see pbsgpu.h). `id_key` = an IdKey of
        this engine: every record's digest is the keyed SHA-256(chunk || id_key) (pbsgpu_submit_*_keyed; not together with
        `suggested`); keep the key open until the ticket is collected."""
        segs, nseg = _segs(segments)
        t = C.c_uint64()
        ptr, n = self._dev(data, nbytes)
        if id_key is not None:
            if suggested is not None:
                raise ValueError("there is no keyed submit with suggested boundaries")
            if ptr is not None:
                check(self._L.pbsgpu_submit_device_keyed(self._h, id_key._h, ptr, n, segs, nseg, C.byref(t)), "submit_device_keyed")
            else:
                a = _host_view(data)
                check(self._L.pbsgpu_submit_host_keyed(self._h, id_key._h, a.ctypes.data, a.size, segs, nseg, C.byref(t)),
                      "submit_host_keyed")
            return t.value
        if suggested is not None:
            ns = max(nseg, 1)
            assert len(suggested) == ns, "one suggested-boundary list per segment"
            flat = (np.concatenate([np.asarray(x, dtype=np.uint64).reshape(-1) for x in suggested])
                    if ns else np.zeros(0, np.uint64))
            flat = np.ascontiguousarray(flat, dtype=np.uint64)
            idx = np.zeros(ns + 1, dtype=np.uint32)
            idx[1:] = np.cumsum([len(x) for x in suggested])
            fp = flat.ctypes.data if flat.size else None
            if ptr is not None:
                check(self._L.pbsgpu_submit_device_suggested(self._h, ptr, n, segs, nseg, fp, idx.ctypes.data,
                                                             C.byref(t)), "submit_device_suggested")
            else:
                a = _host_view(data)
                check(self._L.pbsgpu_submit_host_suggested(self._h, a.ctypes.data, a.size, segs, nseg, fp,
                                                           idx.ctypes.data, C.byref(t)), "submit_host_suggested")
            return t.value
        if ptr is not None:
            check(self._L.pbsgpu_submit_device(self._h, ptr, n, segs, nseg, C.byref(t)), "submit_device")
        else:
            a = _host_view(data)
            check(self._L.pbsgpu_submit_host(self._h, a.ctypes.data, a.size, segs, nseg, C.byref(t)), "submit_host")
        return t.value

    def h2d_bandwidth(self, nbytes: int = 1 << 30) -> float:
        """Measured pinned host -> device copy rate of this box in GB/s."""
        v = C.c_double()
        check(self._L.pbsgpu_measure_h2d(self._h, int(nbytes), C.byref(v)), "measure_h2d")
        return float(v.value)

    def wait(self, ticket: int) -> int:
        n = C.c_uint64()
        check(self._L.pbsgpu_wait(self._h, ticket, C.byref(n)), "wait")
        return n.value

    def done(self, ticket: int) -> bool:
        """Non-blocking: has everything enqueued for the ticket finished on the device?"""
        d = C.c_int(0)
        check(self._L.pbsgpu_ticket_done(self._h, int(ticket), C.byref(d)), "ticket_done")
        return bool(d.value)

    def timing(self, ticket: int) -> dict:
        t = _lib.Timing()
        check(self._L.pbsgpu_ticket_timing(self._h, ticket, C.byref(t)), "ticket_timing")
        return {k: getattr(t, k) for k, _ in _lib.Timing._fields_ if k != "reserved"}

    def collect(self, ticket: int) -> np.ndarray:
        n = self.wait(ticket)
        out = np.zeros(max(n, 1), dtype=RECORD_DTYPE)
        got = C.c_uint64()
        check(self._L.pbsgpu_collect(self._h, ticket, out.ctypes.data, n, C.byref(got)), "collect")
        return out[: got.value]

    def chunk_and_digest(self, data, segments=None, nbytes: int | None = None, suggested=None, id_key=None) -> np.ndarray:
        return self.collect(self.submit(data, segments, nbytes, suggested, id_key))

    def candidates(self, data, nbytes: int | None = None) -> np.ndarray:
        """Raw Buzhash candidates (ascending END offsets) of a device byte range."""
        ptr, n = self._dev(data, nbytes)
        assert ptr is not None, "candidates() wants device memory"
        cnt = C.c_uint64()
        st = self._L.pbsgpu_candidates_device(self._h, ptr, n, None, 0, C.byref(cnt))
        if st == _lib.OK and cnt.value == 0:
            return np.zeros(0, dtype=np.uint64)
        if st != _lib.E_CAPACITY:
            check(st, "candidates_device")
        out = np.empty(cnt.value, dtype=np.uint64)
        check(self._L.pbsgpu_candidates_device(self._h, ptr, n, out.ctypes.data, out.size, C.byref(cnt)),
              "candidates_device")
        return out[: cnt.value]

    def resolve_candidates(self, cands: np.ndarray, stream_len: int) -> np.ndarray:
        """Cut one stream from an explicit ascending candidate list (records without digests)."""
        c = np.ascontiguousarray(cands, dtype=np.uint64)
        n = C.c_uint64()
        st = self._L.pbsgpu_resolve_candidates(self._h, c.ctypes.data if c.size else None, c.size, stream_len, None, 0,
                                               C.byref(n))
        if st not in (_lib.OK, _lib.E_CAPACITY):
            check(st, "resolve_candidates")
        out = np.zeros(max(n.value, 1), dtype=RECORD_DTYPE)
        check(self._L.pbsgpu_resolve_candidates(self._h, c.ctypes.data if c.size else None, c.size, stream_len,
                                                out.ctypes.data, n.value, C.byref(n)), "resolve_candidates")
        return out[: n.value]

    # ---- whole-stream SHA-256 (verification.HashFile for many files) --------------------------------
    def sha256_many(self, data, segments, nbytes: int | None = None) -> np.ndarray:
        segs, nseg = _segs(segments)
        out = np.zeros((max(nseg, 1), 32), dtype=np.uint8)
        ptr, n = self._dev(data, nbytes)
        if ptr is not None:
            check(self._L.pbsgpu_sha256_many_device(self._h, ptr, n, segs, nseg, out.ctypes.data), "sha256_many_device")
        else:
            a = _host_view(data)
            check(self._L.pbsgpu_sha256_many_host(self._h, a.ctypes.data if a.size else None, a.size, segs, nseg,
                                                  out.ctypes.data), "sha256_many_host")
        return out[:nseg]

    def sha256_keyed_many(self, key: "IdKey", data, segments, nbytes: int | None = None) -> np.ndarray:
        """sha256_many() with an id key: row i = SHA-256(range i || id_key), the index digest of a chunk of an encrypted
        backup (pbsgpu_sha256_keyed_many_*). The key's engine does the work; a key of another engine is refused here."""
        if key._eng is not self:
            raise _lib.PbsGpuError(_lib.E_INVALID, "sha256_keyed_many: the key belongs to another engine")
        segs, nseg = _segs(segments)
        out = np.zeros((max(nseg, 1), 32), dtype=np.uint8)
        ptr, n = self._dev(data, nbytes)
        if ptr is not None:
            check(self._L.pbsgpu_sha256_keyed_many_device(key._h, ptr, n, segs, nseg, out.ctypes.data), "sha256_keyed_many_device")
        else:
            a = _host_view(data)
            check(self._L.pbsgpu_sha256_keyed_many_host(key._h, a.ctypes.data if a.size else None, a.size, segs, nseg,
                                                        out.ctypes.data), "sha256_keyed_many_host")
        return out[:nseg]

    # ---- whole-stream XXH3-64 (the xxh3.New() tee of writeBackedFile / verifyBackedFileHashes) -------
    def xxh3_many(self, data, segments, nbytes: int | None = None) -> np.ndarray:
        segs, nseg = _segs(segments)
        out = np.zeros(max(nseg, 1), dtype=np.uint64)
        ptr, n = self._dev(data, nbytes)
        if ptr is not None:
            check(self._L.pbsgpu_xxh3_many_device(self._h, ptr, n, segs, nseg, out.ctypes.data), "xxh3_many_device")
        else:
            a = _host_view(data)
            check(self._L.pbsgpu_xxh3_many_host(self._h, a.ctypes.data if a.size else None, a.size, segs, nseg,
                                                out.ctypes.data), "xxh3_many_host")
        return out[:nseg]

    def xxh64_many(self, data, segments, seed: int = 0, nbytes: int | None = None) -> np.ndarray:
        """XXH64 with `seed` of the ranges [(offset, length)] of the device buffer `data` (pbsgpu_xxh64_many_device): what
        a zstd frame's content checksum is the low 32 bits of. Ranges may be empty, unaligned and overlapping."""
        segs, nseg = _segs(segments)
        out = np.zeros(max(nseg, 1), dtype=np.uint64)
        ptr, n = self._dev(data, nbytes)
        assert ptr is not None, "xxh64_many() wants device memory"
        check(self._L.pbsgpu_xxh64_many_device(self._h, ptr, n, segs, nseg, int(seed), out.ctypes.data), "xxh64_many_device")
        return out[:nseg]

    # ---- CRC-32 and data blobs (the upload step and the chunk check of the read side) -------------------
    def crc32_many(self, data, segments, nbytes: int | None = None) -> np.ndarray:
        """CRC-32 (zlib's crc32) of every (offset, length) range of device or host bytes."""
        segs, nseg = _segs(segments)
        out = np.zeros(max(nseg, 1), dtype=np.uint32)
        ptr, n = self._dev(data, nbytes)
        if ptr is not None:
            check(self._L.pbsgpu_crc32_many_device(self._h, ptr, n, segs, nseg, out.ctypes.data), "crc32_many_device")
        else:
            a = _host_view(data)
            check(self._L.pbsgpu_crc32_many_host(self._h, a.ctypes.data if a.size else None, a.size, segs, nseg,
                                                 out.ctypes.data), "crc32_many_host")
        return out[:nseg]

    def blob_encode(self, src, chunks, nbytes: int | None = None):
        """Uncompressed data blobs of the device byte ranges `chunks` = [(offset, length)], laid out back to back in a new
        DeviceBuffer. Returns (buffer, offsets (n + 1, uint64: blob i = [offsets[i], offsets[i + 1])), CRCs (n, uint32))."""
        segs, n = _segs(chunks)
        sp, sn = self._dev(src, nbytes)
        assert sp is not None, "blob_encode() wants device memory"
        total = C.c_uint64()
        check(self._L.pbsgpu_blob_encoded_size(segs, n, C.byref(total)), "blob_encoded_size")
        dst = self.alloc(total.value)
        offs = np.zeros(n + 1, dtype=np.uint64)
        crcs = np.zeros(max(n, 1), dtype=np.uint32)
        try:
            check(self._L.pbsgpu_blob_encode_device(self._h, sp, sn, segs, n, dst.ptr, dst.nbytes, C.byref(total),
                                                    offs.ctypes.data, crcs.ctypes.data), "blob_encode_device")
        except Exception:
            dst.free()
            raise
        return dst, offs, crcs[:n]

    def blob_verify(self, data, blobs, digests=None, sizes=None, nbytes: int | None = None):
        """Check whole blobs [(offset, length)] of device or host bytes: magic, CRC and, for uncompressed blobs, the data
        length against `sizes` and its SHA-256 against `digests` ((n, 32) uint8; either may be None). Returns
        (status per blob, uint8 BLOB_* codes; stats dict with a count per status name and the byte totals)."""
        segs, n = _segs(blobs)
        status = np.zeros(max(n, 1), dtype=np.uint8)
        dg = None if digests is None else np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
        sz = None if sizes is None else np.ascontiguousarray(sizes, dtype=np.uint32).reshape(-1)
        assert dg is None or dg.shape[0] == n
        assert sz is None or sz.size == n
        dp = dg.ctypes.data if dg is not None and n else None
        zp = sz.ctypes.data if sz is not None and n else None
        st = _lib.BlobStats()
        ptr, nb = self._dev(data, nbytes)
        if ptr is not None:
            check(self._L.pbsgpu_blob_verify_device(self._h, ptr, nb, segs, n, dp, zp, status.ctypes.data, C.byref(st)),
                  "blob_verify_device")
        else:
            a = _host_view(data)
            check(self._L.pbsgpu_blob_verify_host(self._h, a.ctypes.data if a.size else None, a.size, segs, n, dp, zp,
                                                  status.ctypes.data, C.byref(st)), "blob_verify_host")
        stats = {name: int(st.count[k]) for k, name in enumerate(_lib.BLOB_STATUS_NAMES)}
        stats.update(blob_bytes=int(st.blob_bytes), crc_bytes=int(st.crc_bytes), sha_bytes=int(st.sha_bytes))
        return status[:n], stats

    def blob_decode(self, data, blobs, idx, blob_of=None, start=None, end=None, check_digest=True, dst=None,
                    nbytes: int | None = None):
        """The stream bytes [start, end) from a contiguous slice `idx` of an index (records as didx_decode returns them) and
        the blobs [(offset, length)] of the device buffer `data` (pbsgpu_blob_decode_device): blob_of[i] = the blob that
        carries entry i (None: blob i, see blob_index()); start / end default to the slice's span; dst None allocates
        end - start bytes. Returns (dst DeviceBuffer, status per entry as blob_verify() gives it for that blob with the
        entry's size and digest, stats dict: a count per status name, blob_bytes / crc_bytes / sha_bytes over the distinct
        referenced blobs, out_bytes). An entry whose blob is not an uncompressed one of its size leaves its part of dst as
        it was: read the status."""
        recs = np.ascontiguousarray(idx, dtype=RECORD_DTYPE).reshape(-1)
        n = int(recs.size)
        segs, nblob = _segs(blobs)
        bp, bn = self._dev(data, nbytes)
        assert bp is not None, "blob_decode() wants device memory"
        bo = None if blob_of is None else np.ascontiguousarray(blob_of, dtype=np.uint32).reshape(-1)
        assert bo is None or bo.size == n
        if start is None:
            start = int(recs["end"][0]) - int(recs["size"][0]) if n else 0
        if end is None:
            end = int(recs["end"][-1]) if n else start
        own = dst is None
        if own:
            dst = self.alloc(max(int(end) - int(start), 16))
        status = np.zeros(max(n, 1), dtype=np.uint8)
        st = _lib.DecodeStats()
        try:
            check(self._L.pbsgpu_blob_decode_device(self._h, bp, bn, segs, nblob, recs.ctypes.data if n else None, n,
                                                    bo.ctypes.data if bo is not None and n else None, int(start), int(end),
                                                    int(bool(check_digest)), dst.ptr, dst.nbytes, status.ctypes.data,
                                                    C.byref(st)), "blob_decode_device")
        except Exception:
            if own:
                dst.free()
            raise
        stats = {name: int(st.count[k]) for k, name in enumerate(_lib.BLOB_STATUS_NAMES)}
        stats.update(blob_bytes=int(st.blob_bytes), crc_bytes=int(st.crc_bytes), sha_bytes=int(st.sha_bytes),
                     out_bytes=int(st.out_bytes))
        return dst, status[:n], stats

    def blob_decode2(self, data, blobs, idx, blob_of=None, start=None, end=None, check_digest=True, dst=None,
                     nbytes: int | None = None, zstd=True):
        """blob_decode() with the zstd-compressed blobs decoded on the device (pbsgpu_blob_decode2_device): with zstd=True a
        compressed blob whose CRC is good is decoded to its entries' places, checked for the entry's size and, with
        check_digest, for the SHA-256 of the DECODED bytes; status 6 (bad_data) is a malformed or unsupported frame, and 5
        (crc_only) then means encrypted only. zstd=False gives blob_decode()'s outputs exactly. The stats dict has a count
        per status name ("bad_data" included) and zstd_in_bytes / zstd_out_bytes beside blob_decode()'s byte counts."""
        recs = np.ascontiguousarray(idx, dtype=RECORD_DTYPE).reshape(-1)
        n = int(recs.size)
        segs, nblob = _segs(blobs)
        bp, bn = self._dev(data, nbytes)
        assert bp is not None, "blob_decode2() wants device memory"
        bo = None if blob_of is None else np.ascontiguousarray(blob_of, dtype=np.uint32).reshape(-1)
        assert bo is None or bo.size == n
        if start is None:
            start = int(recs["end"][0]) - int(recs["size"][0]) if n else 0
        if end is None:
            end = int(recs["end"][-1]) if n else start
        own = dst is None
        if own:
            dst = self.alloc(max(int(end) - int(start), 16))
        status = np.zeros(max(n, 1), dtype=np.uint8)
        st = _lib.DecodeStats2()
        flags = (_lib.DECODE_F_DIGEST if check_digest else 0) | (_lib.DECODE_F_ZSTD if zstd else 0)
        try:
            check(self._L.pbsgpu_blob_decode2_device(self._h, bp, bn, segs, nblob, recs.ctypes.data if n else None, n,
                                                     bo.ctypes.data if bo is not None and n else None, int(start), int(end),
                                                     flags, dst.ptr, dst.nbytes, status.ctypes.data, C.byref(st)),
                  "blob_decode2_device")
        except Exception:
            if own:
                dst.free()
            raise
        stats = {name: int(st.count[k]) for k, name in enumerate(_lib.BLOB_STATUS_NAMES2)}
        stats.update(blob_bytes=int(st.blob_bytes), crc_bytes=int(st.crc_bytes), sha_bytes=int(st.sha_bytes),
                     out_bytes=int(st.out_bytes), zstd_in_bytes=int(st.zstd_in_bytes), zstd_out_bytes=int(st.zstd_out_bytes))
        return dst, status[:n], stats

    def blob_decode4(self, data, blobs, idx, blob_of=None, start=None, end=None, check_digest=True, dst=None,
                     nbytes: int | None = None, zstd=True, key=None, aes=None, id_key=None):
        """blob_decode3() with the keyed digest check (pbsgpu_blob_decode4_device): with aes, check_digest and `id_key`, an
        IdKey of this engine, an entry of an encrypted kind that passed tag, frame and size is checked against
        SHA-256(plaintext || id_key) and gets status 3 (bad_digest) on a mismatch; its bytes stay restored. Entries of the
        plain kinds keep the plain digest. sha_bytes counts the plaintext of each distinct encrypted blob once. With
        id_key=None every output is blob_decode3()'s."""
        return self.blob_decode3(data, blobs, idx, blob_of, start, end, check_digest, dst, nbytes, zstd, key, aes,
                                 _id_key=id_key, _four=True)

    def blob_decode3(self, data, blobs, idx, blob_of=None, start=None, end=None, check_digest=True, dst=None,
                     nbytes: int | None = None, zstd=True, key=None, aes=None, _id_key=None, _four=False):
        """blob_decode2() with the encrypted blobs decrypted on the device under `key`, an AesKey of this engine
        (pbsgpu_blob_decode3_device). aes defaults to "a key was given"; aes=True without a key raises PbsGpuError
        (E_INVALID). An encrypted blob whose CRC is good is decrypted to its entries' places; an encrypted-compressed one is
        then decoded as a frame if zstd is set, and stays 5 (crc_only) if not. Status 7 (bad_tag): a wrong key or a damaged
        blob, the entry's part of dst is zero where the blob was decrypted in place and untouched otherwise. check_digest is
        not applied to encrypted entries. Without aes every output is blob_decode2()'s. The stats dict has a count per status
        name ("bad_tag" included) and aes_bytes beside blob_decode2()'s byte counts."""
        recs = np.ascontiguousarray(idx, dtype=RECORD_DTYPE).reshape(-1)
        n = int(recs.size)
        segs, nblob = _segs(blobs)
        bp, bn = self._dev(data, nbytes)
        assert bp is not None, "blob_decode3() wants device memory"
        bo = None if blob_of is None else np.ascontiguousarray(blob_of, dtype=np.uint32).reshape(-1)
        assert bo is None or bo.size == n
        if start is None:
            start = int(recs["end"][0]) - int(recs["size"][0]) if n else 0
        if end is None:
            end = int(recs["end"][-1]) if n else start
        own = dst is None
        if own:
            dst = self.alloc(max(int(end) - int(start), 16))
        status = np.zeros(max(n, 1), dtype=np.uint8)
        st = _lib.DecodeStats3()
        if aes is None:
            aes = key is not None
        flags = (_lib.DECODE_F_DIGEST if check_digest else 0) | (_lib.DECODE_F_ZSTD if zstd else 0) | (_lib.DECODE_F_AES if aes else 0)
        try:
            if _four:
                check(self._L.pbsgpu_blob_decode4_device(self._h, bp, bn, segs, nblob, recs.ctypes.data if n else None, n,
                                                         bo.ctypes.data if bo is not None and n else None, int(start), int(end),
                                                         flags, key._h if key is not None else None,
                                                         _id_key._h if _id_key is not None else None, dst.ptr, dst.nbytes,
                                                         status.ctypes.data, C.byref(st)),
                      "blob_decode4_device")
            else:
                check(self._L.pbsgpu_blob_decode3_device(self._h, bp, bn, segs, nblob, recs.ctypes.data if n else None, n,
                                                         bo.ctypes.data if bo is not None and n else None, int(start), int(end),
                                                         flags, key._h if key is not None else None, dst.ptr, dst.nbytes,
                                                         status.ctypes.data, C.byref(st)),
                      "blob_decode3_device")
        except Exception:
            if own:
                dst.free()
            raise
        stats = {name: int(st.count[k]) for k, name in enumerate(_lib.BLOB_STATUS_NAMES3)}
        stats.update(blob_bytes=int(st.blob_bytes), crc_bytes=int(st.crc_bytes), sha_bytes=int(st.sha_bytes),
                     out_bytes=int(st.out_bytes), zstd_in_bytes=int(st.zstd_in_bytes), zstd_out_bytes=int(st.zstd_out_bytes),
                     aes_bytes=int(st.aes_bytes))
        return dst, status[:n], stats

    def zstd_decode2(self, data, frames, out=None, dst=None, nbytes: int | None = None, checksum=False, stream=False):
        """zstd_decode() with flags (pbsgpu_zstd_decode2_device). checksum=True: a frame that carries a content checksum
        is checked against it, a mismatch is status 4 (_lib.ZSTD_BAD_CHECKSUM) with 0 bytes decoded. stream=True: every
        segment is a whole zstd stream (frames one behind the other, skippable frames skipped, an empty segment is ok
        with 0 bytes), decoded as ZSTD_decompress does it; `out` must then be given (zstd_stream_info() sizes a stream
        on the host). With neither it is zstd_decode(), output for output."""
        flags = (_lib.ZSTD_F_CHECKSUM if checksum else 0) | (_lib.ZSTD_F_STREAM if stream else 0)
        if stream and out is None:
            raise ValueError("stream=True: pass out= (zstd_stream_info() gives a stream's content size)")
        return self._zstd_decode(data, frames, out, dst, nbytes, flags)

    def zstd_decode(self, data, frames, out=None, dst=None, nbytes: int | None = None):
        """Decode the zstd frames [(offset, length)] of the device buffer `data` in one launch (pbsgpu_zstd_decode_device):
        frame i goes to dst at out[i] = (offset, room). out None lays the frames out back to back by the content size
        their headers declare (read back from the device; a frame that declares none is a ValueError); dst None allocates
        what `out` needs. Returns (dst, status per frame: 0 ok, 1 bad frame, 2 bad size, 3 unsupported, bytes decoded per
        frame, out as an (n, 2) array). On a status other than 0 the frame's own room holds unspecified bytes."""
        return self._zstd_decode(data, frames, out, dst, nbytes, None)

    def _zstd_decode(self, data, frames, out, dst, nbytes, flags):  # flags None: the call without flags
        dp, dn = self._dev(data, nbytes)
        assert dp is not None, "zstd_decode() wants device memory"
        fr = np.ascontiguousarray(frames, dtype=np.uint64).reshape(-1, 2)
        n = int(fr.shape[0])
        if out is None:
            rooms = np.zeros(n, dtype=np.uint64)
            if n:  # the first 18 bytes of every frame (the longest header), gathered on the device and read back in one copy
                take = np.minimum(fr[:, 1], 18)
                items = np.stack([fr[:, 0], np.arange(n, dtype=np.uint64) * 18, take], axis=1)
                heads = self.alloc(18 * n)
                try:
                    check(self._L.pbsgpu_gather_device(self._h, dp, dn, heads.ptr, heads.nbytes, items.ctypes.data, n),
                          "gather_device")
                    host = heads.download()
                finally:
                    heads.free()
            for i in range(n):
                info = zstd_frame_info(host[18 * i:18 * i + int(take[i])])
                if info["status"] == 0 and info["content_size"] is None:
                    raise ValueError(f"frame {i} declares no content size: pass out=")
                rooms[i] = info["content_size"] if info["status"] == 0 else 0
            ends = np.cumsum(rooms)
            out = np.stack([ends - rooms, rooms], axis=1)
        oa = np.ascontiguousarray(out, dtype=np.uint64).reshape(-1, 2)
        assert oa.shape[0] == n, "one (offset, room) per frame"
        own = dst is None
        if own:
            dst = self.alloc(max(int((oa[:, 0] + oa[:, 1]).max()) if n else 0, 16))
        status = np.zeros(max(n, 1), dtype=np.uint8)
        decoded = np.zeros(max(n, 1), dtype=np.uint64)
        try:
            args = (self._h, dp, dn, fr.ctypes.data if n else None, n, oa.ctypes.data if n else None, dst.ptr, dst.nbytes,
                    status.ctypes.data, decoded.ctypes.data)
            if flags is None:
                check(self._L.pbsgpu_zstd_decode_device(*args), "zstd_decode_device")
            else:
                check(self._L.pbsgpu_zstd_decode2_device(*args, flags), "zstd_decode2_device")
        except Exception:
            if own:
                dst.free()
            raise
        return dst, status[:n], decoded[:n], oa

    def aes_gcm_many(self, key, data, messages, ivs, tags=None, out=None, dst=None, nbytes: int | None = None, encrypt=False):
        """AES-256-GCM (empty AAD, 16-byte tags) over the messages [(offset, length)] of the device buffer `data` in one
        call (pbsgpu_aes_gcm_many_device) under `key`, an AesKey of this engine. ivs: one IV of 12 or 16 bytes per message
        (bytes each, or an (n, iv_len) uint8 array). Decrypting wants tags, an (n, 16) uint8 array; encrypt=True returns
        them. Message i goes to dst at out[i] = (offset, room >= length); out None lays the messages out back to back,
        dst None allocates what `out` needs. Returns (dst, status per message: 0 ok, 1 bad tag, tags as an (n, 16) array,
        out as an (n, 2) array). A message whose tag is bad has its output zeroed."""
        dp, dn = self._dev(data, nbytes)
        assert dp is not None, "aes_gcm_many() wants device memory"
        ms = np.ascontiguousarray(messages, dtype=np.uint64).reshape(-1, 2)
        n = int(ms.shape[0])
        def flat(items):  # an array as it is, else one bytes-like per message
            if isinstance(items, np.ndarray):
                return np.ascontiguousarray(items, dtype=np.uint8).reshape(-1)
            return np.frombuffer(b"".join(bytes(v) for v in items), dtype=np.uint8)

        iva = flat(ivs) if n else np.zeros(0, np.uint8)
        iv_len = iva.size // n if n else 16
        if n and (iva.size != n * iv_len or iv_len not in (12, 16)):
            raise ValueError("one IV of 12 or 16 bytes per message, all of one length")
        if encrypt:
            ta = np.zeros((max(n, 1), 16), dtype=np.uint8)
        else:
            if tags is None:
                raise ValueError("decrypting wants tags=")
            ta = flat(tags).reshape(-1, 16).copy()
            assert ta.shape[0] == n, "one 16-byte tag per message"
            if n == 0:
                ta = np.zeros((1, 16), dtype=np.uint8)
        if out is None:
            ends = np.cumsum(ms[:, 1])
            out = np.stack([ends - ms[:, 1], ms[:, 1]], axis=1)
        oa = np.ascontiguousarray(out, dtype=np.uint64).reshape(-1, 2)
        assert oa.shape[0] == n, "one (offset, room) per message"
        own = dst is None
        if own:
            dst = self.alloc(max(int((oa[:, 0] + oa[:, 1]).max()) if n else 0, 16))
        status = np.zeros(max(n, 1), dtype=np.uint8)
        try:
            check(self._L.pbsgpu_aes_gcm_many_device(key._h, dp, dn, ms.ctypes.data if n else None, n, iva.ctypes.data if n else None,
                                                     iv_len, ta.ctypes.data, oa.ctypes.data if n else None, dst.ptr, dst.nbytes,
                                                     status.ctypes.data, _lib.AES_F_ENCRYPT if encrypt else 0),
                  "aes_gcm_many_device")
        except Exception:
            if own:
                dst.free()
            raise
        return dst, status[:n], ta[:n], oa

    def zstd_encode2(self, data, chunks, out=None, dst=None, nbytes: int | None = None, checksum=False):
        """zstd_encode() with flags (pbsgpu_zstd_encode2_device). checksum=True: every frame carries the content checksum
        (the flag in its header, the low 32 bits of XXH64(content, 0) behind its last block: 4 bytes more); out None then
        lays out rooms of zstd_encode_bound2(length, checksum=True). Without it it is zstd_encode()."""
        return self._zstd_encode(data, chunks, out, dst, nbytes, _lib.ZSTD_F_CHECKSUM if checksum else 0)

    def zstd_encode(self, data, chunks, out=None, dst=None, nbytes: int | None = None):
        """Compress the chunks [(offset, length)] of the device buffer `data` to one zstd frame each in one call
        (pbsgpu_zstd_encode_device): frame i goes to dst at out[i] = (offset, room). out None lays rooms of
        zstd_encode_bound(length) out back to back; dst None allocates what `out` needs. Returns (dst, status per chunk:
        0 ok, 2 the room is too small, frame length per chunk (0 unless ok), out as an (n, 2) array)."""
        return self._zstd_encode(data, chunks, out, dst, nbytes, None)

    def _zstd_encode(self, data, chunks, out, dst, nbytes, flags):  # flags None: the call without flags
        dp, dn = self._dev(data, nbytes)
        assert dp is not None, "zstd_encode() wants device memory"
        ch = np.ascontiguousarray(chunks, dtype=np.uint64).reshape(-1, 2)
        n = int(ch.shape[0])
        if out is None:
            rooms = np.array([zstd_encode_bound2(int(v), bool(flags)) for v in ch[:, 1]], dtype=np.uint64)
            ends = np.cumsum(rooms)
            out = np.stack([ends - rooms, rooms], axis=1)
        oa = np.ascontiguousarray(out, dtype=np.uint64).reshape(-1, 2)
        assert oa.shape[0] == n, "one (offset, room) per chunk"
        own = dst is None
        if own:
            dst = self.alloc(max(int((oa[:, 0] + oa[:, 1]).max()) if n else 0, 16))
        status = np.zeros(max(n, 1), dtype=np.uint8)
        flen = np.zeros(max(n, 1), dtype=np.uint64)
        try:
            args = (self._h, dp, dn, ch.ctypes.data if n else None, n, oa.ctypes.data if n else None, dst.ptr, dst.nbytes,
                    status.ctypes.data, flen.ctypes.data)
            if flags is None:
                check(self._L.pbsgpu_zstd_encode_device(*args), "zstd_encode_device")
            else:
                check(self._L.pbsgpu_zstd_encode2_device(*args, flags), "zstd_encode2_device")
        except Exception:
            if own:
                dst.free()
            raise
        return dst, status[:n], flen[:n], oa

    def blob_encode2(self, src, chunks, dst=None, nbytes: int | None = None, zstd=True):
        """blob_encode() with the blob's kind decided on the device (pbsgpu_blob_encode2_device): with zstd=True a chunk whose
        zstd frame is strictly shorter than the chunk becomes a compressed blob, every other one the uncompressed blob
        blob_encode() writes. Blob i lies at offsets[i] and is lens[i] long; the slots [offsets[i], offsets[i + 1]) are
        those of the uncompressed layout and are not compacted. zstd=False gives blob_encode()'s outputs exactly.
        Returns (buffer, offsets (n + 1), lens (n), kinds (n: 0 uncompressed, 1 compressed), CRCs (n), stats dict)."""
        segs, n = _segs(chunks)
        sp, sn = self._dev(src, nbytes)
        assert sp is not None, "blob_encode2() wants device memory"
        own = dst is None
        if own:
            total = C.c_uint64()
            check(self._L.pbsgpu_blob_encoded_size(segs, n, C.byref(total)), "blob_encoded_size")
            dst = self.alloc(max(total.value, 16))
        offs = np.zeros(n + 1, dtype=np.uint64)
        lens = np.zeros(max(n, 1), dtype=np.uint32)
        kinds = np.zeros(max(n, 1), dtype=np.uint8)
        crcs = np.zeros(max(n, 1), dtype=np.uint32)
        st = _lib.EncodeStats()
        try:
            check(self._L.pbsgpu_blob_encode2_device(self._h, sp, sn, segs, n, _lib.ENCODE_F_ZSTD if zstd else 0, dst.ptr,
                                                     dst.nbytes, offs.ctypes.data, lens.ctypes.data, kinds.ctypes.data,
                                                     crcs.ctypes.data, C.byref(st)), "blob_encode2_device")
        except Exception:
            if own:
                dst.free()
            raise
        return dst, offs, lens[:n], kinds[:n], crcs[:n], _encode_stats(st)

    def blob_encode3(self, src, chunks, key=None, ivs=None, dst=None, nbytes: int | None = None, zstd=True, aes=None):
        """blob_encode2() with the blobs encrypted on the device under `key`, an AesKey of this engine
        (pbsgpu_blob_encode3_device). aes defaults to "a key was given"; aes=True without a key raises PbsGpuError
        (E_INVALID). With aes, blob i lies in the slot [offsets[i], offsets[i] + 44 + length): magic, CRC of the ciphertext,
        IV, tag, ciphertext; kind 2 (encrypted) holds the chunk, kind 3 (encrypted-compressed, zstd=True and the frame
        strictly shorter than the chunk) its frame. ivs: one 16-byte IV per chunk (bytes each, or an (n, 16) uint8 array);
        None draws os.urandom(16 * n). Two equal IVs in one call are refused; uniqueness across calls under one key is the
        caller's. Without aes every output is blob_encode2()'s and the IVs come back empty.
        Returns (buffer, offsets (n + 1), lens (n), kinds (n), CRCs (n), stats dict with aes_bytes, IVs used as (n, 16))."""
        segs, n = _segs(chunks)
        sp, sn = self._dev(src, nbytes)
        assert sp is not None, "blob_encode3() wants device memory"
        if aes is None:
            aes = key is not None
        flags = (_lib.ENCODE_F_ZSTD if zstd else 0) | (_lib.ENCODE_F_AES if aes else 0)
        if not aes:
            iva = np.zeros((0, 16), dtype=np.uint8)
        elif ivs is None:
            iva = np.frombuffer(os.urandom(16 * n), dtype=np.uint8).reshape(n, 16).copy()
        elif isinstance(ivs, np.ndarray):
            iva = np.ascontiguousarray(ivs, dtype=np.uint8).reshape(-1, 16)
        else:
            iva = np.frombuffer(b"".join(bytes(v) for v in ivs), dtype=np.uint8).reshape(-1, 16).copy()
        if aes and iva.shape[0] != n:
            raise ValueError("one 16-byte IV per chunk")
        own = dst is None
        if own:
            total = C.c_uint64()
            check(self._L.pbsgpu_blob_encoded_size3(segs, n, flags, C.byref(total)), "blob_encoded_size3")
            dst = self.alloc(max(total.value, 16))
        offs = np.zeros(n + 1, dtype=np.uint64)
        lens = np.zeros(max(n, 1), dtype=np.uint32)
        kinds = np.zeros(max(n, 1), dtype=np.uint8)
        crcs = np.zeros(max(n, 1), dtype=np.uint32)
        st = _lib.EncodeStats3()
        try:
            check(self._L.pbsgpu_blob_encode3_device(self._h, sp, sn, segs, n, flags, key._h if key is not None else None,
                                                     iva.ctypes.data if aes and n else None, dst.ptr, dst.nbytes,
                                                     offs.ctypes.data, lens.ctypes.data, kinds.ctypes.data, crcs.ctypes.data,
                                                     C.byref(st)), "blob_encode3_device")
        except Exception:
            if own:
                dst.free()
            raise
        stats = _encode_stats(st)
        stats["aes_bytes"] = int(st.aes_bytes)
        return dst, offs, lens[:n], kinds[:n], crcs[:n], stats, iva

    # ---- payload-stream assembly (.ppxar layout: markers + 16-byte headers + file bodies) ----------
    def payload_pack(self, src, files, dst, with_start: bool = True, with_tail: bool = True):
        """Lay the file bodies `files` = [(offset, length)] of device buffer `src` out as the pxar
        payload stream in device buffer `dst`. Returns (stream length, payload offset of every file's header)."""
        fmt = _lib.PayloadFormat()
        check(self._L.pbsgpu_payload_format_default(C.byref(fmt)), "payload_format_default")
        fmt.with_start, fmt.with_tail = int(with_start), int(with_tail)
        segs, n = _segs(files)
        sp, sn = self._dev(src)
        dp, dn = self._dev(dst)
        out_len = C.c_uint64()
        offs = np.zeros(max(n, 1), dtype=np.uint64)
        check(self._L.pbsgpu_payload_pack_device(self._h, sp, sn, segs, n, C.byref(fmt), dp, dn, C.byref(out_len),
                                                 offs.ctypes.data), "payload_pack_device")
        return out_len.value, offs[:n]

    def gather(self, src, dst, items) -> None:
        """Piece-table copy on the device: items = (n, 3) uint64 rows (src_off, dst_off, len)."""
        a = np.ascontiguousarray(items, dtype=np.uint64).reshape(-1, 3)
        sp, sn = self._dev(src)
        dp, dn = self._dev(dst)
        check(self._L.pbsgpu_gather_device(self._h, sp, sn, dp, dn, a.ctypes.data if a.size else None, a.shape[0]),
              "gather_device")

    # ---- digest set ------------------------------------------------------------------------------------
    def dedup(self, records: np.ndarray):
        """(dup flags, stats) — dup[i] = 1 when an earlier record has the same digest."""
        recs = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        dup = np.zeros(max(recs.size, 1), dtype=np.uint8)
        st = _lib.DedupStats()
        check(self._L.pbsgpu_dedup_host(self._h, recs.ctypes.data if recs.size else None, recs.size, dup.ctypes.data,
                                        C.byref(st)), "dedup_host")
        return dup[: recs.size], {k: getattr(st, k) for k, _ in _lib.DedupStats._fields_}

    def dedup_device(self, dptr: int, n: int, want_flags: bool = True):
        """dedup() on n records that already are in device memory (e.g. an RCCL all-gather's output)."""
        dup = np.zeros(max(n, 1), dtype=np.uint8) if want_flags else None
        st = _lib.DedupStats()
        check(self._L.pbsgpu_dedup_device(self._h, dptr, n, dup.ctypes.data if want_flags else None, C.byref(st)),
              "dedup_device")
        return (dup[:n] if want_flags else None), {k: getattr(st, k) for k, _ in _lib.DedupStats._fields_}

    # ---- dynamic index ------------------------------------------------------------------------------
    def didx_encode(self, records: np.ndarray, uuid: bytes = b"\0" * 16, ctime: int = 0) -> bytes:
        recs = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        nb = C.c_uint64()
        check(self._L.pbsgpu_didx_size(recs.size, C.byref(nb)), "didx_size")
        out = np.zeros(nb.value, dtype=np.uint8)
        u = (C.c_uint8 * 16).from_buffer_copy(uuid)
        check(self._L.pbsgpu_didx_encode(self._h, recs.ctypes.data if recs.size else None, recs.size, u, ctime,
                                         out.ctypes.data, out.size), "didx_encode")
        return out.tobytes()


def didx_decode(blob: bytes):
    """(records, ctime, index_csum) from a .didx image."""
    L = _lib.lib()
    a = np.frombuffer(blob, dtype=np.uint8)
    n = C.c_uint64()
    ct = C.c_int64()
    cs = (C.c_uint8 * 32)()
    st = L.pbsgpu_didx_decode(a.ctypes.data, a.size, None, 0, C.byref(n), C.byref(ct), cs)
    if st not in (_lib.OK, _lib.E_CAPACITY):
        check(st, "didx_decode")
    out = np.zeros(max(n.value, 1), dtype=RECORD_DTYPE)
    check(L.pbsgpu_didx_decode(a.ctypes.data, a.size, out.ctypes.data, n.value, C.byref(n), C.byref(ct), cs),
          "didx_decode")
    return out[: n.value], ct.value, bytes(cs)


def blob_magic(kind: int) -> bytes:
    """The 8-byte magic of a data blob kind (_lib.BLOB_UNCOMPRESSED ... BLOB_ENCRYPTED_COMPRESSED)."""
    out = (C.c_uint8 * 8)()
    check(_lib.lib().pbsgpu_blob_magic(int(kind), out), "blob_magic")
    return bytes(out)


def _encode_stats(st) -> dict:
    return dict(blobs=[int(v) for v in st.blobs], blob_bytes=[int(v) for v in st.blob_bytes],
                chunk_bytes=[int(v) for v in st.chunk_bytes], frame_bytes=int(st.frame_bytes), crc_bytes=int(st.crc_bytes))


class _Upload2Out:
    """the host outputs of the two upload_new2 calls"""

    def __init__(self, n):
        self.n = n
        self.flags = np.zeros(max(n, 1), dtype=np.uint8)
        self.offs = np.zeros(max(n, 1), dtype=np.uint64)
        self.lens = np.zeros(max(n, 1), dtype=np.uint32)
        self.kinds = np.zeros(max(n, 1), dtype=np.uint8)
        self.crcs = np.zeros(max(n, 1), dtype=np.uint32)
        self.used, self.st, self.enc = C.c_uint64(), _lib.DedupStats(), _lib.EncodeStats()

    def args(self):
        return (self.flags.ctypes.data, self.offs.ctypes.data, self.lens.ctypes.data, self.kinds.ctypes.data,
                self.crcs.ctypes.data, C.byref(self.used), C.byref(self.st), C.byref(self.enc))

    def result(self, dst):
        n = self.n
        dst.used = int(self.used.value)
        return (dst, self.flags[:n], self.offs[:n], self.lens[:n], self.kinds[:n], self.crcs[:n],
                {k: getattr(self.st, k) for k, _ in _lib.DedupStats._fields_}, _encode_stats(self.enc))


def zstd_encode_bound(n: int) -> int:
    """No zstd frame Engine.zstd_encode() writes for n bytes of content is longer (pbsgpu_zstd_encode_bound, host only)."""
    return int(_lib.lib().pbsgpu_zstd_encode_bound(int(n)))


def zstd_encode_bound2(n: int, checksum: bool = False) -> int:
    """zstd_encode_bound() for Engine.zstd_encode2(): 4 bytes more with checksum (pbsgpu_zstd_encode_bound2, host only)."""
    return int(_lib.lib().pbsgpu_zstd_encode_bound2(int(n), _lib.ZSTD_F_CHECKSUM if checksum else 0))


def zstd_stream_info(stream) -> dict:
    """What the headers of a whole zstd stream declare (pbsgpu_zstd_stream_info, host only): status as the headers alone
    decide it, content_size (the sum over the frames; None if a frame declares none), frames, skippable, any_checksum.
    What a caller sizes the destination of Engine.zstd_decode2(stream=True) with."""
    a = _host_view(stream)
    size = C.c_uint64(0)
    nf, ns = C.c_uint32(0), C.c_uint32(0)
    ck = C.c_int(0)
    st = _lib.lib().pbsgpu_zstd_stream_info(a.ctypes.data if a.size else None, a.size, C.byref(size), C.byref(nf), C.byref(ns),
                                            C.byref(ck))
    if st < 0:
        raise _lib.PbsGpuError(st, "zstd_stream_info")
    return dict(status=int(st), content_size=None if size.value == 2**64 - 1 else int(size.value), frames=int(nf.value),
                skippable=int(ns.value), any_checksum=bool(ck.value))


def zstd_frame_info(frame) -> dict:
    """What the header of one zstd frame declares (pbsgpu_zstd_frame_info, host only): status (0 ok, 1 bad frame,
    3 unsupported), content_size (None when the frame declares none), window_size, header_bytes, has_checksum."""
    a = _host_view(frame)
    size, window, hb, ck = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_int()
    st = _lib.lib().pbsgpu_zstd_frame_info(a.ctypes.data if a.size else None, a.size, C.byref(size), C.byref(window), C.byref(hb),
                                           C.byref(ck))
    if st < 0:
        raise _lib.PbsGpuError(st, "zstd_frame_info")
    return {"status": st, "content_size": None if size.value == (1 << 64) - 1 else size.value, "window_size": window.value,
            "header_bytes": hb.value, "has_checksum": bool(ck.value)}


def blob_index(blob_digests, idx) -> np.ndarray:
    """blob_of for Engine.blob_decode by digest: blob_digests is an (nblob, 32) uint8 array (blob b carries the chunk
    with that SHA-256; of equal digests the first is taken), idx the index entries. KeyError on an entry whose digest no
    blob carries."""
    dg = np.ascontiguousarray(blob_digests, dtype=np.uint8).reshape(-1, 32)
    recs = np.ascontiguousarray(idx, dtype=RECORD_DTYPE).reshape(-1)
    where = {}
    for b in range(dg.shape[0]):
        where.setdefault(dg[b].tobytes(), b)
    out = np.empty(recs.size, dtype=np.uint32)
    want = np.ascontiguousarray(recs["digest"])
    for i in range(recs.size):
        key = want[i].tobytes()
        if key not in where:
            raise KeyError("entry %d: no blob carries digest %s" % (i, key.hex()))
        out[i] = where[key]
    return out


def crc32_combine(crc_a: int, crc_b: int, len_b: int) -> int:
    """zlib.crc32(A + B) from zlib.crc32(A), zlib.crc32(B) and len(B)."""
    out = C.c_uint32()
    check(_lib.lib().pbsgpu_crc32_combine(int(crc_a), int(crc_b), int(len_b), C.byref(out)), "crc32_combine")
    return int(out.value)


def chunk_ranges(records: np.ndarray, segments=None, known=None) -> np.ndarray:
    """(n, 2) uint64 (offset, length) of each record's chunk in the submitted buffer: a record's `end` is relative to its
    segment, so the chunk is [segments[segment].offset + end - size, + size). segments = None: one segment at offset 0.
    known (flags of KnownChunks.classify / Engine.dedup) keeps only the records flagged 0 — the chunks to upload."""
    recs = np.asarray(records, dtype=RECORD_DTYPE).reshape(-1)
    if known is not None:
        recs = recs[np.asarray(known).reshape(-1)[: recs.size] == 0]
    if segments is None or len(segments) == 0:
        base = np.zeros(recs.size, dtype=np.uint64)
    else:
        segs = np.ascontiguousarray(segments, dtype=np.uint64).reshape(-1, 2)
        base = segs[recs["segment"].astype(np.int64), 0]
    out = np.empty((recs.size, 2), dtype=np.uint64)
    size = recs["size"].astype(np.uint64)
    out[:, 0] = base + recs["end"] - size
    out[:, 1] = size
    return out


class AesKey:
    """An AES-256 key on the device (pbsgpu_aes_key_*): its round keys, hash key and multiplier tables, for
    Engine.aes_gcm_many. The 32 key bytes are expanded once and not kept on the host; close() zeroes the device copy. The
    key keeps its engine alive."""

    def __init__(self, eng: "Engine", key: bytes):
        if len(key) != 32:
            raise ValueError("an AES-256 key is 32 bytes")
        self._eng = eng
        self._L = eng._L
        h = C.c_void_p()
        buf = (C.c_uint8 * 32).from_buffer_copy(bytes(key))
        try:
            check(self._L.pbsgpu_aes_key_create(eng._h, buf, C.byref(h)), "aes_key_create")
        finally:
            C.memset(buf, 0, 32)
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.pbsgpu_aes_key_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __repr__(self):  # (never the key)
        return "AesKey(<32 bytes>)"


class IdKey:
    """The 32-byte id key of keyed chunk digests on the device (pbsgpu_id_key_*), for Engine.sha256_keyed_many,
    Engine.chunk_and_digest(id_key=) and Engine.blob_decode4(id_key=): SHA-256(content || id_key) is what an encrypted
    backup's index calls a chunk. The bytes are not kept on the host; close() zeroes the device copy. The key keeps its engine
    alive. Nothing is derived here: the caller brings the 32 bytes."""

    def __init__(self, eng: "Engine", id_key: bytes):
        if len(id_key) != 32:
            raise ValueError("an id key is 32 bytes")
        self._eng = eng
        self._L = eng._L
        h = C.c_void_p()
        buf = (C.c_uint8 * 32).from_buffer_copy(bytes(id_key))
        try:
            check(self._L.pbsgpu_id_key_create(eng._h, buf, C.byref(h)), "id_key_create")
        finally:
            C.memset(buf, 0, 32)
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.pbsgpu_id_key_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __repr__(self):  # (never the key)
        return "IdKey(<32 bytes>)"


class KnownChunks:
    """Device-resident known-chunk set of an incremental session (pbsgpu_known_*): the previous snapshot's digests
    (PreviousBackup, commit_orchestrate.go:127-158) plus every chunk sent so far. ``classify`` says per record whether
    the server already has the chunk (1) or it is the first occurrence of a new one (0: upload it). The set keeps its
    engine alive; one thread per set at a time."""

    def __init__(self, eng: Engine, capacity: int = 0):
        self._eng = eng
        self._L = eng._L
        h = C.c_void_p()
        check(self._L.pbsgpu_known_create(eng._h, int(capacity), C.byref(h)), "known_create")
        self._h = h

    def add(self, records: np.ndarray) -> None:
        """Insert every digest (idempotent)."""
        recs = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        check(self._L.pbsgpu_known_add_host(self._h, recs.ctypes.data if recs.size else None, recs.size), "known_add_host")

    def add_device(self, dptr: int, n: int) -> None:
        """add() on n records in device memory."""
        check(self._L.pbsgpu_known_add_device(self._h, int(dptr) if n else None, int(n)), "known_add_device")

    def add_didx(self, blob: bytes) -> None:
        """Insert the digests of a .didx image (its index checksum is not verified)."""
        a = np.frombuffer(blob, dtype=np.uint8)
        check(self._L.pbsgpu_known_add_didx(self._h, a.ctypes.data, a.size), "known_add_didx")

    def classify(self, records: np.ndarray, insert: bool = True, want_flags: bool = True):
        """(known flags, stats): known[i] = 1 when the set held the digest or an earlier record of this call carries it.
        stats as Engine.dedup(), with nunique / unique_bytes counting the new records."""
        recs = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        known = np.zeros(max(recs.size, 1), dtype=np.uint8) if want_flags else None
        st = _lib.DedupStats()
        check(self._L.pbsgpu_known_classify_host(self._h, recs.ctypes.data if recs.size else None, recs.size, int(insert),
                                                 known.ctypes.data if want_flags else None, C.byref(st)),
              "known_classify_host")
        return (known[: recs.size] if want_flags else None), {k: getattr(st, k) for k, _ in _lib.DedupStats._fields_}

    def classify_device(self, dptr: int, n: int, insert: bool = True, want_flags: bool = True):
        """classify() on n records in device memory."""
        known = np.zeros(max(n, 1), dtype=np.uint8) if want_flags else None
        st = _lib.DedupStats()
        check(self._L.pbsgpu_known_classify_device(self._h, int(dptr) if n else None, int(n), int(insert),
                                                   known.ctypes.data if want_flags else None, C.byref(st)),
              "known_classify_device")
        return (known[:n] if want_flags else None), {k: getattr(st, k) for k, _ in _lib.DedupStats._fields_}

    def upload_new(self, src, recs: np.ndarray, chunks, insert: bool = True, dst: DeviceBuffer | None = None,
                   nbytes: int | None = None):
        """classify + Engine.blob_encode of the new chunks in one device-side call (pbsgpu_known_upload_new_device):
        chunk i = (offset, length) `chunks[i]` of the device buffer `src` carries the digest of `recs[i]`. dst None
        allocates the worst case, sum(length + 12). Returns (buffer with .used, known flags (n), offsets (n, uint64; 0 for
        known records), CRCs (n, uint32), stats)."""
        recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE)
        n = int(recs.size)
        segs, nseg = _segs(chunks)
        assert nseg == n, "one chunk range per record"
        sp, sn = self._eng._dev(src, nbytes)
        assert sp is not None, "upload_new() wants device memory"
        own = dst is None
        if own:
            lens = np.ascontiguousarray(chunks, dtype=np.uint64).reshape(-1, 2)[:, 1] if n else np.zeros(0, dtype=np.uint64)
            dst = self._eng.alloc(max(int(lens.sum()) + 12 * n, 16))
        flags = np.zeros(max(n, 1), dtype=np.uint8)
        offs = np.zeros(max(n, 1), dtype=np.uint64)
        crcs = np.zeros(max(n, 1), dtype=np.uint32)
        used, st = C.c_uint64(), _lib.DedupStats()
        try:
            check(self._L.pbsgpu_known_upload_new_device(self._h, sp, sn, recs.ctypes.data if n else None, segs, n, int(insert),
                                                         dst.ptr, dst.nbytes, flags.ctypes.data, offs.ctypes.data,
                                                         crcs.ctypes.data, C.byref(used), C.byref(st)),
                  "known_upload_new_device")
        except Exception:
            if own:
                dst.free()
            raise
        dst.used = int(used.value)
        return dst, flags[:n], offs[:n], crcs[:n], {k: getattr(st, k) for k, _ in _lib.DedupStats._fields_}

    def upload_new2(self, src, recs: np.ndarray, chunks, insert: bool = True, zstd: bool = False,
                    dst: DeviceBuffer | None = None, nbytes: int | None = None):
        """upload_new() with the blob's kind decided on the device (pbsgpu_known_upload_new2_device): with zstd=True a new
        chunk whose zstd frame is strictly shorter than the chunk becomes a compressed blob, as Engine.blob_encode2() makes
        it; blob i lies at offsets[i], in the slot of the uncompressed layout, and is lens[i] long. zstd=False gives
        upload_new()'s outputs exactly. Returns (buffer with .used, known flags, offsets, lens, kinds (0 uncompressed,
        1 compressed), CRCs (n each; 0 for known records), stats, encode stats as Engine.blob_encode2())."""
        recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE)
        n = int(recs.size)
        segs, nseg = _segs(chunks)
        assert nseg == n, "one chunk range per record"
        sp, sn = self._eng._dev(src, nbytes)
        assert sp is not None, "upload_new2() wants device memory"
        own = dst is None
        if own:
            sizes = np.ascontiguousarray(chunks, dtype=np.uint64).reshape(-1, 2)[:, 1] if n else np.zeros(0, dtype=np.uint64)
            dst = self._eng.alloc(max(int(sizes.sum()) + 12 * n, 16))
        o = _Upload2Out(n)
        try:
            check(self._L.pbsgpu_known_upload_new2_device(self._h, sp, sn, recs.ctypes.data if n else None, segs, n, int(insert),
                                                          _lib.ENCODE_F_ZSTD if zstd else 0, dst.ptr, dst.nbytes, *o.args()),
                  "known_upload_new2_device")
        except Exception:
            if own:
                dst.free()
            raise
        return o.result(dst)

    def __len__(self) -> int:
        n = C.c_uint64()
        check(self._L.pbsgpu_known_count(self._h, C.byref(n)), "known_count")
        return int(n.value)

    def close(self):
        if getattr(self, "_h", None):
            self._L.pbsgpu_known_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class PayloadStream:
    """The payload-stream seam ``WriteEntryReader`` feeds (transfer.ArchiveWriter,
    internal/pxarmount/commit_test.go:33-67): append bytes, get (end, digest) records."""

    def __init__(self, eng: Engine, window_bytes: int = 0, hold: bool = False):
        """hold=True: the stream keeps its pages until release() (pbsgpu_stream_hold): upload_new2() frames the new chunks
        of what write() was given straight out of them. A call that needs a page then raises PbsGpuError(E_BUSY) instead
        of waiting for a page only a release can bring; write() may have taken a prefix (bytes_written())."""
        self._eng = eng
        self._L = eng._L
        h = C.c_void_p()
        check(self._L.pbsgpu_stream_create(eng._h, window_bytes, C.byref(h)), "stream_create")
        self._h = h
        if hold:
            try:
                check(self._L.pbsgpu_stream_hold(self._h), "stream_hold")
            except Exception:
                self.close()
                raise

    # ---- held pages (hold=True) -------------------------------------------------------------------------------
    def release(self, upto: int) -> None:
        """The payload below position `upto` (at most the `end` of the last polled record) is no longer needed."""
        check(self._L.pbsgpu_stream_release(self._h, int(upto)), "stream_release")

    def held(self) -> tuple:
        """(lowest position whose bytes are still available, handed-back pages the stream holds, free pages of the ring)"""
        first, pages, free = C.c_uint64(), C.c_uint32(), C.c_uint32()
        check(self._L.pbsgpu_stream_held(self._h, C.byref(first), C.byref(pages), C.byref(free)), "stream_held")
        return int(first.value), int(pages.value), int(free.value)

    def upload_new2(self, known: "KnownChunks", recs: np.ndarray, insert: bool = True, zstd: bool = False,
                    dst: DeviceBuffer | None = None):
        """PageRing.upload_new2() for records of this stream, exactly as poll() returned them (a batch may span sections):
        classified against `known`, the new ones framed out of the stream's held pages. Returns (buffer with .used, known
        flags, offsets, lens, kinds, CRCs, stats, encode stats)."""
        recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE)
        n = int(recs.size)
        own = dst is None
        if own:
            dst = self._eng.alloc(max(int(recs["size"].astype(np.uint64).sum()) + 12 * n, 16))
        o = _Upload2Out(n)
        try:
            check(self._L.pbsgpu_stream_upload_new2_device(self._h, known._h, recs.ctypes.data if n else None, n, int(insert),
                                                           _lib.ENCODE_F_ZSTD if zstd else 0, dst.ptr, dst.nbytes, *o.args()),
                  "stream_upload_new2_device")
        except Exception:
            if own:
                dst.free()
            raise
        return o.result(dst)

    def copy(self, position: int, length: int, dst: DeviceBuffer | None = None) -> DeviceBuffer:
        """The raw payload bytes [position, position + length) out of the held pages into dst (None: a new DeviceBuffer).
        The range lies in one section, is covered by polled records and is not released."""
        own = dst is None
        if own:
            dst = self._eng.alloc(max(int(length), 16))
        try:
            assert dst.nbytes >= int(length), "dst is too small"
            check(self._L.pbsgpu_stream_copy_device(self._h, int(position), int(length), dst.ptr), "stream_copy_device")
        except Exception:
            if own:
                dst.free()
            raise
        return dst

    def write(self, data) -> None:
        a = _host_view(data)
        check(self._L.pbsgpu_stream_write(self._h, a.ctypes.data if a.size else None, a.size), "stream_write")

    def reserve(self) -> np.ndarray:
        """Borrow pinned staging memory as a writable uint8 array; fill a prefix, then commit(n)."""
        buf, cap = C.c_void_p(), C.c_size_t()
        check(self._L.pbsgpu_stream_reserve(self._h, C.byref(buf), C.byref(cap)), "stream_reserve")
        return np.ctypeslib.as_array((C.c_uint8 * cap.value).from_address(buf.value))

    def commit(self, n: int) -> None:
        check(self._L.pbsgpu_stream_commit(self._h, n), "stream_commit")

    def inject(self, nbytes: int = 0) -> None:
        """Forced cut (InjectChunks flushes the open chunk, commit_reuse.go:315-341)."""
        check(self._L.pbsgpu_stream_cut(self._h, nbytes), "stream_cut")

    def finish(self) -> None:
        check(self._L.pbsgpu_stream_finish(self._h), "stream_finish")

    def finish_begin(self) -> None:
        """Close the input without waiting for the last records (the writer goes on with its next archive); poll() keeps
        delivering, done() tells when the last record is out."""
        check(self._L.pbsgpu_stream_finish_begin(self._h), "stream_finish_begin")

    def done(self) -> bool:
        d = C.c_int()
        check(self._L.pbsgpu_stream_done(self._h, C.byref(d)), "stream_done")
        return bool(d.value)

    def poll(self, cap: int = 1 << 16) -> np.ndarray:
        outs = []
        while True:
            out = np.zeros(cap, dtype=RECORD_DTYPE)
            n = C.c_uint64()
            check(self._L.pbsgpu_stream_poll(self._h, out.ctypes.data, cap, C.byref(n)), "stream_poll")
            outs.append(out[: n.value])
            if n.value < cap:
                break
        return np.concatenate(outs) if outs else np.zeros(0, dtype=RECORD_DTYPE)

    def position(self) -> int:
        """Encoder().PayloadPosition(): bytes written + bytes injected (the records' coordinate system)."""
        n = C.c_uint64()
        check(self._L.pbsgpu_stream_position(self._h, C.byref(n)), "stream_position")
        return n.value

    def bytes_written(self) -> int:
        n = C.c_uint64()
        check(self._L.pbsgpu_stream_bytes_written(self._h, C.byref(n)), "stream_bytes_written")
        return n.value

    # ---- per-file XXH3-64 tee + pxar payload entries ---------------------------------------------------------
    def begin_file(self) -> None:
        check(self._L.pbsgpu_stream_begin_file(self._h), "stream_begin_file")

    def end_file(self) -> int:
        i = C.c_uint64()
        check(self._L.pbsgpu_stream_end_file(self._h, C.byref(i)), "stream_end_file")
        return i.value

    def begin_entry(self, content_len: int) -> int:
        """Append the 16-byte payload header of a file body of content_len bytes; returns its payload offset
        (the PAYLOAD_REF / WriteEntryRef value) and opens the file tee."""
        off = C.c_uint64()
        check(self._L.pbsgpu_stream_begin_entry(self._h, None, int(content_len), C.byref(off)), "stream_begin_entry")
        return off.value

    def end_entry(self) -> int:
        i = C.c_uint64()
        check(self._L.pbsgpu_stream_end_entry(self._h, C.byref(i)), "stream_end_entry")
        return i.value

    def write_marker(self, tail: bool = False) -> None:
        check(self._L.pbsgpu_stream_write_marker(self._h, None, int(tail)), "stream_write_marker")

    def poll_files(self, cap: int = 4096) -> list:
        """[(index, size, xxh3)] of the files hashed so far (in file order)."""
        outs = []
        while True:
            buf = (_lib.FileHash * cap)()
            n = C.c_uint64()
            check(self._L.pbsgpu_stream_poll_files(self._h, buf, cap, C.byref(n)), "stream_poll_files")
            outs += [(int(buf[i].index), int(buf[i].size), int(buf[i].xxh3)) for i in range(n.value)]
            if n.value < cap:
                return outs

    def suggest(self, offset: int | None = None) -> None:
        """Suggest a chunk boundary at absolute payload position `offset` (default: here)."""
        check(self._L.pbsgpu_stream_suggest(self._h, self.position() if offset is None else int(offset)),
              "stream_suggest")

    def close(self):
        if getattr(self, "_h", None):
            self._L.pbsgpu_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def split_plan(total_len: int, world: int, rank: int, max_chunk: int):
    """(own_start, own_end, lo, hi) of `rank` for a stream split over `world` ranks (pbsgpu_split_plan: arithmetic only)."""
    v = [C.c_uint64() for _ in range(4)]
    check(_lib.lib().pbsgpu_split_plan(int(total_len), int(world), int(rank), int(max_chunk), *[C.byref(x) for x in v]),
          "split_plan")
    return tuple(int(x.value) for x in v)


class Comm:
    """The multi-GPU digest-set reduce through the C ABI (pbsgpu_comm_*): ONE RCCL all-gather of the ranks' (digest, size)
    records over xGMI + the device dedup — what a Go host binds directly (go/pbsgpu: Comm), no torch involved.
    ``Comm.unique_id()`` on rank 0, ship the 128 bytes to the other ranks, ``Comm(engine, id, rank, world)`` on every rank
    (collective), then ``dedup(records, cap_records)`` on every rank in the same order."""

    ID_BYTES = 128

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * Comm.ID_BYTES)()
        check(_lib.lib().pbsgpu_comm_unique_id(buf), "comm_unique_id")
        return bytes(buf)

    def __init__(self, eng: Engine, unique_id: bytes, rank: int, world: int):
        assert len(unique_id) == Comm.ID_BYTES
        self._eng = eng
        self._L = eng._L
        self.rank, self.world = int(rank), int(world)
        h = C.c_void_p()
        idb = (C.c_uint8 * Comm.ID_BYTES).from_buffer_copy(unique_id)
        check(self._L.pbsgpu_comm_create(eng._h, idb, self.rank, self.world, C.byref(h)), "comm_create")
        self._h = h

    def dedup(self, records: np.ndarray, cap_records: int, want_flags: bool = True):
        """(dup flags of THIS rank's records, stats of the union over all ranks). cap_records: the same on every rank."""
        recs = np.ascontiguousarray(records, dtype=RECORD_DTYPE)
        dup = np.zeros(max(recs.size, 1), dtype=np.uint8) if want_flags else None
        st = _lib.DedupStats()
        check(self._L.pbsgpu_digest_allgather_dedup(self._h, recs.ctypes.data if recs.size else None, recs.size,
                                                    int(cap_records), dup.ctypes.data if want_flags else None,
                                                    C.byref(st)), "digest_allgather_dedup")
        return (dup[: recs.size] if want_flags else None), {k: getattr(st, k) for k, _ in _lib.DedupStats._fields_}

    def split_stream(self, local_dptr: int, total_len: int) -> np.ndarray:
        """Cut + hash ONE stream of total_len bytes that is split over the ranks (collective, pbsgpu_comm_split_stream):
        local_dptr = device pointer to this rank's bytes [lo, hi) of split_plan(). The whole stream's records."""
        cap = int(total_len) // max(64, min(self._eng.config.MinSize, 1 << 30)) + 16
        out = np.zeros(cap, dtype=RECORD_DTYPE)
        n = C.c_uint64()
        check(self._L.pbsgpu_comm_split_stream(self._h, int(local_dptr) if local_dptr else None, int(total_len),
                                               out.ctypes.data, cap, C.byref(n)), "comm_split_stream")
        return out[: n.value].copy()

    def dedup_device(self, dptr: int, n: int, cap_records: int, want_flags: bool = True):
        """dedup() on n records that already are in DEVICE memory (they travel device -> device, no host round trip)."""
        dup = np.zeros(max(n, 1), dtype=np.uint8) if want_flags else None
        st = _lib.DedupStats()
        check(self._L.pbsgpu_digest_allgather_dedup(self._h, int(dptr) if n else None, int(n), int(cap_records),
                                                    dup.ctypes.data if want_flags else None, C.byref(st)),
              "digest_allgather_dedup")
        return (dup[:n] if want_flags else None), {k: getattr(st, k) for k, _ in _lib.DedupStats._fields_}

    def close(self):
        if getattr(self, "_h", None):
            self._L.pbsgpu_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Chunker:
    """Upstream-style streaming chunker: ``scan(data) -> pos`` (0 = no boundary yet)."""

    def __init__(self, eng: Engine):
        self._eng = eng
        self._L = eng._L
        h = C.c_void_p()
        check(self._L.pbsgpu_chunker_create(eng._h, C.byref(h)), "chunker_create")
        self._h = h

    def scan(self, data) -> int:
        a = _host_view(data)
        pos = C.c_size_t()
        check(self._L.pbsgpu_chunker_scan(self._h, a.ctypes.data if a.size else None, a.size, C.byref(pos)),
              "chunker_scan")
        return pos.value

    def reset(self) -> None:
        check(self._L.pbsgpu_chunker_reset(self._h), "chunker_reset")

    def close(self):
        if getattr(self, "_h", None):
            self._L.pbsgpu_chunker_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PageRing:
    """Many payload streams through one device arena with page-granular memory release and the persistent SHA-256
    service (pbsgpu_ring_*, include/pbsgpu.h): the chunk loop behind ``WriteEntryReader`` for several archives at once
    (internal/pxarmount/commit_reuse.go:457, internal/tapeio/converter.go:836) when bytes are in device memory."""

    def __init__(self, eng: Engine, arena_bytes: int = 0, page_bytes: int = 0, max_streams: int = 0, sha_cus: int = 0,
                 round_pages: int = 0, express_cus: int = 0, hold: bool = False, **options):
        """`options`: the other fields of pbsgpu_ring_options by name (flags=_lib.RING_F_NO_STAGE, lone_defer_ms=-1.0, ...).
        `hold`: PBSGPU_RING_F_HOLD_PAGES — pages stay with their stream until release(): see blob_encode() / copy()."""
        self._eng = eng
        self._L = eng._L
        opt = _lib.RingOptions(int(arena_bytes), int(page_bytes), int(max_streams), int(sha_cus), int(round_pages),
                               int(express_cus))
        for k, v in options.items():
            setattr(opt, k, v)
        if hold:
            opt.flags |= _lib.RING_F_HOLD_PAGES
        h = C.c_void_p()
        check(self._L.pbsgpu_ring_create(eng._h, C.byref(opt), C.byref(h)), "ring_create")
        self._h = h
        self.page_bytes = self.stats()["page_bytes"]

    def open(self) -> int:
        s = C.c_uint32()
        check(self._L.pbsgpu_ring_open(self._h, C.byref(s)), "ring_open")
        return s.value

    def reserve(self, stream: int):
        """(device pointer, capacity) of the stream's next page, or None when no page is free right now."""
        p, cap = C.c_void_p(), C.c_uint64()
        st = self._L.pbsgpu_ring_reserve(self._h, stream, C.byref(p), C.byref(cap))
        if st == _lib.E_BUSY:
            return None
        check(st, "ring_reserve")
        return p.value, cap.value

    def commit(self, stream: int, nbytes: int, final: bool = False) -> None:
        check(self._L.pbsgpu_ring_commit(self._h, stream, int(nbytes), int(final)), "ring_commit")

    def fill(self, stream: int, seed: int, kind: int, nbytes: int, final: bool = False) -> int:
        """Synthetic producer: bytes accepted (whole pages that were free); call again with the rest after pump()."""
        t = C.c_uint64()
        check(self._L.pbsgpu_ring_fill(self._h, stream, int(seed), int(kind), int(nbytes), int(final), C.byref(t)),
              "ring_fill")
        return t.value

    def fill_pieces(self, stream: int, pieces, nbytes: int, final: bool = False) -> int:
        """Synthetic producer for an EDITED stream: `pieces` = (n, 4) uint64 rows (dst_off, len, src_off, seed) over
        generator 4 with the stream's first call, None afterwards. Bytes accepted, as fill()."""
        t = C.c_uint64()
        if pieces is not None:
            a = np.ascontiguousarray(pieces, dtype=np.uint64).reshape(-1, 4)
            ptr, n = a.ctypes.data, a.shape[0]
        else:
            ptr, n = None, 0
        check(self._L.pbsgpu_ring_fill_pieces(self._h, stream, ptr, n, int(nbytes), int(final), C.byref(t)), "ring_fill_pieces")
        return t.value

    def pump(self) -> None:
        check(self._L.pbsgpu_ring_pump(self._h), "ring_pump")

    def poll(self, stream: int, cap: int = 4096):
        """(records, finished) — records in stream order, `end` = absolute stream offset."""
        out = np.zeros(cap, dtype=RECORD_DTYPE)
        n, fin = C.c_uint64(), C.c_int()
        check(self._L.pbsgpu_ring_poll(self._h, stream, out.ctypes.data, cap, C.byref(n), C.byref(fin)), "ring_poll")
        return out[: n.value], bool(fin.value)

    def poll_any(self, cap: int = 16384, fcap: int = 4096):
        """(records of any open stream with `segment` = stream id, ids of the streams that have just finished)"""
        if getattr(self, "_any_buf", None) is None or self._any_buf.size < cap:
            self._any_buf = np.zeros(cap, dtype=RECORD_DTYPE)
            self._fin_buf = np.zeros(fcap, dtype=np.uint32)
        n, nf = C.c_uint64(), C.c_uint32()
        check(self._L.pbsgpu_ring_poll_any(self._h, self._any_buf.ctypes.data, cap, C.byref(n), self._fin_buf.ctypes.data,
                                           min(fcap, self._fin_buf.size), C.byref(nf)), "ring_poll_any")
        return self._any_buf[: n.value].copy(), self._fin_buf[: nf.value].copy()

    def close_stream(self, stream: int) -> None:
        check(self._L.pbsgpu_ring_close(self._h, stream), "ring_close")

    # ---- held pages (hold=True): the polled chunks' bytes stay in the ring until released ----------
    def release(self, stream: int, upto: int) -> None:
        """The stream's bytes below `upto` (at most the `end` of its last polled record) are no longer needed: pages that
        lie wholly below go back to the free list. A holder that never releases stalls fill() / reserve()."""
        check(self._L.pbsgpu_ring_release(self._h, stream, int(upto)), "ring_release")

    def held(self, stream: int) -> tuple:
        """(stream offset from which bytes are still available, handed-back pages the stream is holding)"""
        first, pages = C.c_uint64(), C.c_uint32()
        check(self._L.pbsgpu_ring_held(self._h, stream, C.byref(first), C.byref(pages)), "ring_held")
        return int(first.value), int(pages.value)

    def blob_encode(self, stream, recs: np.ndarray, skip=None):
        """Uncompressed data blobs of the polled records `recs`, framed on the device straight out of the ring's pages,
        back to back in a new DeviceBuffer. `stream` None: every record's stream is its `segment` (poll_any). `skip`
        (n, truthy = leave the record out: it is known). Returns (buffer, offsets (n, uint64; untouched 0 for skipped
        records), CRCs (n, uint32)); the bytes used are sum(size + 12) over the records kept."""
        recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE)
        n = int(recs.size)
        sid = _lib.RING_ANY_STREAM if stream is None else int(stream)
        sk = None if skip is None else np.ascontiguousarray(np.asarray(skip) != 0, dtype=np.uint8)
        assert sk is None or sk.size == n
        offs = np.zeros(max(n, 1), dtype=np.uint64)
        crcs = np.zeros(max(n, 1), dtype=np.uint32)
        used = C.c_uint64()
        args = (self._h, sid, recs.ctypes.data if n else None, n, sk.ctypes.data if sk is not None and n else None)
        st = self._L.pbsgpu_ring_blob_encode_device(*args, None, 0, offs.ctypes.data, None, C.byref(used))  # the size
        if st != _lib.E_CAPACITY:
            check(st, "ring_blob_encode_device")
        dst = self._eng.alloc(max(int(used.value), 16))
        try:
            check(self._L.pbsgpu_ring_blob_encode_device(*args, dst.ptr, dst.nbytes, offs.ctypes.data, crcs.ctypes.data,
                                                         C.byref(used)), "ring_blob_encode_device")
        except Exception:
            dst.free()
            raise
        dst.used = int(used.value)
        return dst, offs[:n], crcs[:n]

    def upload_new(self, known: "KnownChunks", stream, recs: np.ndarray, insert: bool = True, dst: DeviceBuffer | None = None):
        """classify + blob_encode(skip = known) in one device-side call (pbsgpu_ring_upload_new_device): the polled
        records `recs` are classified against `known`, and the new ones framed out of the ring's pages with a plan built on
        the device. `stream` None: every record's stream is its `segment` (poll_any). dst None allocates the worst case,
        sum(size + 12); a dst that is too small raises PbsGpuError(E_CAPACITY) with the set unchanged. Returns (buffer
        with .used, known flags (n), offsets (n, uint64; 0 for known records), CRCs (n, uint32), stats)."""
        recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE)
        n = int(recs.size)
        sid = _lib.RING_ANY_STREAM if stream is None else int(stream)
        own = dst is None
        if own:
            dst = self._eng.alloc(max(int(recs["size"].astype(np.uint64).sum()) + 12 * n, 16))
        flags = np.zeros(max(n, 1), dtype=np.uint8)
        offs = np.zeros(max(n, 1), dtype=np.uint64)
        crcs = np.zeros(max(n, 1), dtype=np.uint32)
        used, st = C.c_uint64(), _lib.DedupStats()
        try:
            check(self._L.pbsgpu_ring_upload_new_device(self._h, known._h, sid, recs.ctypes.data if n else None, n, int(insert),
                                                        dst.ptr, dst.nbytes, flags.ctypes.data, offs.ctypes.data,
                                                        crcs.ctypes.data, C.byref(used), C.byref(st)),
                  "ring_upload_new_device")
        except Exception:
            if own:
                dst.free()
            raise
        dst.used = int(used.value)
        return dst, flags[:n], offs[:n], crcs[:n], {k: getattr(st, k) for k, _ in _lib.DedupStats._fields_}

    def upload_new2(self, known: "KnownChunks", stream, recs: np.ndarray, insert: bool = True, zstd: bool = False,
                    dst: DeviceBuffer | None = None):
        """upload_new() with the blob's kind decided on the device (pbsgpu_ring_upload_new2_device): with zstd=True a new
        chunk whose zstd frame is strictly shorter than the chunk becomes a compressed blob, straight out of the ring's
        pages; blob i lies at offsets[i], in the slot of the uncompressed layout, and is lens[i] long. zstd=False gives
        upload_new()'s outputs exactly. Returns (buffer with .used, known flags, offsets, lens, kinds (0 uncompressed,
        1 compressed), CRCs (n each; 0 for known records), stats, encode stats as Engine.blob_encode2())."""
        recs = np.ascontiguousarray(recs, dtype=RECORD_DTYPE)
        n = int(recs.size)
        sid = _lib.RING_ANY_STREAM if stream is None else int(stream)
        own = dst is None
        if own:
            dst = self._eng.alloc(max(int(recs["size"].astype(np.uint64).sum()) + 12 * n, 16))
        o = _Upload2Out(n)
        try:
            check(self._L.pbsgpu_ring_upload_new2_device(self._h, known._h, sid, recs.ctypes.data if n else None, n, int(insert),
                                                         _lib.ENCODE_F_ZSTD if zstd else 0, dst.ptr, dst.nbytes, *o.args()),
                  "ring_upload_new2_device")
        except Exception:
            if own:
                dst.free()
            raise
        return o.result(dst)

    def copy(self, stream: int, offset: int, length: int) -> DeviceBuffer:
        """The raw stream bytes [offset, offset + length) out of the ring's pages into a new DeviceBuffer (the range must
        be covered by polled records and not be released)."""
        dst = self._eng.alloc(max(int(length), 16))
        try:
            check(self._L.pbsgpu_ring_copy_device(self._h, int(stream), int(offset), int(length), dst.ptr), "ring_copy_device")
        except Exception:
            dst.free()
            raise
        return dst

    def quiesce(self) -> None:
        check(self._L.pbsgpu_ring_quiesce(self._h), "ring_quiesce")

    def park(self) -> None:
        """Stop the service behind everything enqueued WITHOUT waiting for it (the next pump starts a new one)."""
        check(self._L.pbsgpu_ring_park(self._h), "ring_park")

    def suggest(self, stream: int, offset: int) -> None:
        """Suggested boundary at `offset` bytes from the stream's start (ascending, ahead of the bytes around it)."""
        check(self._L.pbsgpu_ring_suggest(self._h, stream, int(offset)), "ring_suggest")

    def stats(self) -> dict:
        st = _lib.RingStats()
        check(self._L.pbsgpu_ring_get_stats(self._h, C.byref(st)), "ring_get_stats")
        return {k: getattr(st, k) for k, _ in _lib.RingStats._fields_}

    def express(self) -> tuple:
        """(CUs of the express service, chunk size from which a chunk takes it) — (0, 0) when the ring has none"""
        cus, lb = C.c_uint32(0), C.c_uint64(0)
        check(self._L.pbsgpu_ring_express(self._h, C.byref(cus), C.byref(lb)), "ring_express")
        return int(cus.value), int(lb.value)

    def probe(self) -> dict:
        """Cumulative regime counters of the two services (pbsgpu_ring_get_probe): steps, shader cycles, 100 MHz ticks."""
        p = _lib.RingProbe()
        check(self._L.pbsgpu_ring_get_probe(self._h, C.byref(p)), "ring_get_probe")
        return {k: int(getattr(p, k)) for k, _ in _lib.RingProbe._fields_}

    @staticmethod
    def probe_delta(a: dict, b: dict) -> dict:
        """What the services did between two probe() readings: ns per block step and shader clock, per service."""
        out = {}
        for svc, blocks in (("pair", 1), ("express", 2)):
            st, cy, tk = (b[f"{svc}_{k}"] - a[f"{svc}_{k}"] for k in ("steps", "cycles", "ticks"))
            if st and tk:
                out[svc] = {"ns_per_block_step": round(tk * 10.0 / st / blocks, 1), "sclk_mhz": round(cy * 100.0 / tk, 1),
                            "wave_steps_sampled": int(st)}
        return out

    def debug(self) -> str:
        buf = C.create_string_buffer(1 << 16)
        check(self._L.pbsgpu_ring_debug(self._h, buf, len(buf)), "ring_debug")
        return buf.value.decode(errors="replace")

    def ingest_synthetic(self, jobs, timeout_s: float = 120.0, concurrent: int | None = None):
        """Drive whole synthetic streams through the ring: jobs = [(seed, kind, nbytes)]; returns one record array per
        job. At most `concurrent` (default: all slots) streams are open at a time."""
        import time

        res = [[] for _ in jobs]
        todo = list(range(len(jobs)))
        active = {}                                   # stream id -> [job index, bytes left]
        limit = concurrent or len(jobs)
        t0 = time.perf_counter()
        while todo or active:
            # `limit` streams are FED at a time; a stream whose bytes are all in only waits for its last chunks
            while todo and sum(1 for v in active.values() if not v[2]) < limit:
                try:
                    sid = self.open()
                except _lib.PbsGpuError as exc:
                    if exc.status != _lib.E_BUSY:
                        raise
                    break
                j = todo.pop(0)
                active[sid] = [j, int(jobs[j][2]), False]
            quota = 16 * self.page_bytes            # pages are dealt out evenly among the open streams
            for sid, a in active.items():
                j, left, sent_final = a
                if not sent_final:
                    want = min(left, quota)
                    got = self.fill(sid, jobs[j][0], jobs[j][1], want, final=(want == left))
                    a[1] -= got
                    if a[1] == 0 and (got == want):
                        a[2] = True
            self.pump()
            for sid in list(active):
                recs, fin = self.poll(sid)
                if recs.size:
                    res[active[sid][0]].append(recs.copy())
                if fin:
                    self.close_stream(sid)
                    del active[sid]
            if time.perf_counter() - t0 > timeout_s:
                raise TimeoutError(f"ring ingest did not finish in {timeout_s} s: {self.stats()}\n{self.debug()}")
        return [np.concatenate(r) if r else np.zeros(0, dtype=RECORD_DTYPE) for r in res]

    def close(self):
        if getattr(self, "_h", None):
            self._L.pbsgpu_ring_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
