"""ctypes binding of libpbsgpu (the C ABI in include/pbsgpu.h).

Loads the in-tree shared library ``pbs_plus_amd/lib/libpbsgpu.so`` (built by
``__graft_entry__.build()`` / ``make -C pbs_plus_amd/csrc``). There is no
fallback of any kind: a missing library or a missing GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PBSGPU_LIB_PATH") or os.path.join(_HERE, "lib", "libpbsgpu.so")   # (override: A/B builds, scripts/)
CSRC = os.path.join(_HERE, "csrc")

OK = 0
E_INVALID, E_NO_DEVICE, E_HIP, E_NOMEM, E_CAPACITY, E_BUSY, E_TICKET, _E_RETIRED_8, E_STATE = range(-1, -10, -1)  # (-8 was E_DENSITY until ABI v4)


class PbsGpuError(RuntimeError):
    def __init__(self, status: int, what: str = ""):
        self.status = status
        msg = lib().pbsgpu_strerror(status).decode() if _lib is not None else str(status)
        hip = lib().pbsgpu_last_hip_error() if _lib is not None else 0
        extra = ""
        if _lib is not None and ("comm" in what or "allgather" in what):
            txt = lib().pbsgpu_comm_last_error()
            if txt:
                extra = f"; RCCL: {txt.decode(errors='replace')}"
        super().__init__(f"{what}: {msg} (status {status}, hipError {hip}{extra})")


class Config(C.Structure):
    """pbsgpu_config — mirrors buzhash.Config (reference commit_orchestrate.go:143-149)."""

    _fields_ = [
        ("avg", C.c_uint32),
        ("min", C.c_uint32),
        ("max", C.c_uint32),
        ("window", C.c_uint32),
        ("mask", C.c_uint32),
        ("break_min", C.c_uint32),
        ("table", C.c_uint32 * 256),
    ]


class Segment(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("length", C.c_uint64)]


class Timing(C.Structure):
    _fields_ = [
        ("h2d_ms", C.c_float),
        ("scan_ms", C.c_float),
        ("resolve_ms", C.c_float),
        ("sha_ms", C.c_float),
        ("total_ms", C.c_float),
        ("ncandidates", C.c_uint64),
        ("nrecords", C.c_uint64),
        ("retries", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class PayloadFormat(C.Structure):
    _fields_ = [
        ("payload_type", C.c_uint64),
        ("start_type", C.c_uint64),
        ("tail_type", C.c_uint64),
        ("with_start", C.c_uint32),
        ("with_tail", C.c_uint32),
    ]


class ReuseChunk(C.Structure):
    _fields_ = [("size", C.c_uint64), ("padding", C.c_uint64), ("end_offset", C.c_uint64), ("digest", C.c_uint8 * 32)]


class FileHash(C.Structure):
    _fields_ = [("index", C.c_uint64), ("size", C.c_uint64), ("xxh3", C.c_uint64)]


RING_OFF = 0xFFFFFFFF
RING_F_NO_OVERLAP, RING_F_NO_STAGE, RING_F_NO_CUT_PRIO, RING_F_NO_SPLIT_AUTO, RING_F_DEFER_SERVICE, RING_F_FILL_SERIAL = 1, 2, 4, 8, 16, 32
RING_F_DENSE_SERVICE = 64
RING_F_DENSE_LANES = 128
RING_F_TIER_TAG = 256
RING_F_HOLD_PAGES = 512
RING_ANY_STREAM = 0xFFFFFFFF


class RingOptions(C.Structure):
    """pbsgpu_ring_options (ABI v5): positional use keeps working for the first six fields; the rest by keyword."""
    _fields_ = [("arena_bytes", C.c_uint64), ("page_bytes", C.c_uint64), ("max_streams", C.c_uint32),
                ("sha_cus", C.c_uint32), ("round_pages", C.c_uint32), ("express_cus", C.c_uint32),
                ("min_round_pages", C.c_uint32), ("max_inflight", C.c_uint32), ("long_bytes", C.c_uint32),
                ("long_lo_bytes", C.c_uint32), ("long_spill", C.c_uint32), ("poll_every", C.c_uint32), ("flags", C.c_uint32),
                ("lanes_cus", C.c_uint32), ("backlog_mib", C.c_double), ("lone_defer_ms", C.c_double),
                ("idle_timeout_s", C.c_double), ("autopark_ms", C.c_double), ("short_bytes", C.c_uint64), ("fill_cus", C.c_uint32),
                ("reserved1", C.c_uint32), ("reserved", C.c_uint64 * 2)]


class EngineOptions(C.Structure):
    """pbsgpu_engine_options (ABI v5)"""
    _fields_ = [("inflight", C.c_uint32), ("sha_form", C.c_uint32), ("sha_slack_pct", C.c_uint32), ("sha_dense_pct", C.c_uint32),
                ("resolve_par_min", C.c_uint64), ("sha_many_files_per_core", C.c_uint32), ("stream_sha_cus", C.c_uint32),
                ("stream_express_cus", C.c_uint32), ("stream_ring_slots", C.c_uint32), ("stream_ctx_pool", C.c_uint32),
                ("zstd_seq_tables", C.c_uint32), ("stream_ring_gib", C.c_double), ("stream_page_bytes", C.c_uint64),
                ("zstd_window_log", C.c_uint32), ("reserved1", C.c_uint32), ("reserved", C.c_uint64 * 3)]


class RingStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("page_bytes", "bytes_enqueued", "chunks", "candidates", "pages_enqueued",
                                          "pages_recycled", "service_bytes_last")] + \
               [(k, C.c_uint32) for k in ("pages_total", "pages_free", "sha_cus", "rounds", "rounds_done",
                                          "rounds_in_flight", "streams_opened", "service_launches")] + \
               [("service_ms_last", C.c_double), ("service_ms_total", C.c_double)]


class RingProbe(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("pair_steps", "pair_cycles", "pair_ticks", "express_steps", "express_cycles",
                                          "express_ticks")]


class DedupStats(C.Structure):
    _fields_ = [
        ("nrecords", C.c_uint64),
        ("nunique", C.c_uint64),
        ("total_bytes", C.c_uint64),
        ("unique_bytes", C.c_uint64),
    ]


BLOB_UNCOMPRESSED, BLOB_COMPRESSED, BLOB_ENCRYPTED, BLOB_ENCRYPTED_COMPRESSED = range(4)
BLOB_HEADER_SIZE, BLOB_ENCRYPTED_HEADER_SIZE = 12, 44
BLOB_OK, BLOB_BAD_MAGIC, BLOB_BAD_CRC, BLOB_BAD_SIZE, BLOB_BAD_DIGEST, BLOB_CRC_ONLY = range(6)
BLOB_STATUS_NAMES = ("ok", "bad_magic", "bad_crc", "bad_size", "bad_digest", "crc_only")


BLOB_BAD_DATA = 6  # blob_decode2 only
BLOB_STATUS_NAMES2 = BLOB_STATUS_NAMES + ("bad_data",)
DECODE_F_DIGEST, DECODE_F_ZSTD = 1, 2


class DecodeStats2(C.Structure):
    _fields_ = [("count", C.c_uint64 * 8), ("blob_bytes", C.c_uint64), ("crc_bytes", C.c_uint64), ("sha_bytes", C.c_uint64),
                ("out_bytes", C.c_uint64), ("zstd_in_bytes", C.c_uint64), ("zstd_out_bytes", C.c_uint64)]


BLOB_BAD_TAG = 7  # blob_decode3 only
BLOB_STATUS_NAMES3 = BLOB_STATUS_NAMES2 + ("bad_tag",)
DECODE_F_AES = 4


class DecodeStats3(C.Structure):
    _fields_ = DecodeStats2._fields_ + [("aes_bytes", C.c_uint64)]


ZSTD_OK, ZSTD_BAD_FRAME, ZSTD_BAD_SIZE, ZSTD_UNSUPPORTED = range(4)
ZSTD_STATUS_NAMES = ("ok", "bad_frame", "bad_size", "unsupported")
ZSTD_BAD_CHECKSUM = 4  # zstd_decode2(checksum=True) only
ZSTD_F_CHECKSUM, ZSTD_F_STREAM = 1, 2
ENCODE_F_ZSTD = 1
AES_OK, AES_BAD_TAG = 0, 1
AES_F_ENCRYPT = 1


class EncodeStats(C.Structure):
    _fields_ = [("blobs", C.c_uint64 * 2), ("blob_bytes", C.c_uint64 * 2), ("chunk_bytes", C.c_uint64 * 2),
                ("frame_bytes", C.c_uint64), ("crc_bytes", C.c_uint64)]


ENCODE_F_AES = 2  # blob_encode3 only


class EncodeStats3(C.Structure):
    _fields_ = [("blobs", C.c_uint64 * 4), ("blob_bytes", C.c_uint64 * 4), ("chunk_bytes", C.c_uint64 * 4),
                ("frame_bytes", C.c_uint64), ("crc_bytes", C.c_uint64), ("aes_bytes", C.c_uint64)]


class BlobStats(C.Structure):
    _fields_ = [("count", C.c_uint64 * 6), ("blob_bytes", C.c_uint64), ("crc_bytes", C.c_uint64), ("sha_bytes", C.c_uint64)]


class DecodeStats(C.Structure):
    _fields_ = [("count", C.c_uint64 * 6), ("blob_bytes", C.c_uint64), ("crc_bytes", C.c_uint64), ("sha_bytes", C.c_uint64),
                ("out_bytes", C.c_uint64)]


# pbsgpu_record: 48 bytes, same layout as a DIDX entry + (segment, size)
RECORD_DTYPE = np.dtype([("end", "<u8"), ("digest", "u1", (32,)), ("segment", "<u4"), ("size", "<u4")])
assert RECORD_DTYPE.itemsize == 48

# every symbol include/pbsgpu.h declares: name -> (restype, argtypes)
_P = C.c_void_p
_U64P = C.POINTER(C.c_uint64)
SYMBOLS = {
    "pbsgpu_strerror": (C.c_char_p, [C.c_int]),
    "pbsgpu_abi_version": (C.c_int, []),
    "pbsgpu_last_hip_error": (C.c_int, []),
    "pbsgpu_device_count": (C.c_int, []),
    "pbsgpu_config_init": (C.c_int, [C.c_uint64, _P, C.POINTER(Config)]),
    "pbsgpu_default_table": (C.POINTER(C.c_uint32), []),
    "pbsgpu_engine_create": (C.c_int, [C.c_int, C.POINTER(Config), C.c_uint32, C.POINTER(_P)]),
    "pbsgpu_engine_create_opt": (C.c_int, [C.c_int, C.POINTER(Config), C.POINTER(EngineOptions), C.POINTER(_P)]),
    "pbsgpu_engine_destroy": (None, [_P]),
    "pbsgpu_engine_config": (C.c_int, [_P, C.POINTER(Config)]),
    "pbsgpu_engine_trim": (C.c_int, [_P, _U64P]),
    "pbsgpu_engine_set_suggested_feed": (C.c_int, [_P, C.c_uint64, C.c_int]),
    "pbsgpu_sha256_many_pays": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(C.c_int)]),
    "pbsgpu_submit_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _U64P]),
    "pbsgpu_submit_host": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _U64P]),
    "pbsgpu_submit_device_suggested": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P, _P, _U64P]),
    "pbsgpu_submit_host_suggested": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P, _P, _U64P]),
    "pbsgpu_wait": (C.c_int, [_P, C.c_uint64, _U64P]),
    "pbsgpu_ticket_done": (C.c_int, [_P, C.c_uint64, C.POINTER(C.c_int)]),
    "pbsgpu_collect": (C.c_int, [_P, C.c_uint64, _P, C.c_uint64, _U64P]),
    "pbsgpu_ticket_timing": (C.c_int, [_P, C.c_uint64, C.POINTER(Timing)]),
    "pbsgpu_candidates_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, _U64P]),
    "pbsgpu_resolve_candidates": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, _P, C.c_uint64, _U64P]),
    "pbsgpu_chunker_create": (C.c_int, [_P, C.POINTER(_P)]),
    "pbsgpu_chunker_destroy": (None, [_P]),
    "pbsgpu_chunker_scan": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
    "pbsgpu_chunker_reset": (C.c_int, [_P]),
    "pbsgpu_stream_create": (C.c_int, [_P, C.c_uint64, C.POINTER(_P)]),
    "pbsgpu_stream_destroy": (None, [_P]),
    "pbsgpu_stream_write": (C.c_int, [_P, _P, C.c_size_t]),
    "pbsgpu_stream_reserve": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "pbsgpu_stream_commit": (C.c_int, [_P, C.c_size_t]),
    "pbsgpu_stream_cut": (C.c_int, [_P, C.c_uint64]),
    "pbsgpu_stream_finish": (C.c_int, [_P]),
    "pbsgpu_stream_finish_begin": (C.c_int, [_P]),
    "pbsgpu_stream_done": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "pbsgpu_stream_poll": (C.c_int, [_P, _P, C.c_uint64, _U64P]),
    "pbsgpu_stream_position": (C.c_int, [_P, _U64P]),
    "pbsgpu_stream_bytes_written": (C.c_int, [_P, _U64P]),
    "pbsgpu_stream_suggest": (C.c_int, [_P, C.c_uint64]),
    "pbsgpu_stream_hold": (C.c_int, [_P]),
    "pbsgpu_stream_release": (C.c_int, [_P, C.c_uint64]),
    "pbsgpu_stream_held": (C.c_int, [_P, _U64P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "pbsgpu_stream_upload_new2_device": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_int, C.c_uint32, _P, C.c_uint64, _P, _P, _P, _P, _P,
                                                   _U64P, C.POINTER(DedupStats), C.POINTER(EncodeStats)]),
    "pbsgpu_stream_copy_device": (C.c_int, [_P, C.c_uint64, C.c_uint64, _P]),
    "pbsgpu_stream_begin_file": (C.c_int, [_P]),
    "pbsgpu_stream_end_file": (C.c_int, [_P, _U64P]),
    "pbsgpu_stream_poll_files": (C.c_int, [_P, _P, C.c_uint64, _U64P]),
    "pbsgpu_stream_begin_entry": (C.c_int, [_P, _P, C.c_uint64, _U64P]),
    "pbsgpu_stream_end_entry": (C.c_int, [_P, _U64P]),
    "pbsgpu_stream_write_marker": (C.c_int, [_P, _P, C.c_int]),
    "pbsgpu_ring_create": (C.c_int, [_P, C.POINTER(RingOptions), C.POINTER(_P)]),
    "pbsgpu_ring_destroy": (None, [_P]),
    "pbsgpu_ring_open": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "pbsgpu_ring_reserve": (C.c_int, [_P, C.c_uint32, C.POINTER(_P), _U64P]),
    "pbsgpu_ring_commit": (C.c_int, [_P, C.c_uint32, C.c_uint64, C.c_int]),
    "pbsgpu_ring_fill": (C.c_int, [_P, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, _U64P]),
    "pbsgpu_ring_pump": (C.c_int, [_P]),
    "pbsgpu_ring_poll": (C.c_int, [_P, C.c_uint32, _P, C.c_uint64, _U64P, C.POINTER(C.c_int)]),
    "pbsgpu_ring_poll_any": (C.c_int, [_P, _P, C.c_uint64, _U64P, _P, C.c_uint32, C.POINTER(C.c_uint32)]),
    "pbsgpu_ring_close": (C.c_int, [_P, C.c_uint32]),
    "pbsgpu_ring_quiesce": (C.c_int, [_P]),
    "pbsgpu_ring_park": (C.c_int, [_P]),
    "pbsgpu_ring_fill_pieces": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, C.c_uint64, C.c_int, _U64P]),
    "pbsgpu_ring_suggest": (C.c_int, [_P, C.c_uint32, C.c_uint64]),
    "pbsgpu_ring_get_stats": (C.c_int, [_P, C.POINTER(RingStats)]),
    "pbsgpu_ring_debug": (C.c_int, [_P, C.c_char_p, C.c_uint64]),
    "pbsgpu_ring_express": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "pbsgpu_ring_get_probe": (C.c_int, [_P, C.POINTER(RingProbe)]),
    "pbsgpu_ring_release": (C.c_int, [_P, C.c_uint32, C.c_uint64]),
    "pbsgpu_ring_held": (C.c_int, [_P, C.c_uint32, _U64P, C.POINTER(C.c_uint32)]),
    "pbsgpu_ring_blob_encode_device": (C.c_int, [_P, C.c_uint32, _P, C.c_uint64, _P, _P, C.c_uint64, _P, _P, _U64P]),
    "pbsgpu_ring_copy_device": (C.c_int, [_P, C.c_uint32, C.c_uint64, C.c_uint64, _P]),
    "pbsgpu_sha256_many_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P]),
    "pbsgpu_sha256_many_host": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P]),
    "pbsgpu_xxh3_many_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P]),
    "pbsgpu_xxh3_many_host": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P]),
    "pbsgpu_dedup_host": (C.c_int, [_P, _P, C.c_uint64, _P, C.POINTER(DedupStats)]),
    "pbsgpu_dedup_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.POINTER(DedupStats)]),
    "pbsgpu_known_create": (C.c_int, [_P, C.c_uint64, C.POINTER(_P)]),
    "pbsgpu_known_destroy": (None, [_P]),
    "pbsgpu_known_count": (C.c_int, [_P, _U64P]),
    "pbsgpu_known_add_host": (C.c_int, [_P, _P, C.c_uint64]),
    "pbsgpu_known_add_device": (C.c_int, [_P, _P, C.c_uint64]),
    "pbsgpu_known_add_didx": (C.c_int, [_P, _P, C.c_uint64]),
    "pbsgpu_known_classify_host": (C.c_int, [_P, _P, C.c_uint64, C.c_int, _P, C.POINTER(DedupStats)]),
    "pbsgpu_known_classify_device": (C.c_int, [_P, _P, C.c_uint64, C.c_int, _P, C.POINTER(DedupStats)]),
    "pbsgpu_blob_magic": (C.c_int, [C.c_int, _P]),
    "pbsgpu_crc32_combine": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32)]),
    "pbsgpu_crc32_many_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P]),
    "pbsgpu_crc32_many_host": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P]),
    "pbsgpu_blob_encoded_size": (C.c_int, [_P, C.c_uint32, _U64P]),
    "pbsgpu_blob_encode_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P, C.c_uint64, _U64P, _P, _P]),
    "pbsgpu_blob_verify_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P, _P, _P, C.POINTER(BlobStats)]),
    "pbsgpu_blob_verify_host": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P, _P, _P, C.POINTER(BlobStats)]),
    "pbsgpu_blob_decode_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P, C.c_uint64, _P, C.c_uint64, C.c_uint64,
                                            C.c_int, _P, C.c_uint64, _P, C.POINTER(DecodeStats)]),
    "pbsgpu_blob_decode2_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P, C.c_uint64, _P, C.c_uint64, C.c_uint64,
                                             C.c_uint32, _P, C.c_uint64, _P, C.POINTER(DecodeStats2)]),
    "pbsgpu_zstd_frame_info": (C.c_int, [_P, C.c_uint64, _U64P, _U64P, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    "pbsgpu_zstd_decode_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P, _P, C.c_uint64, _P, _P]),
    "pbsgpu_zstd_encode_bound": (C.c_uint64, [C.c_uint64]),
    "pbsgpu_xxh64_many_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, C.c_uint64, _P]),
    "pbsgpu_zstd_decode2_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P, _P, C.c_uint64, _P, _P, C.c_uint32]),
    "pbsgpu_zstd_stream_info": (C.c_int, [_P, C.c_uint64, _U64P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    "pbsgpu_zstd_encode_bound2": (C.c_uint64, [C.c_uint64, C.c_uint32]),
    "pbsgpu_zstd_encode2_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P, _P, C.c_uint64, _P, _P, C.c_uint32]),
    "pbsgpu_zstd_encode_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P, _P, C.c_uint64, _P, _P]),
    "pbsgpu_blob_encode2_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, C.c_uint32, _P, C.c_uint64, _P, _P, _P, _P, _P]),
    "pbsgpu_ring_upload_new_device": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint64, C.c_int, _P, C.c_uint64, _P, _P, _P, _U64P,
                                                C.POINTER(DedupStats)]),
    "pbsgpu_known_upload_new_device": (C.c_int, [_P, _P, C.c_uint64, _P, _P, C.c_uint64, C.c_int, _P, C.c_uint64, _P, _P, _P,
                                                 _U64P, C.POINTER(DedupStats)]),
    "pbsgpu_ring_upload_new2_device": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint64, C.c_int, C.c_uint32, _P, C.c_uint64, _P, _P, _P,
                                                 _P, _P, _U64P, C.POINTER(DedupStats), C.POINTER(EncodeStats)]),
    "pbsgpu_known_upload_new2_device": (C.c_int, [_P, _P, C.c_uint64, _P, _P, C.c_uint64, C.c_int, C.c_uint32, _P, C.c_uint64, _P,
                                                  _P, _P, _P, _P, _U64P, C.POINTER(DedupStats), C.POINTER(EncodeStats)]),
    "pbsgpu_aes_key_create": (C.c_int, [_P, _P, C.POINTER(_P)]),
    "pbsgpu_aes_key_destroy": (None, [_P]),
    "pbsgpu_aes_gcm_many_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P, C.c_uint32, _P, _P, _P, C.c_uint64, _P,
                                             C.c_uint32]),
    "pbsgpu_blob_decode3_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P, C.c_uint64, _P, C.c_uint64, C.c_uint64,
                                             C.c_uint32, _P, _P, C.c_uint64, _P, C.POINTER(DecodeStats3)]),
    "pbsgpu_id_key_create": (C.c_int, [_P, _P, C.POINTER(_P)]),
    "pbsgpu_id_key_destroy": (None, [_P]),
    "pbsgpu_sha256_keyed_many_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P]),
    "pbsgpu_sha256_keyed_many_host": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P]),
    "pbsgpu_submit_device_keyed": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.c_uint32, _U64P]),
    "pbsgpu_submit_host_keyed": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.c_uint32, _U64P]),
    "pbsgpu_blob_decode4_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P, C.c_uint64, _P, C.c_uint64, C.c_uint64,
                                             C.c_uint32, _P, _P, _P, C.c_uint64, _P, C.POINTER(DecodeStats3)]),
    "pbsgpu_blob_encoded_size3": (C.c_int, [_P, C.c_uint32, C.c_uint32, _U64P]),
    "pbsgpu_blob_encode3_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_uint64, _P, _P, _P, _P,
                                             C.POINTER(EncodeStats3)]),
    "pbsgpu_comm_unique_id": (C.c_int, [_P]),
    "pbsgpu_comm_create": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(_P)]),
    "pbsgpu_comm_destroy": (None, [_P]),
    "pbsgpu_comm_rank": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pbsgpu_comm_last_error": (C.c_char_p, []),
    "pbsgpu_digest_allgather_dedup": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, _P, C.POINTER(DedupStats)]),
    "pbsgpu_split_plan": (C.c_int, [C.c_uint64, C.c_int, C.c_int, C.c_uint32] + [C.POINTER(C.c_uint64)] * 4),
    "pbsgpu_comm_split_stream": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pbsgpu_didx_size": (C.c_int, [C.c_uint64, _U64P]),
    "pbsgpu_didx_encode": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_int64, _P, C.c_uint64]),
    "pbsgpu_didx_decode": (C.c_int, [_P, C.c_uint64, _P, C.c_uint64, _U64P, C.POINTER(C.c_int64), _P]),
    "pbsgpu_payload_format_default": (C.c_int, [C.POINTER(PayloadFormat)]),
    "pbsgpu_payload_size": (C.c_int, [_P, C.c_uint32, C.POINTER(PayloadFormat), _U64P]),
    "pbsgpu_payload_pack_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, C.POINTER(PayloadFormat), _P, C.c_uint64,
                                             _U64P, _P]),
    "pbsgpu_reuse_lookup": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint64, _P, C.c_uint64, _U64P, _U64P, _U64P]),
    "pbsgpu_reuse_should": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint64, _P, C.c_double, C.POINTER(C.c_int)]),
    "pbsgpu_fill_device": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32]),
    "pbsgpu_gather_device": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, _P, C.c_uint32]),
    "pbsgpu_measure_h2d": (C.c_int, [_P, C.c_uint64, C.POINTER(C.c_double)]),
    "pbsgpu_device_alloc": (C.c_int, [_P, C.c_uint64, C.POINTER(_P)]),
    "pbsgpu_device_free": (C.c_int, [_P, _P]),
    "pbsgpu_memcpy_h2d": (C.c_int, [_P, _P, _P, C.c_uint64]),
    "pbsgpu_memcpy_d2h": (C.c_int, [_P, _P, _P, C.c_uint64]),
}


def build(force: bool = False) -> str:
    """Compile libpbsgpu.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:
        subprocess.run(["make", "-C", CSRC, "-s", "clean"], check=True)
    subprocess.run(["make", "-C", CSRC, "-s", "-j4", "all"], check=True)
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError = the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(status: int, what: str) -> None:
    if status != OK:
        raise PbsGpuError(status, what)
