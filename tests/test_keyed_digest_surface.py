"""The surface of the keyed chunk digest without a GPU: the header declares the new entry points and PBSGPU_HAS_KEYED_DIGEST,
the ABI version stays 5, the library exports them, and every call refuses a NULL where it needs a value before it touches a
device. The documents name what the change leaves out."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pbsgpu_id_key_create", "pbsgpu_id_key_destroy", "pbsgpu_sha256_keyed_many_device", "pbsgpu_sha256_keyed_many_host",
         "pbsgpu_submit_device_keyed", "pbsgpu_submit_host_keyed", "pbsgpu_blob_decode4_device")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_header_declares_the_entry_points_and_keeps_the_abi_version():
    hdr = _read("include", "pbsgpu.h")
    assert "#define PBSGPU_HAS_KEYED_DIGEST 1" in hdr and "#define PBSGPU_ABI_VERSION 5" in hdr
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
    assert "typedef struct pbsgpu_id_key pbsgpu_id_key;" in hdr
    # decode4 = decode3 plus one pointer
    args = lambda n: re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S), re.S).group(1).count(",") + 1  # noqa: E731
    assert args("pbsgpu_blob_decode4_device") == args("pbsgpu_blob_decode3_device") + 1
    assert args("pbsgpu_submit_device_keyed") == args("pbsgpu_submit_device") + 1
    assert args("pbsgpu_sha256_keyed_many_device") == args("pbsgpu_sha256_many_device")


def test_the_calls_refuse_nulls_before_any_device_work():
    from pbs_plus_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    assert L.pbsgpu_abi_version() == 5
    out, t = C.c_void_p(), C.c_uint64()
    key = (C.c_uint8 * 32)()
    dig = (C.c_uint8 * 32)()
    assert L.pbsgpu_id_key_create(None, key, C.byref(out)) == _lib.E_INVALID and not out.value
    L.pbsgpu_id_key_destroy(None)  # NULL is allowed
    assert L.pbsgpu_sha256_keyed_many_device(None, None, 0, None, 0, dig) == _lib.E_INVALID
    assert L.pbsgpu_sha256_keyed_many_host(None, None, 0, None, 0, dig) == _lib.E_INVALID
    assert L.pbsgpu_submit_device_keyed(None, None, None, 0, None, 0, C.byref(t)) == _lib.E_INVALID
    assert L.pbsgpu_submit_host_keyed(None, None, None, 0, None, 0, C.byref(t)) == _lib.E_INVALID
    st = (C.c_uint8 * 4)()
    assert L.pbsgpu_blob_decode4_device(None, None, 0, None, 0, None, 1, None, 0, 0, 0, None, None, None, 0, st, None) == _lib.E_INVALID
    assert L.pbsgpu_blob_decode4_device(None, None, 0, None, 0, None, 0, None, 0, 0, 8, None, None, None, 0, st, None) == _lib.E_INVALID  # flag


def test_the_kernels_share_one_tail_function_with_the_cpu_test():
    kern = _read("pbs_plus_amd", "csrc", "kernels.hip")
    cpu = _read("tests", "native", "test_sha256_suffix.cpp")
    assert '#include "sha256_suffix.h"' in kern and "pbss::sha256_suffix_block(" in kern
    assert "sha256_suffix.h" in cpu and "pbss::sha256_suffix_block(" in cpu
    # the page ring's source has no keyed twin
    assert "KeyedRecordSource" in kern and "KeyedSegmentSource" in kern and "KeyedRingSource" not in kern


def test_the_documents_say_what_is_done_and_what_is_left():
    design, integ, nxt, readme = _read("DESIGN.md"), _read("INTEGRATION.md"), _read("NEXT.md"), _read("README.md")
    assert "## 23. Keyed chunk digests" in design and "**Measured**" in design.split("## 23. Keyed chunk digests")[1]
    assert "Why not the ring" in design
    assert "DecodeBlobs4" in integ and "SubmitKeyed" in integ and "UNVERIFIED" in integ and "_id_key" in integ
    assert "pbsgpu_blob_decode4_device" in readme
    for left in ("page ring's services", "`pbsgpu_blob_verify_*` with keys", "keyed `_suggested` submits", "key-file KDF",
                 "encrypted kinds inside the fused upload calls"):
        assert left in nxt, left
