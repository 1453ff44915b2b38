"""Data blobs (pbsgpu_crc32_* / pbsgpu_blob_*) without a GPU: the C ABI, the Python / C++ / Go surfaces, the host-only
calls (the blob magics, crc32_combine against zlib, the encoded size), the argument checks that come before any device
work, and the build-quality guard for the kernels of blob.hip (no scratch, no spills, no flat_* instructions)."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOB_SYMBOLS = ("pbsgpu_blob_magic", "pbsgpu_crc32_combine", "pbsgpu_crc32_many_device", "pbsgpu_crc32_many_host",
                "pbsgpu_blob_encoded_size", "pbsgpu_blob_encode_device", "pbsgpu_blob_verify_device",
                "pbsgpu_blob_verify_host")
KERNELS = ("k_crc_pieces", "k_crc_fold", "k_blob_heads")
NAMES = ("uncompressed", "zstd compressed", "encrypted", "zstd compressed encrypted")


@pytest.fixture(scope="module")
def L():
    from pbs_plus_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _header():
    return open(os.path.join(ROOT, "include", "pbsgpu.h")).read()


def test_entry_points_are_declared_exported_and_bound(L):
    from pbs_plus_amd import _lib

    hdr = _header()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pbsgpu_[a-z0-9_]+)", out))
    for name in BLOB_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in exported, name
        assert name in _lib.SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name


def test_feature_macro_abi_version_and_constants():
    from pbs_plus_amd import _lib

    hdr = _header()
    assert re.search(r"^#define PBSGPU_HAS_BLOB 1\b", hdr, flags=re.M)
    assert re.search(r"^#define PBSGPU_ABI_VERSION 5\b", hdr, flags=re.M)  # additive: the version stays
    for name, v in (("OK", 0), ("BAD_MAGIC", 1), ("BAD_CRC", 2), ("BAD_SIZE", 3), ("BAD_DIGEST", 4), ("CRC_ONLY", 5)):
        assert re.search(r"^#define PBSGPU_BLOB_%s %d\b" % (name, v), hdr, flags=re.M), name
        assert getattr(_lib, "BLOB_" + name) == v
    assert re.search(r"^#define PBSGPU_BLOB_HEADER_SIZE 12u", hdr, flags=re.M)
    assert re.search(r"^#define PBSGPU_BLOB_ENCRYPTED_HEADER_SIZE 44u", hdr, flags=re.M)
    assert C.sizeof(_lib.BlobStats) == 9 * 8


def test_magics_are_the_sha256_derivations(L):
    want = {0: [66, 171, 56, 7, 190, 131, 112, 161], 1: [49, 185, 88, 66, 111, 182, 163, 127],
            2: [123, 103, 133, 190, 34, 45, 76, 240], 3: [230, 89, 27, 191, 11, 191, 216, 11]}
    from pbs_plus_amd import blob_magic

    for kind, name in enumerate(NAMES):
        h = hashlib.sha256(f"Proxmox Backup {name} blob v1.0".encode()).digest()[:8]
        assert list(h) == want[kind]
        assert blob_magic(kind) == h
        out = (C.c_uint8 * 8)()
        assert L.pbsgpu_blob_magic(kind, out) == 0 and bytes(out) == h
    # the same derivation gives the DIDX magic hostonly.cpp carries
    didx = hashlib.sha256(b"Proxmox Backup dynamic sized chunk index v1.0").digest()[:8]
    assert list(didx) == [28, 145, 78, 165, 25, 186, 179, 205]
    out = (C.c_uint8 * 8)()
    assert L.pbsgpu_blob_magic(4, out) == -1 and L.pbsgpu_blob_magic(-1, out) == -1 and L.pbsgpu_blob_magic(0, None) == -1


def test_crc32_combine_matches_zlib_on_random_splits(L):
    from pbs_plus_amd import crc32_combine

    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, 1 << 17, dtype=np.uint8).tobytes()
    cuts = [0, 1, 2, 3, 4, 5] + [(1 << k) + d for k in range(1, 17) for d in (-1, 0, 1)]
    cuts += [int(x) for x in rng.integers(0, len(data), 40)]
    for n in (len(data), 1000, 77, 3):
        whole = zlib.crc32(data[:n])
        for c in cuts:
            if c > n:
                continue
            a, b = data[:n - c], data[n - c:n]  # len_b = c, including 0, 1 and 2^k +- 1
            assert crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == whole, (n, c)
    out = C.c_uint32()
    assert L.pbsgpu_crc32_combine(0xCBF43926, 0, 0, C.byref(out)) == 0 and out.value == 0xCBF43926
    assert L.pbsgpu_crc32_combine(1, 2, 3, None) == -1


def test_crc32_combine_is_associative_up_to_2_to_the_40(L):
    """combine(combine(a, b, |B|), c, |C|) == combine(a, combine(b, c, |C|), |B| + |C|) for lengths up to 2^40 — the
    property the kernels' fold rests on — and a run of zero bytes checked against zlib."""
    from pbs_plus_amd import crc32_combine

    rng = np.random.default_rng(2)
    for _ in range(200):
        a, b, c = (int(x) for x in rng.integers(0, 1 << 32, 3))
        lb, lc = (int(x) for x in rng.integers(0, (1 << 40) + 1, 2))
        left = crc32_combine(crc32_combine(a, b, lb), c, lc)
        right = crc32_combine(a, crc32_combine(b, c, lc), lb + lc)
        assert left == right, (a, b, c, lb, lc)
    zeros = bytes(1 << 20)
    head = b"pbs"
    assert crc32_combine(zlib.crc32(head), zlib.crc32(zeros), len(zeros)) == zlib.crc32(head + zeros)


def test_encoded_size_and_its_overflow(L):
    from pbs_plus_amd import _lib

    n = C.c_uint64()
    segs = np.array([[0, 0], [5, 100], [7, 1 << 30]], dtype=np.uint64)
    assert L.pbsgpu_blob_encoded_size(segs.ctypes.data, 3, C.byref(n)) == 0 and n.value == 36 + 100 + (1 << 30)
    assert L.pbsgpu_blob_encoded_size(None, 0, C.byref(n)) == 0 and n.value == 0
    assert L.pbsgpu_blob_encoded_size(None, 1, C.byref(n)) == _lib.E_INVALID
    assert L.pbsgpu_blob_encoded_size(segs.ctypes.data, 3, None) == _lib.E_INVALID
    big = np.array([[0, (1 << 64) - 12]], dtype=np.uint64)  # 12 + length wraps
    assert L.pbsgpu_blob_encoded_size(big.ctypes.data, 1, C.byref(n)) == _lib.E_INVALID
    two = np.array([[0, 1 << 63], [0, 1 << 63]], dtype=np.uint64)  # the sum wraps
    assert L.pbsgpu_blob_encoded_size(two.ctypes.data, 2, C.byref(n)) == _lib.E_INVALID
    edge = np.array([[0, (1 << 64) - 13]], dtype=np.uint64)
    assert L.pbsgpu_blob_encoded_size(edge.ctypes.data, 1, C.byref(n)) == 0 and n.value == (1 << 64) - 1


def test_argument_checks_need_no_device(L):
    """NULL engine / outputs, ranges outside the buffer and host pointers handed to the _device variants are E_INVALID;
    an encode whose destination is too small is E_CAPACITY with the size it needs; empty batches are OK. None of it
    touches a device."""
    from pbs_plus_amd import _lib

    E = _lib.E_INVALID
    fake = C.cast(C.create_string_buffer(256), C.c_void_p)
    host = np.zeros(4096, dtype=np.uint8)
    segs = np.array([[0, 100], [10, 20]], dtype=np.uint64)
    outside = np.array([[4000, 100]], dtype=np.uint64)
    out = np.zeros(2, dtype=np.uint32)
    status = np.zeros(2, dtype=np.uint8)
    st = _lib.BlobStats()
    n = C.c_uint64()
    for fn in (L.pbsgpu_crc32_many_device, L.pbsgpu_crc32_many_host):
        assert fn(None, host.ctypes.data, host.size, segs.ctypes.data, 2, out.ctypes.data) == E
        assert fn(fake, host.ctypes.data, host.size, segs.ctypes.data, 2, None) == E
        assert fn(fake, host.ctypes.data, host.size, None, 2, out.ctypes.data) == E
        assert fn(fake, None, 10, segs.ctypes.data, 2, out.ctypes.data) == E
        assert fn(fake, host.ctypes.data, host.size, outside.ctypes.data, 1, out.ctypes.data) == E
        assert fn(fake, host.ctypes.data, host.size, None, 0, None) == 0
    assert L.pbsgpu_crc32_many_device(fake, host.ctypes.data, host.size, segs.ctypes.data, 2, out.ctypes.data) == E
    for fn in (L.pbsgpu_blob_verify_device, L.pbsgpu_blob_verify_host):
        assert fn(None, host.ctypes.data, host.size, segs.ctypes.data, 2, None, None, status.ctypes.data, C.byref(st)) == E
        assert fn(fake, host.ctypes.data, host.size, segs.ctypes.data, 2, None, None, None, C.byref(st)) == E
        assert fn(fake, host.ctypes.data, host.size, outside.ctypes.data, 1, None, None, status.ctypes.data, None) == E
        st.count[0] = st.blob_bytes = 9
        assert fn(fake, host.ctypes.data, host.size, None, 0, None, None, None, C.byref(st)) == 0
        assert st.count[0] == 0 and st.blob_bytes == 0
    assert L.pbsgpu_blob_verify_device(fake, host.ctypes.data, host.size, segs.ctypes.data, 2, None, None,
                                       status.ctypes.data, C.byref(st)) == E
    enc = L.pbsgpu_blob_encode_device
    assert enc(None, host.ctypes.data, host.size, segs.ctypes.data, 2, host.ctypes.data, 1 << 20, C.byref(n), None, None) == E
    assert enc(fake, host.ctypes.data, host.size, segs.ctypes.data, 2, host.ctypes.data, 1 << 20, None, None, None) == E
    assert enc(fake, host.ctypes.data, host.size, outside.ctypes.data, 1, host.ctypes.data, 1 << 20, C.byref(n), None,
               None) == E
    assert enc(fake, host.ctypes.data, host.size, segs.ctypes.data, 2, None, 0, C.byref(n), None, None) == _lib.E_CAPACITY
    assert n.value == 12 + 100 + 12 + 20
    assert enc(fake, host.ctypes.data, host.size, segs.ctypes.data, 2, host.ctypes.data, 143, C.byref(n), None,
               None) == _lib.E_CAPACITY and n.value == 144
    # enough room, but host memory where device memory belongs
    assert enc(fake, host.ctypes.data, host.size, segs.ctypes.data, 2, host.ctypes.data, 144, C.byref(n), None, None) == E
    offs = np.full(1, 7, dtype=np.uint64)
    assert enc(fake, None, 0, None, 0, None, 0, C.byref(n), offs.ctypes.data, None) == 0 and n.value == 0 and offs[0] == 0


def test_chunk_ranges_from_records_segments_and_flags():
    from pbs_plus_amd import RECORD_DTYPE, chunk_ranges

    r = np.zeros(5, dtype=RECORD_DTYPE)
    r["segment"] = [0, 0, 1, 1, 1]
    r["size"] = [10, 20, 5, 6, 7]
    r["end"] = [10, 30, 5, 11, 18]  # relative to the record's segment
    segs = [(100, 30), (1000, 18)]
    got = chunk_ranges(r, segs)
    assert got.dtype == np.uint64
    assert got.tolist() == [[100, 10], [110, 20], [1000, 5], [1005, 6], [1011, 7]]
    assert chunk_ranges(r, segs, known=np.array([1, 0, 1, 0, 0], np.uint8)).tolist() == [[110, 20], [1005, 6], [1011, 7]]
    assert chunk_ranges(r[:2]).tolist() == [[0, 10], [10, 20]]
    assert chunk_ranges(r[:0], segs).shape == (0, 2)


def test_python_surface():
    import pbs_plus_amd
    from pbs_plus_amd import Engine

    for name in ("blob_magic", "chunk_ranges", "crc32_combine"):
        assert name in pbs_plus_amd.__all__ and callable(getattr(pbs_plus_amd, name)), name
    for m in ("crc32_many", "blob_encode", "blob_verify"):
        assert callable(getattr(Engine, m)), m


def test_cpp_mirror_has_the_blob_calls():
    hpp = open(os.path.join(ROOT, "include", "pbsgpu.hpp")).read()
    for fn in ("pbsgpu_crc32_many_host", "pbsgpu_crc32_many_device", "pbsgpu_blob_encoded_size", "pbsgpu_blob_encode_device",
               "pbsgpu_blob_verify_host", "pbsgpu_blob_verify_device", "pbsgpu_blob_magic", "pbsgpu_crc32_combine"):
        assert fn + "(" in hpp, fn


def test_go_binding_calls_the_entry_points_and_fallback_mirrors_them():
    go = open(os.path.join(ROOT, "go", "pbsgpu", "pbsgpu.go")).read()
    fb = open(os.path.join(ROOT, "go", "pbsgpu", "fallback.go")).read()
    for name in ("pbsgpu_crc32_many_host", "pbsgpu_blob_encoded_size", "pbsgpu_blob_encode_device", "pbsgpu_blob_verify_host",
                 "pbsgpu_blob_verify_device", "pbsgpu_blob_magic", "pbsgpu_crc32_combine"):
        assert re.search(r"\bC\.%s\(" % name, go), name
    for sig in (r"^func \(e \*Engine\) CRC32Files\(", r"^func \(e \*Engine\) EncodeBlobsDevice\(",
                r"^func \(e \*Engine\) VerifyBlobs\(", r"^func \(e \*Engine\) VerifyBlobsDevice\(", r"^func BlobMagic\(",
                r"^func CRC32Combine\(", r"^func BlobEncodedSize\("):
        assert re.search(sig, go, flags=re.M), sig
        assert re.search(sig, fb, flags=re.M), sig


def test_blob_kernels_do_not_spill_and_use_no_flat_memory_instructions(tmp_path):
    src = os.path.join(ROOT, "pbs_plus_amd", "csrc", "blob.hip")
    asm = str(tmp_path / "blob.s")
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only",
                          "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", asm],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    usage, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"),
                         ("vgpr_spill", r"VGPRs Spill: (\d+)")):
            mm = re.search(pat, line)
            if mm:
                cur[key] = int(mm.group(1))
    text = open(asm).read()
    for k in KERNELS:
        names = [n for n in usage if k in n]
        assert len(names) == 1, (k, list(usage))
        r = usage[names[0]]
        assert r.get("scratch", -1) == 0 and r.get("sgpr_spill", -1) == 0 and r.get("vgpr_spill", -1) == 0, (k, r)
        m = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape(names[0]), text, flags=re.S | re.M)
        assert m, k
        body = m.group(1).splitlines()
        assert not [ln for ln in body if re.match(r"\s+flat_", ln)], k
        assert [ln for ln in body if re.match(r"\s+global_", ln)], k
    # the piece kernel reads its tables from LDS
    m = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape([n for n in usage if "k_crc_pieces" in n][0]), text,
                  flags=re.S | re.M)
    assert [ln for ln in m.group(1).splitlines() if re.match(r"\s+ds_read", ln)]
