"""The surface of the encrypted blob writer without a GPU: the C ABI additions (pbsgpu_blob_encode3_device,
pbsgpu_blob_encoded_size3), their bindings in Python, the C++ mirror, Go and the Go fallback, the refusals that come before
any device work, and the build-quality guard for the kernels of aes_encode.hip and the new CRC pair of blob.hip (no spills,
no scratch, no flat_* instructions, LDS within the budget of eight workgroups per CU) with the unit listed in the Makefile."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_zstd_surface import _body, _compile  # noqa: E402  (resource usage per kernel and assembly text of a translation unit)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = {"pbsgpu_blob_encode3_device": 15, "pbsgpu_blob_encoded_size3": 4}
AES_KERNELS = ("k_aese_head", "k_aese_pieces", "k_aese_fold")
CRC_KERNELS = ("k_enc3_pieces", "k_enc3_fold")
LDS_BUDGET = 20 << 10  # eight workgroups fit a CU's 160 KiB


@pytest.fixture(scope="module")
def L():
    from pbs_plus_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_names_are_declared_exported_and_bound(L):
    from pbs_plus_amd import _lib

    hdr = _read("include", "pbsgpu.h")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pbsgpu_[a-z0-9_]+)", out))
    for name, n in NARGS.items():
        assert re.search(r"^int %s\s*\(" % name, hdr, flags=re.M), name
        assert name in exported and name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == n, name
        assert getattr(L, name).argtypes is not None
    for name, val in (("PBSGPU_HAS_BLOB_ENCRYPT", "1"), ("PBSGPU_ENCODE_F_AES", "2u"), ("PBSGPU_ENCODE_F_ZSTD", "1u")):
        assert re.search(r"^#define %s %s\b" % (name, val), hdr, flags=re.M), name
    assert (_lib.ENCODE_F_ZSTD, _lib.ENCODE_F_AES) == (1, 2)
    st = _lib.EncodeStats3
    assert C.sizeof(st) == 15 * 8 and st.blobs.offset == 0 and st.blob_bytes.offset == 32 and st.chunk_bytes.offset == 64
    assert (st.frame_bytes.offset, st.crc_bytes.offset, st.aes_bytes.offset) == (96, 104, 112)
    assert re.search(r"uint64_t blobs\[4\];.*\n\s+uint64_t blob_bytes\[4\];.*\n\s+uint64_t chunk_bytes\[4\];.*\n\s+uint64_t frame_bytes;.*\n"
                     r"\s+uint64_t crc_bytes;.*\n\s+uint64_t aes_bytes;.*\n\} pbsgpu_encode_stats3;", hdr)
    # no new engine option and no ABI bump
    assert re.search(r"^#define PBSGPU_ABI_VERSION 5\b", hdr, flags=re.M) and L.pbsgpu_abi_version() == 5
    assert C.sizeof(_lib.EngineOptions) == 96
    # the section holds the decisions and names what is left
    sec = hdr[hdr.index("---- encrypted data blobs written on the device"):hdr.index("int pbsgpu_blob_encode3_device")]
    for text in ("NO counter", "two of the nseg IVs are equal", "ACROSS calls", "os.urandom", "crypto/rand", "CIPHERTEXT",
                 "ONE synchronisation", "timing channel", "SHA-256(content || id_key)", "key-file KDF", "fused", "ring",
                 "4 GiB - 44", "NEXT.md", "never appears in a trace or an error string", "not compacted"):
        assert text in sec, text
    # the key is a secret: no environment variable, no trace or error text carries it
    unit = _read("pbs_plus_amd", "csrc", "aes_encode.hip")
    assert "getenv" not in unit and "printf" not in unit


def test_python_cpp_and_go_surfaces():
    from pbs_plus_amd import Engine

    sig = inspect.signature(Engine.blob_encode3).parameters
    assert list(sig) == ["self", "src", "chunks", "key", "ivs", "dst", "nbytes", "zstd", "aes"]
    assert sig["key"].default is None and sig["ivs"].default is None and sig["zstd"].default is True and sig["aes"].default is None
    assert "os.urandom(16 * n)" in inspect.getsource(Engine.blob_encode3)
    hpp, go, fb = _read("include", "pbsgpu.hpp"), _read("go", "pbsgpu", "pbsgpu.go"), _read("go", "pbsgpu", "fallback.go")
    blob_ns = hpp[hpp.index("namespace blob {"):hpp.index("}  // namespace blob")]
    assert re.search(r"\bResult<Encoded3> Encode3\(", blob_ns) and "pbsgpu_blob_encode3_device(" in blob_ns
    assert re.search(r"\bC\.pbsgpu_blob_encode3_device\(", go) and '"crypto/rand"' in go and "rand.Read(ivs)" in go
    for text in (go, fb):
        for pat in (r"^type EncodeStats3 struct", r"^type Encoded3 struct", r"^func \(e \*Engine\) EncodeBlobs3\("):
            assert re.search(pat, text, flags=re.M), pat
    sig_go = re.search(r"^func \(e \*Engine\) EncodeBlobs3\((.*?)\) \(Encoded3, error\)", go, flags=re.M | re.S).group(1)
    assert [w.strip().split()[-1] for w in sig_go.replace("\n", " ").split(",")] == \
        ["unsafe.Pointer", "uint64", "offsets", "[]uint64", "bool", "*AesKey", "[]byte", "unsafe.Pointer", "uint64"]
    assert ("func (e *Engine) EncodeBlobs3(unsafe.Pointer, uint64, []uint64, []uint64, bool, *AesKey, []byte, unsafe.Pointer, uint64) "
            "(Encoded3, error)") in fb
    body = fb[fb.index("func (e *Engine) EncodeBlobs3("):]
    assert "ErrNotBuilt" in body[:body.index("}\n")]


def test_the_cpp_mirror_compiles():
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), "-x", "c++",
                          os.path.join(ROOT, "include", "pbsgpu.hpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]


class Args:
    """one call's arguments on pointers that are never dereferenced; the outputs are pre-filled and checked untouched.
    A pbsgpu_aes_key begins with its engine: the stand-in for a key points at the stand-in for the engine, so that the
    checks behind "a key of another engine" are reached."""

    def __init__(self):
        self.eng_buf = C.create_string_buffer(4096)
        self.eng = C.cast(self.eng_buf, C.c_void_p)
        self.key_buf = C.create_string_buffer(4096)
        C.memmove(self.key_buf, C.byref(C.c_uint64(self.eng.value)), 8)
        self.key = C.cast(self.key_buf, C.c_void_p)
        self.foreign_buf = C.create_string_buffer(4096)  # its engine is NULL
        self.foreign = C.cast(self.foreign_buf, C.c_void_p)
        self.src, self.dst = 0x10000000, 0x20000000
        self.segs = np.array([[0, 100], [100, 50]], dtype=np.uint64)
        self.ivs = np.arange(32, dtype=np.uint8)
        self.reset()

    def reset(self):
        self.offs = np.full(3, 77, dtype=np.uint64)
        self.lens = np.full(2, 9, dtype=np.uint32)
        self.kinds = np.full(2, 9, dtype=np.uint8)
        self.crcs = np.full(2, 9, dtype=np.uint32)

    def untouched(self, offsets=True):
        return ((not offsets or np.all(self.offs == 77)) and np.all(self.lens == 9) and np.all(self.kinds == 9)
                and np.all(self.crcs == 9))


def test_refusals_that_need_no_device(L):
    """every refusal that is decided before the runtime is touched"""
    from pbs_plus_amd import _lib

    E = _lib.E_INVALID
    a = Args()
    f = L.pbsgpu_blob_encode3_device
    NOKEY = object()

    def call(eng=a.eng, sp=a.src, nbytes=1024, sg=a.segs, n=2, flags=2, key=a.key, iv=a.ivs, dp=a.dst, cap=238):
        p = lambda v: None if v is None else v.ctypes.data  # noqa: E731
        return f(eng, sp, nbytes, p(sg), n, flags, None if key is NOKEY else key, p(iv), dp, cap, a.offs.ctypes.data,
                 a.lens.ctypes.data, a.kinds.ctypes.data, a.crcs.ctypes.data, None)

    for flags in (2, 3):
        # encode2's refusals
        assert call(eng=None, flags=flags) == E and call(sp=None, flags=flags) == E and call(sg=None, flags=flags) == E
        assert call(nbytes=149, flags=flags) == E
        assert call(sg=np.array([[1 << 63, 1 << 63], [0, 1]], dtype=np.uint64), flags=flags) == E
        # the key, the IVs
        assert call(key=NOKEY, flags=flags) == E                 # F_AES without a key
        assert call(key=a.foreign, flags=flags) == E             # a key of another engine
        assert call(iv=None, flags=flags) == E
        dup = a.ivs.copy()
        dup[16:] = dup[:16]
        assert call(iv=dup, flags=flags) == E and call(iv=dup, cap=0, flags=flags) == E  # (before the capacity is looked at)
        # a chunk of 4 GiB - 44 or more: lens is 32 bits wide
        big = np.array([[0, (1 << 32) - 44], [0, 1]], dtype=np.uint64)
        assert call(sg=big, nbytes=1 << 40, cap=1 << 41, flags=flags) == E
        assert a.untouched(), flags
        # the capacity: offsets is filled in first, nothing else is
        assert call(cap=237, flags=flags) == _lib.E_CAPACITY and list(a.offs) == [0, 144, 238]  # slots of 44 + length
        assert a.untouched(offsets=False)
        a.reset()
        fits = np.array([[0, (1 << 32) - 45], [0, 1]], dtype=np.uint64)  # the longest chunk that is taken
        assert call(sg=fits, nbytes=1 << 40, cap=0, flags=flags) == _lib.E_CAPACITY
        assert list(a.offs) == [0, (1 << 32) - 1, (1 << 32) + 44]
        a.reset()
        # dst: NULL, or overlapping the source (a frame is encrypted where it lies)
        assert call(dp=None, flags=flags) == E
        assert call(sp=a.dst - 1000, dp=a.dst, flags=flags) == E and call(sp=a.dst + 237, dp=a.dst, flags=flags) == E
        assert a.untouched(offsets=False)
        a.reset()
        assert call(n=0, sg=None, iv=None, dp=None, cap=0, sp=None, nbytes=0, flags=flags) == _lib.OK
        a.reset()
    for flags in (4, 6, 8, 1 << 31, 0xFFFFFFFF):
        assert call(flags=flags) == E and call(flags=flags, key=NOKEY, iv=None) == E, flags
    assert a.untouched()
    # the host-only size: 12 or 44 per chunk
    total = C.c_uint64(5)
    g = L.pbsgpu_blob_encoded_size3
    assert g(a.segs.ctypes.data, 2, 0, C.byref(total)) == _lib.OK and total.value == 174
    assert g(a.segs.ctypes.data, 2, 1, C.byref(total)) == _lib.OK and total.value == 174
    assert g(a.segs.ctypes.data, 2, 2, C.byref(total)) == _lib.OK and total.value == 238
    assert g(a.segs.ctypes.data, 2, 3, C.byref(total)) == _lib.OK and total.value == 238
    assert g(None, 0, 2, C.byref(total)) == _lib.OK and total.value == 0
    assert g(a.segs.ctypes.data, 2, 4, C.byref(total)) == E and g(None, 2, 2, C.byref(total)) == E
    assert g(a.segs.ctypes.data, 2, 2, None) == E
    wraps = np.array([[0, (1 << 64) - 20]], dtype=np.uint64)
    assert g(wraps.ctypes.data, 1, 2, C.byref(total)) == E
    old = C.c_uint64()
    assert L.pbsgpu_blob_encoded_size(a.segs.ctypes.data, 2, C.byref(old)) == _lib.OK and old.value == 174


def test_without_the_flag_the_argument_checks_are_encode2s(L):
    """flags 0 and F_ZSTD: the same answers and the same outputs as pbsgpu_blob_encode2_device, key and IVs not looked at"""
    a, b = Args(), Args()
    f3, f2 = L.pbsgpu_blob_encode3_device, L.pbsgpu_blob_encode2_device
    junk = 0x30000000  # stands for a key and for IVs: never dereferenced

    def both(eng="fake", sp=a.src, nbytes=1024, sg=a.segs, n=2, flags=0, dp=a.dst, cap=174):
        p = lambda v: None if v is None else v.ctypes.data  # noqa: E731
        r3 = f3(a.eng if eng == "fake" else eng, sp, nbytes, p(sg), n, flags, junk, junk, dp, cap, a.offs.ctypes.data,
                a.lens.ctypes.data, a.kinds.ctypes.data, a.crcs.ctypes.data, None)
        r2 = f2(b.eng if eng == "fake" else eng, sp, nbytes, p(sg), n, flags, dp, cap, b.offs.ctypes.data, b.lens.ctypes.data,
                b.kinds.ctypes.data, b.crcs.ctypes.data, None)
        assert r3 == r2, (r3, r2)
        assert np.array_equal(a.offs, b.offs) and np.array_equal(a.lens, b.lens) and np.array_equal(a.kinds, b.kinds)
        assert np.array_equal(a.crcs, b.crcs)
        return r3

    from pbs_plus_amd import _lib

    E = _lib.E_INVALID
    for flags in (0, 1):
        assert both(eng=None, flags=flags) == E and both(sp=None, flags=flags) == E and both(sg=None, flags=flags) == E
        assert both(nbytes=149, flags=flags) == E
        assert both(cap=173, flags=flags) == _lib.E_CAPACITY and list(a.offs) == [0, 112, 174]  # slots of 12 + length
        big = np.array([[0, (1 << 32) - 12], [0, 1]], dtype=np.uint64)
        assert both(sg=big, nbytes=1 << 40, cap=1 << 41, flags=flags) == E
        almost = np.array([[0, (1 << 32) - 44], [0, 1]], dtype=np.uint64)  # refused with F_AES, taken without
        assert both(sg=almost, nbytes=1 << 40, cap=0, flags=flags) == _lib.E_CAPACITY
        assert both(n=0, sg=None, dp=None, cap=0, sp=None, nbytes=0, flags=flags) == _lib.OK
    assert both(dp=None, flags=1) == E


def _guard(usage, text, k):
    names = [n for n in usage if re.search(r"\d%s[A-Z]" % k, n)]
    assert len(names) == 1, (k, list(usage))
    r = usage[names[0]]
    assert r.get("scratch", -1) == 0 and r.get("sgpr_spill", -1) == 0 and r.get("vgpr_spill", -1) == 0, (k, r)
    assert 0 <= r.get("lds", -1) <= LDS_BUDGET, (k, r)
    body = _body(text, names[0])
    assert not [ln for ln in body if re.match(r"\s+flat_", ln)], k
    assert not [ln for ln in body if re.match(r"\s+scratch_", ln)], k
    assert [ln for ln in body if re.match(r"\s+global_", ln)], k
    return r, body


def test_the_kernels_do_not_spill_use_no_flat_memory_instructions_and_keep_to_the_lds_budget(tmp_path):
    usage, text = _compile(tmp_path, "aes_encode")
    assert len(usage) == len(AES_KERNELS), list(usage)
    got = {k: _guard(usage, text, k) for k in AES_KERNELS}
    pieces, body = got["k_aese_pieces"]
    assert pieces["lds"] >= 1024 + 1024 + 4096 and got["k_aese_head"][0]["lds"] >= 1024  # the AES table, the reductions, H^256's
    assert [ln for ln in body if re.match(r"\s+ds_read_b128", ln)]         # a multiplier entry is one 16-byte LDS read
    assert [ln for ln in body if re.match(r"\s+global_load_dwordx4", ln)]  # the payload moves in 16-byte loads and stores
    assert [ln for ln in body if re.match(r"\s+global_store_dwordx4", ln)]
    mk = _read("pbs_plus_amd", "csrc", "Makefile")
    assert "$(OBJ)/aes_encode.o" in mk.split("OBJS :=")[1].split("\n")[0] and "aes_encode.hip" in mk.split("SRCS :=")[1].split("\n")[0]
    assert re.search(r"^\$\(OBJ\)/aes_encode\.o: aes_encode\.hip aes_gcm\.h engine_internal\.h blob_plan\.h", mk, flags=re.M)
    # the unit compiles the one format core and holds no cipher of its own
    unit = _read("pbs_plus_amd", "csrc", "aes_encode.hip")
    assert '#include "aes_gcm.h"' in unit and "pbsa::piece_lane(" in unit and "pbsa::fold_piece(" in unit and "pbsa::tag_of(" in unit


def test_the_new_crc_pair_of_blob_hip(tmp_path):
    usage, text = _compile(tmp_path, "blob")
    for k in CRC_KERNELS:
        r, body = _guard(usage, text, k)
    pieces, body = _guard(usage, text, "k_enc3_pieces")
    assert pieces["lds"] == 17 * 1024  # the sixteen slice tables and the byte table, as in every piece kernel
    assert [ln for ln in body if re.match(r"\s+global_load_dwordx4", ln)]
    assert not [ln for ln in body if re.match(r"\s+global_store_dwordx[34]", ln)]  # the walk stores nothing: the ciphertext lies there
