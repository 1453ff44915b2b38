"""The surface of AES-256-GCM without a GPU: the C ABI additions (pbsgpu_aes_key_create, pbsgpu_aes_key_destroy,
pbsgpu_aes_gcm_many_device, pbsgpu_blob_decode3_device), their bindings in Python, the C++ mirror, Go and the Go fallback,
the refusals that come before any device work, and the build-quality guard for the kernels of aes_gcm.hip (no spills, no
scratch, no flat_* instructions, LDS within the budget of eight workgroups per CU) with the unit listed in the Makefile."""
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
NARGS = {"pbsgpu_aes_key_create": 3, "pbsgpu_aes_key_destroy": 1, "pbsgpu_aes_gcm_many_device": 13, "pbsgpu_blob_decode3_device": 16}
KERNELS = ("k_aes_head", "k_aes_pieces", "k_aes_fold", "k_aes_zero", "k_aesr_select", "k_aesr_frames", "k_aesr_merge", "k_aesr_status")
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
    assert re.search(r"^int pbsgpu_aes_key_create\s*\(", hdr, flags=re.M) and re.search(r"^void pbsgpu_aes_key_destroy\s*\(", hdr, flags=re.M)
    assert re.search(r"^int pbsgpu_aes_gcm_many_device\s*\(", hdr, flags=re.M)
    assert re.search(r"^int pbsgpu_blob_decode3_device\s*\(", hdr, flags=re.M)
    assert re.search(r"^typedef struct pbsgpu_aes_key pbsgpu_aes_key;", hdr, flags=re.M)
    for name, n in NARGS.items():
        assert name in exported and name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == n, name
        assert getattr(L, name).argtypes is not None
    for name, val in (("PBSGPU_HAS_AES_GCM", "1"), ("PBSGPU_AES_OK", "0"), ("PBSGPU_AES_BAD_TAG", "1"), ("PBSGPU_AES_F_ENCRYPT", "1u")):
        assert re.search(r"^#define %s %s\b" % (name, val), hdr, flags=re.M), name
    for name, val in (("PBSGPU_DECODE_F_AES", "4u"), ("PBSGPU_BLOB_BAD_TAG", "7")):
        assert re.search(r"^#define %s %s\b" % (name, val), hdr, flags=re.M), name
    assert (_lib.AES_OK, _lib.AES_BAD_TAG, _lib.AES_F_ENCRYPT) == (0, 1, 1)
    assert (_lib.DECODE_F_AES, _lib.BLOB_BAD_TAG, _lib.BLOB_STATUS_NAMES3[7]) == (4, 7, "bad_tag")
    assert C.sizeof(_lib.DecodeStats3) == C.sizeof(_lib.DecodeStats2) + 8 and _lib.DecodeStats3.aes_bytes.offset == 112
    d3 = hdr[hdr.index("Restore with the encrypted blobs decrypted"):hdr.index("int pbsgpu_blob_decode3_device")]
    assert "magic, header, CRC,\n * tag" in d3 and "ZERO where the blob was" in d3 and "UNTOUCHED otherwise" in d3
    assert "SHA-256(content || id_key)" in d3 and "ONE synchronisation" in d3 and "PBSGPU_BLOB_CRC_ONLY" in d3
    # no new engine option and no ABI bump
    assert re.search(r"^#define PBSGPU_ABI_VERSION 5\b", hdr, flags=re.M) and L.pbsgpu_abi_version() == 5
    assert C.sizeof(_lib.EngineOptions) == 96
    # the section names the reference's call site, the decisions and what is left
    sec = hdr[hdr.index("---- AES-256-GCM on the device"):hdr.index("int pbsgpu_aes_gcm_many_device")]
    assert "cmd/pxar-mount/main.go:43" in sec and "[EXTERNAL]" in sec and "ONE synchronisation" in sec
    assert "timing" in sec and "ZEROED" in sec and "GHASH(IV || 0^64 || [128]_64)" in sec and "wipes the host copy" in sec
    assert "PBSGPU_BLOB_CRC_ONLY" in sec and "NEXT.md" in sec
    # the key is a secret: no option, no environment variable, no trace or error text carries it
    unit = _read("pbs_plus_amd", "csrc", "aes_gcm.hip")
    assert "getenv" not in unit and "printf" not in unit and "fprintf" not in unit


def test_python_cpp_and_go_surfaces():
    import pbs_plus_amd
    from pbs_plus_amd import AesKey, Engine

    sig = inspect.signature(Engine.aes_gcm_many).parameters
    assert list(sig)[:5] == ["self", "key", "data", "messages", "ivs"] and sig["encrypt"].default is False and sig["tags"].default is None
    assert list(inspect.signature(AesKey.__init__).parameters) == ["self", "eng", "key"]
    assert "AesKey" in pbs_plus_amd.__all__
    with pytest.raises(ValueError):
        AesKey(None, b"short")  # (decided before the engine is looked at)
    hpp, go, fb = _read("include", "pbsgpu.hpp"), _read("go", "pbsgpu", "pbsgpu.go"), _read("go", "pbsgpu", "fallback.go")
    blob_ns = hpp[hpp.index("namespace blob {"):hpp.index("}  // namespace blob")]
    assert re.search(r"\bclass AesKey\b", blob_ns) and re.search(r"\bResult<AesResult> AesGcmMany\(", blob_ns)
    assert re.search(r"\bResult<Decoded3> Decode3\(", blob_ns)
    sig = inspect.signature(Engine.blob_decode3).parameters
    assert list(sig)[:4] == ["self", "data", "blobs", "idx"] and sig["key"].default is None and sig["aes"].default is None
    for name in NARGS:
        assert name + "(" in blob_ns, name
        assert re.search(r"\bC\.%s\(" % name, go), name
    for text in (go, fb):
        for pat in (r"^type AesKey struct", r"^func \(e \*Engine\) NewAesKey\(", r"^func \(k \*AesKey\) Close\(\)",
                    r"^func \(k \*AesKey\) AesGcmMany\(", r"^\tAesBadTag\s+= 1\b", r"^\tAesFlagEncrypt = 1$",
                    r"^func \(e \*Engine\) DecodeBlobs3\(", r"^const BlobBadTag = 7$", r"^type DecodeStats3 struct"):
            assert re.search(pat, text, flags=re.M), pat
    for fn in ("func (e *Engine) NewAesKey(", "func (k *AesKey) AesGcmMany(", "func (e *Engine) DecodeBlobs3("):
        body = fb[fb.index(fn):]
        assert "ErrNotBuilt" in body[:body.index("}\n")], fn


def test_the_cpp_mirror_compiles():
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), "-x", "c++",
                          os.path.join(ROOT, "include", "pbsgpu.hpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]


def test_refusals_that_need_no_device(L):
    """every PBSGPU_E_INVALID that is decided before the runtime is touched, on pointers that are never dereferenced"""
    from pbs_plus_amd import _lib

    E = _lib.E_INVALID
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)  # stands for a key: the refusals come before it is looked into
    src, dst = 0x10000000, 0x20000000
    segs = np.array([[0, 100], [100, 50]], dtype=np.uint64)
    out = np.array([[0, 300], [300, 200]], dtype=np.uint64)
    ivs, tags, status = np.zeros(32, np.uint8), np.full(32, 7, np.uint8), np.full(2, 9, np.uint8)
    f = L.pbsgpu_aes_gcm_many_device

    def call(key=fake, sp=src, nbytes=1024, sg=segs, n=2, iv=ivs, ivl=16, tg=tags, o=out, dp=dst, cap=500, stat=status, flags=0):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return f(key, sp, nbytes, p(sg), n, p(iv), ivl, p(tg), p(o), dp, cap, p(stat), flags)

    for flags in (0, 1):
        assert call(key=None, flags=flags) == E
        assert call(sp=None, flags=flags) == E and call(sg=None, flags=flags) == E and call(o=None, flags=flags) == E
        assert call(iv=None, flags=flags) == E and call(tg=None, flags=flags) == E
        assert call(stat=None, flags=flags) == E and call(dp=None, flags=flags) == E
        assert call(nbytes=149, flags=flags) == E and call(cap=499, flags=flags) == E
        for ivl in (0, 8, 11, 13, 15, 17, 60):
            assert call(ivl=ivl, flags=flags) == E, ivl
        assert call(o=np.array([[0, 300], [299, 200]], dtype=np.uint64), flags=flags) == E   # the rooms share byte 299
        assert call(o=np.array([[0, 99], [300, 200]], dtype=np.uint64), flags=flags) == E    # a room shorter than its message
        big = np.array([[0, 1 << 32], [0, 1]], dtype=np.uint64)                              # a message of 4 GiB
        assert call(sg=big, o=big, nbytes=1 << 40, cap=1 << 40, flags=flags) == E
        assert call(sp=dst - 1000, dp=dst, flags=flags) == E                                 # dst begins inside the source
        assert call(n=0, sg=None, iv=None, tg=None, o=None, stat=None, dp=None, cap=0, sp=None, nbytes=0, flags=flags) == _lib.OK
    for flags in (2, 4, 1 << 31, 0xFFFFFFFF):
        assert call(flags=flags) == E, flags
    assert np.all(status == 9) and np.all(tags == 7)
    # decode3: an unknown flag, and F_AES without a key, before anything else is looked at
    d3 = L.pbsgpu_blob_decode3_device
    rec = np.zeros(1, dtype=_lib.RECORD_DTYPE)
    rec["end"], rec["size"] = 100, 100
    blob = np.array([[0, 112]], dtype=np.uint64)
    st1 = np.full(1, 9, np.uint8)
    for flags, k in ((8, fake), (1 << 31, fake), (4, None), (7, None)):
        assert d3(fake, src, 1024, blob.ctypes.data, 1, rec.ctypes.data, 1, None, 0, 100, flags, k, dst, 100, st1.ctypes.data, None) == E
    assert st1[0] == 9
    h = C.c_void_p(5)
    key = (C.c_uint8 * 32)()
    assert L.pbsgpu_aes_key_create(None, key, C.byref(h)) == E and L.pbsgpu_aes_key_create(fake, None, C.byref(h)) == E
    assert L.pbsgpu_aes_key_create(fake, key, None) == E
    L.pbsgpu_aes_key_destroy(None)


def test_the_kernels_do_not_spill_use_no_flat_memory_instructions_and_keep_to_the_lds_budget(tmp_path):
    usage, text = _compile(tmp_path, "aes_gcm")
    assert len(usage) == len(KERNELS), list(usage)
    for k in KERNELS:
        names = [n for n in usage if re.search(r"\d%s[A-Z]" % k, n)]
        assert len(names) == 1, (k, list(usage))
        r = usage[names[0]]
        assert r.get("scratch", -1) == 0 and r.get("sgpr_spill", -1) == 0 and r.get("vgpr_spill", -1) == 0, (k, r)
        assert 0 <= r.get("lds", -1) <= LDS_BUDGET, (k, r)
        body = _body(text, names[0])
        assert not [ln for ln in body if re.match(r"\s+flat_", ln)], k
        assert not [ln for ln in body if re.match(r"\s+scratch_", ln)], k
        assert [ln for ln in body if re.match(r"\s+global_", ln)], k
    pieces = usage[[n for n in usage if "k_aes_pieces" in n][0]]
    head = usage[[n for n in usage if "k_aes_head" in n][0]]
    assert pieces["lds"] >= 1024 + 1024 + 4096 and head["lds"] >= 1024  # the AES table, the reductions, the table of H^256
    body = _body(text, [n for n in usage if "k_aes_pieces" in n][0])
    assert [ln for ln in body if re.match(r"\s+ds_read_b128", ln)]         # a multiplier entry is one 16-byte LDS read
    assert [ln for ln in body if re.match(r"\s+global_load_dwordx4", ln)]  # the payload moves in 16-byte loads and stores
    assert [ln for ln in body if re.match(r"\s+global_store_dwordx4", ln)]
    mk = _read("pbs_plus_amd", "csrc", "Makefile")
    assert "$(OBJ)/aes_gcm.o" in mk.split("OBJS :=")[1].split("\n")[0] and "aes_gcm.hip" in mk.split("SRCS :=")[1].split("\n")[0]
    assert re.search(r"^\$\(OBJ\)/aes_gcm\.o: aes_gcm\.hip aes_gcm\.h", mk, flags=re.M)
