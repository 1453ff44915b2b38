"""The known-chunk set (pbsgpu_known_*) without a GPU: the C ABI, the Python / C++ / Go bindings and the argument checks
that come before any device work, plus the build-quality guard for its kernels (known.hip is not part of the
`make usage` resource report of test_kernel_resources.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN_SYMBOLS = ("pbsgpu_known_create", "pbsgpu_known_destroy", "pbsgpu_known_count", "pbsgpu_known_add_host",
                 "pbsgpu_known_add_device", "pbsgpu_known_add_didx", "pbsgpu_known_classify_host",
                 "pbsgpu_known_classify_device")
KERNELS = ("k_known_lookup", "k_known_keys", "k_known_mark", "k_known_insert", "k_known_rehash")


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
    for name in KNOWN_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in exported, name
        assert name in _lib.SYMBOLS, name
        assert getattr(L, name).argtypes is not None or _lib.SYMBOLS[name][1] == [], name


def test_feature_macro_and_abi_version():
    hdr = _header()
    assert re.search(r"^#define PBSGPU_HAS_KNOWN_SET 1\b", hdr, flags=re.M)
    assert re.search(r"^#define PBSGPU_ABI_VERSION 5\b", hdr, flags=re.M)  # additive: the version stays


def test_python_class_is_exported():
    import pbs_plus_amd
    from pbs_plus_amd import KnownChunks

    assert "KnownChunks" in pbs_plus_amd.__all__
    for m in ("add", "add_device", "add_didx", "classify", "classify_device", "close", "__len__"):
        assert callable(getattr(KnownChunks, m)), m


def test_go_binding_calls_the_entry_points_and_fallback_mirrors_them():
    go = open(os.path.join(ROOT, "go", "pbsgpu", "pbsgpu.go")).read()
    fb = open(os.path.join(ROOT, "go", "pbsgpu", "fallback.go")).read()
    for name in ("pbsgpu_known_create", "pbsgpu_known_destroy", "pbsgpu_known_count", "pbsgpu_known_add_host",
                 "pbsgpu_known_add_didx", "pbsgpu_known_classify_host"):
        assert re.search(r"\bC\.%s\(" % name, go), name
    assert re.search(r"^func \(e \*Engine\) NewKnownChunks\(", go, flags=re.M)
    assert re.search(r"^func \(e \*Engine\) NewKnownChunks\(", fb, flags=re.M)
    for meth in ("Add", "AddDynamicIndex", "Classify", "Len", "Close"):
        assert re.search(r"^func \(k \*KnownChunks\) %s\(" % meth, go, flags=re.M), meth
        assert re.search(r"^func \(k \*KnownChunks\) %s\(" % meth, fb, flags=re.M), meth
    assert "func (k *KnownChunks) Classify(recs []ChunkInfo, insert bool) ([]bool, DedupStats, error)" in go


def test_cpp_mirror_has_the_set():
    hpp = open(os.path.join(ROOT, "include", "pbsgpu.hpp")).read()
    assert re.search(r"class KnownChunks\b", hpp)
    for fn in ("pbsgpu_known_create", "pbsgpu_known_add_didx", "pbsgpu_known_classify_host", "pbsgpu_known_destroy"):
        assert fn + "(" in hpp, fn


def test_argument_checks_need_no_device(L):
    from pbs_plus_amd import _lib

    E = _lib.E_INVALID
    h = C.c_void_p()
    n = C.c_uint64()
    st = _lib.DedupStats()
    rec = np.zeros(1, dtype=_lib.RECORD_DTYPE)
    flags = np.zeros(1, dtype=np.uint8)
    # NULL handle / out / stats
    assert L.pbsgpu_known_create(None, 0, C.byref(h)) == E
    assert L.pbsgpu_known_count(None, C.byref(n)) == E
    assert L.pbsgpu_known_add_host(None, rec.ctypes.data, 1) == E
    assert L.pbsgpu_known_add_device(None, None, 0) == E
    assert L.pbsgpu_known_add_didx(None, rec.ctypes.data, 48) == E
    assert L.pbsgpu_known_classify_host(None, rec.ctypes.data, 1, 1, flags.ctypes.data, C.byref(st)) == E
    assert L.pbsgpu_known_classify_device(None, None, 0, 0, None, C.byref(st)) == E
    L.pbsgpu_known_destroy(None)  # no-op
    # a non-NULL handle that is never looked at: every check below fails before the handle is used
    fake = C.create_string_buffer(256)
    assert L.pbsgpu_known_count(C.cast(fake, C.c_void_p), None) == E
    assert L.pbsgpu_known_classify_host(C.cast(fake, C.c_void_p), rec.ctypes.data, 1, 1, None, None) == E
    assert L.pbsgpu_known_classify_device(C.cast(fake, C.c_void_p), None, 1, 0, None, C.byref(st)) == E
    assert L.pbsgpu_known_add_host(C.cast(fake, C.c_void_p), None, 3) == E
    big = 1 << 32
    assert L.pbsgpu_known_add_host(C.cast(fake, C.c_void_p), rec.ctypes.data, big) == E
    assert L.pbsgpu_known_add_device(C.cast(fake, C.c_void_p), rec.ctypes.data, big) == E
    assert L.pbsgpu_known_classify_host(C.cast(fake, C.c_void_p), rec.ctypes.data, big, 1, None, C.byref(st)) == E
    assert L.pbsgpu_known_classify_device(C.cast(fake, C.c_void_p), rec.ctypes.data, big, 0, None, C.byref(st)) == E
    # a host pointer handed to the _device variants
    assert L.pbsgpu_known_add_device(C.cast(fake, C.c_void_p), rec.ctypes.data, 1) == E
    assert L.pbsgpu_known_classify_device(C.cast(fake, C.c_void_p), rec.ctypes.data, 1, 0, None, C.byref(st)) == E


def test_dedup_argument_checks_need_no_device(L):
    """pbsgpu_dedup_host / _device (the set's marking with no table): E_INVALID for a NULL engine, NULL stats, NULL
    records with n > 0, n >= 2^32 and a host pointer to the _device variant; n = 0 is OK with zeroed stats and touches
    neither the engine nor the device."""
    from pbs_plus_amd import _lib

    E = _lib.E_INVALID
    rec = np.zeros(1, dtype=_lib.RECORD_DTYPE)
    st = _lib.DedupStats()
    fake = C.cast(C.create_string_buffer(256), C.c_void_p)
    for fn in (L.pbsgpu_dedup_host, L.pbsgpu_dedup_device):
        assert fn(None, rec.ctypes.data, 1, None, C.byref(st)) == E
        assert fn(None, None, 0, None, C.byref(st)) == E
        assert fn(fake, rec.ctypes.data, 1, None, None) == E
        assert fn(fake, None, 3, None, C.byref(st)) == E
        assert fn(fake, rec.ctypes.data, 1 << 32, None, C.byref(st)) == E
        st.nrecords = st.nunique = st.total_bytes = st.unique_bytes = 7
        assert fn(fake, None, 0, None, C.byref(st)) == 0
        assert (st.nrecords, st.nunique, st.total_bytes, st.unique_bytes) == (0, 0, 0, 0)
    assert L.pbsgpu_dedup_device(fake, rec.ctypes.data, 1, None, C.byref(st)) == E


def _didx_parts(ends, digests):
    """(4096-byte header without its magic, the 40-byte entries) of a .didx image"""
    ent = np.zeros(len(ends), dtype=[("end", "<u8"), ("digest", "u1", (32,))])
    ent["end"] = ends
    ent["digest"] = digests
    return np.zeros(4096, dtype=np.uint8), ent.view(np.uint8).ravel()


def test_add_didx_validates_like_the_decoder_before_any_device_work(L):
    """add_didx rejects what pbsgpu_didx_decode rejects (bad magic, a body that is not whole 40-byte entries, ends that
    go backwards) — checked on the host before the handle is used."""
    from pbs_plus_amd import _lib

    fake = C.cast(C.create_string_buffer(256), C.c_void_p)
    hdr, ent = _didx_parts([100, 200, 300], np.arange(96, dtype=np.uint8).reshape(3, 32))
    for magic in (b"\0" * 8, b"PBSGPU!!"):
        blob = np.concatenate([np.frombuffer(magic, np.uint8), hdr[8:], ent])
        assert L.pbsgpu_known_add_didx(fake, blob.ctypes.data, blob.size) == _lib.E_INVALID
    short = np.zeros(100, dtype=np.uint8)
    assert L.pbsgpu_known_add_didx(fake, short.ctypes.data, short.size) == _lib.E_INVALID
    # with the real magic (Proxmox dynamic index v1.0): a ragged body, ends that go backwards, a chunk above 4 GiB
    magic = np.array([28, 145, 78, 165, 25, 186, 179, 205], dtype=np.uint8)
    digs = np.arange(96, dtype=np.uint8).reshape(3, 32)
    bad = []
    hdr, ent = _didx_parts([100, 200, 300], digs)
    bad.append(np.concatenate([magic, hdr[8:], ent, np.zeros(7, np.uint8)]))
    bad.append(np.concatenate([magic, hdr[8:], ent[:-1]]))
    hdr, ent = _didx_parts([100, 300, 200], digs)
    bad.append(np.concatenate([magic, hdr[8:], ent]))
    hdr, ent = _didx_parts([100, 200, 200 + (1 << 32) + 1], digs)
    bad.append(np.concatenate([magic, hdr[8:], ent]))
    n = C.c_uint64()
    out = np.zeros(8, dtype=_lib.RECORD_DTYPE)
    for blob in bad:
        assert L.pbsgpu_didx_decode(blob.ctypes.data, blob.size, out.ctypes.data, 8, C.byref(n), None, None) == _lib.E_INVALID
        assert L.pbsgpu_known_add_didx(fake, blob.ctypes.data, blob.size) == _lib.E_INVALID
    hdr, ent = _didx_parts([100, 200, 300], digs)  # (the same image, well formed, is what the decoder accepts)
    good = np.concatenate([magic, hdr[8:], ent])
    assert L.pbsgpu_didx_decode(good.ctypes.data, good.size, out.ctypes.data, 8, C.byref(n), None, None) == 0


def test_known_kernels_do_not_spill_and_use_no_flat_memory_instructions(tmp_path):
    """No scratch, no spills, and only global_* memory instructions in the kernels that touch the table."""
    src = os.path.join(ROOT, "pbs_plus_amd", "csrc", "known.hip")
    asm = str(tmp_path / "known.s")
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
