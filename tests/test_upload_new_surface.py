"""Classify and frame in one device-side call (pbsgpu_ring_upload_new_device / pbsgpu_known_upload_new_device) without a
GPU: the C ABI and the Python / C++ / Go surfaces, the argument checks that come before any device work, and the
build-quality guard for the plan kernels the feature adds to blob.hip (no scratch, no spills, no flat_* instructions) with
every earlier kernel of blob.hip and known.hip still there exactly once."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pbsgpu_ring_upload_new_device", "pbsgpu_known_upload_new_device")
NEW_KERNELS = ("k_upnew_count", "k_upnew_scan", "k_upnew_fill", "k_upnew_ppart")
BLOB_KERNELS = ("k_pagecrc_pieces", "k_pagecrc_fold", "k_page_copy", "k_crc_pieces", "k_crc_fold", "k_blob_heads")
KNOWN_KERNELS = ("k_known_lookup", "k_known_keys", "k_known_mark", "k_known_insert", "k_known_rehash")


@pytest.fixture(scope="module")
def L():
    from pbs_plus_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_new_names_are_declared_exported_and_bound(L):
    from pbs_plus_amd import _lib

    hdr = _read("include", "pbsgpu.h")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pbsgpu_[a-z0-9_]+)", out))
    for name in SYMBOLS:
        assert re.search(r"^int %s\s*\(" % name, hdr, flags=re.M), name
        assert name in exported, name
        assert name in _lib.SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    assert len(_lib.SYMBOLS["pbsgpu_ring_upload_new_device"][1]) == 13
    assert len(_lib.SYMBOLS["pbsgpu_known_upload_new_device"][1]) == 14
    assert re.search(r"^#define PBSGPU_HAS_UPLOAD_NEW 1\b", hdr, flags=re.M)
    assert re.search(r"^#define PBSGPU_ABI_VERSION 5\b", hdr, flags=re.M)
    assert L.pbsgpu_abi_version() == 5
    # each entry point names the reference call sites it stands behind
    sec = hdr[hdr.index("---- classify and frame in one device-side call"):hdr.index("int pbsgpu_known_upload_new_device")]
    assert "commit_orchestrate.go:137-158" in sec and "commit_reuse.go:315-341" in sec


def test_python_cpp_and_go_surfaces():
    import inspect

    from pbs_plus_amd import KnownChunks, PageRing

    sig = inspect.signature(PageRing.upload_new).parameters
    assert list(sig)[:4] == ["self", "known", "stream", "recs"] and sig["insert"].default is True and sig["dst"].default is None
    sig = inspect.signature(KnownChunks.upload_new).parameters
    assert list(sig)[:4] == ["self", "src", "recs", "chunks"] and sig["insert"].default is True
    hpp = _read("include", "pbsgpu.hpp")
    go = _read("go", "pbsgpu", "pbsgpu.go")
    fb = _read("go", "pbsgpu", "fallback.go")
    for name in SYMBOLS:
        assert name + "(" in hpp, name
        assert re.search(r"\bC\.%s\(" % name, go), name
    assert len(re.findall(r"\bUploadNew\(", hpp)) == 2
    for sig in (r"^func \(r \*Ring\) UploadNew\(", r"^func \(k \*KnownChunks\) UploadNew\("):
        assert re.search(sig, go, flags=re.M), sig
        assert re.search(sig, fb, flags=re.M), sig
    assert re.search(r"^type Uploaded struct", go, flags=re.M) and re.search(r"^\tUploaded\s+struct", fb, flags=re.M)


def test_argument_checks_that_need_no_device(L):
    """a NULL ring, a NULL set, NULL where a result must go, n >= 2^32: PBSGPU_E_INVALID before anything is looked at"""
    from pbs_plus_amd import RECORD_DTYPE, _lib

    E = _lib.E_INVALID
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)  # never dereferenced: the bad argument is found first
    recs = np.zeros(2, dtype=RECORD_DTYPE)
    chunks = np.zeros((2, 2), dtype=np.uint64)
    offs = np.zeros(2, dtype=np.uint64)
    used, st = C.c_uint64(), _lib.DedupStats()
    ring = L.pbsgpu_ring_upload_new_device
    rp, op, up, sp = recs.ctypes.data, offs.ctypes.data, C.byref(used), C.byref(st)
    assert ring(None, fake, 0, rp, 2, 1, None, 0, None, op, None, up, sp) == E
    assert ring(fake, None, 0, rp, 2, 1, None, 0, None, op, None, up, sp) == E
    assert ring(fake, fake, 0, rp, 2, 1, None, 0, None, op, None, None, sp) == E
    assert ring(fake, fake, 0, rp, 2, 1, None, 0, None, None, None, up, sp) == E
    assert ring(fake, fake, 0, None, 2, 1, None, 0, None, op, None, up, sp) == E
    assert ring(fake, fake, 0, rp, 2, 1, None, 0, None, op, None, up, None) == E
    assert ring(fake, fake, 0, rp, 1 << 32, 1, None, 0, None, op, None, up, sp) == E
    cont = L.pbsgpu_known_upload_new_device
    cp = chunks.ctypes.data
    assert cont(None, None, 0, rp, cp, 2, 1, None, 0, None, op, None, up, sp) == E
    assert cont(fake, None, 0, rp, cp, 2, 1, None, 0, None, op, None, None, sp) == E
    assert cont(fake, None, 0, rp, cp, 2, 1, None, 0, None, None, None, up, sp) == E
    assert cont(fake, None, 0, rp, None, 2, 1, None, 0, None, op, None, up, sp) == E
    assert cont(fake, None, 0, None, cp, 2, 1, None, 0, None, op, None, up, sp) == E
    assert cont(fake, None, 0, rp, cp, 1 << 32, 1, None, 0, None, op, None, up, sp) == E
    assert cont(fake, None, 16, rp, cp, 2, 1, None, 0, None, op, None, up, sp) == E       # bytes without a source
    assert cont(fake, None, 0, rp, cp, 2, 1, None, 64, None, op, None, up, sp) == E       # room without a destination
    chunks[1] = (0, 1)                                                                     # a chunk outside the source
    assert cont(fake, None, 0, rp, cp, 2, 1, None, 0, None, op, None, up, sp) == E


def _compile(tmp_path, name):
    """the method of tests/test_ring_upload_surface.py: (resource usage per kernel, assembly text)"""
    src = os.path.join(ROOT, "pbs_plus_amd", "csrc", name + ".hip")
    asm = str(tmp_path / (name + ".s"))
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
    return usage, open(asm).read()


def _body(text, name):
    m = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape(name), text, flags=re.S | re.M)
    assert m, name
    return m.group(1).splitlines()


def test_plan_kernels_do_not_spill_and_use_no_flat_memory_instructions(tmp_path):
    usage, text = _compile(tmp_path, "blob")
    for k in NEW_KERNELS + BLOB_KERNELS:
        names = [n for n in usage if k in n]
        assert len(names) == 1, (k, list(usage))
    for k in NEW_KERNELS:
        assert not [e for e in BLOB_KERNELS + KNOWN_KERNELS if e in k], k
        name = [n for n in usage if k in n][0]
        r = usage[name]
        assert r.get("scratch", -1) == 0 and r.get("sgpr_spill", -1) == 0 and r.get("vgpr_spill", -1) == 0, (k, r)
        body = _body(text, name)
        assert not [ln for ln in body if re.match(r"\s+flat_", ln)], k
        assert not [ln for ln in body if re.match(r"\s+scratch_", ln)], k
        assert [ln for ln in body if re.match(r"\s+global_", ln)], k
    # the CRC pair reads its counts from device memory when the plan was built there, and still uses no flat access
    for k in ("k_pagecrc_pieces", "k_pagecrc_fold"):
        name = [n for n in usage if k in n][0]
        r = usage[name]
        assert r.get("scratch", -1) == 0 and r.get("sgpr_spill", -1) == 0 and r.get("vgpr_spill", -1) == 0, (k, r)
        assert not [ln for ln in _body(text, name) if re.match(r"\s+flat_", ln)], k


def test_known_kernels_are_still_one_each(tmp_path):
    usage, _ = _compile(tmp_path, "known")
    for k in KNOWN_KERNELS:
        assert len([n for n in usage if k in n]) == 1, (k, list(usage))
    assert not [n for n in usage if "k_upnew" in n]
