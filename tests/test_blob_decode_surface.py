"""Restore a stream from its index and data blobs (pbsgpu_blob_decode_device) without a GPU: the C ABI and the Python /
C++ / Go surfaces, the argument checks that come before any device work, blob_index, and the build-quality guard for the
kernels the feature adds to blob.hip (no scratch, no spills, no flat_* instructions) with every earlier kernel of
blob.hip still there exactly once."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pbsgpu_blob_decode_device"
NEW_KERNELS = ("k_dec_heads", "k_dec_pieces", "k_dec_fold", "k_dec_copy", "k_dec_status")
OLD_KERNELS = ("k_pagecrc_pieces", "k_pagecrc_fold", "k_page_copy", "k_crc_pieces", "k_crc_fold", "k_blob_heads",
               "k_upnew_count", "k_upnew_scan", "k_upnew_fill", "k_upnew_ppart")


@pytest.fixture(scope="module")
def L():
    from pbs_plus_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_name_is_declared_exported_and_bound(L):
    from pbs_plus_amd import _lib

    hdr = _read("include", "pbsgpu.h")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pbsgpu_[a-z0-9_]+)", out))
    assert re.search(r"^int %s\s*\(" % NAME, hdr, flags=re.M)
    assert NAME in exported
    assert NAME in _lib.SYMBOLS
    assert getattr(L, NAME).argtypes is not None
    assert len(_lib.SYMBOLS[NAME][1]) == 15
    assert re.search(r"^#define PBSGPU_HAS_BLOB_DECODE 1\b", hdr, flags=re.M)
    assert re.search(r"^#define PBSGPU_ABI_VERSION 5\b", hdr, flags=re.M)
    assert L.pbsgpu_abi_version() == 5
    assert re.search(r"^typedef struct pbsgpu_decode_stats \{", hdr, flags=re.M)
    assert C.sizeof(_lib.DecodeStats) == 8 * 10
    # the section names the reference call sites it stands behind, and says how often it synchronises
    sec = hdr[hdr.index("---- restore a stream from its index and data blobs"):hdr.index("int " + NAME)]
    assert "verification/job.go:931" in sec and "pxar/format.go:101" in sec and "pxar/client.go" in sec
    assert re.search(r"synchronises it ONCE", sec)


def test_python_cpp_and_go_surfaces():
    import inspect

    import pbs_plus_amd
    from pbs_plus_amd import Engine

    sig = inspect.signature(Engine.blob_decode).parameters
    assert list(sig) == ["self", "data", "blobs", "idx", "blob_of", "start", "end", "check_digest", "dst", "nbytes"]
    assert sig["blob_of"].default is None and sig["start"].default is None and sig["end"].default is None
    assert sig["check_digest"].default is True and sig["dst"].default is None and sig["nbytes"].default is None
    assert list(inspect.signature(pbs_plus_amd.blob_index).parameters) == ["blob_digests", "idx"]
    hpp = _read("include", "pbsgpu.hpp")
    go = _read("go", "pbsgpu", "pbsgpu.go")
    fb = _read("go", "pbsgpu", "fallback.go")
    assert NAME + "(" in hpp
    blob_ns = hpp[hpp.index("namespace blob {"):hpp.index("}  // namespace blob")]
    assert re.search(r"\bResult<Decoded> Decode\(", blob_ns)
    assert re.search(r"\bC\.%s\(" % NAME, go)
    for text in (go, fb):
        assert re.search(r"^func \(e \*Engine\) DecodeBlobs\(", text, flags=re.M)
        assert re.search(r"^type DecodeStats struct", text, flags=re.M)
    body = fb[fb.index("func (e *Engine) DecodeBlobs("):]
    assert "ErrNotBuilt" in body[:body.index("\n}")]


def test_argument_checks_that_need_no_device(L):
    """every PBSGPU_E_INVALID that is decided before the runtime is touched, on pointers that are never dereferenced"""
    from pbs_plus_amd import RECORD_DTYPE, _lib

    E = _lib.E_INVALID
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)
    buf, dst = 0x10000000, 0x20000000  # "device" addresses: the bad argument is found before they are looked at
    blobs = np.array([[0, 112], [112, 212], [400, 12]], dtype=np.uint64)
    idx = np.zeros(3, dtype=RECORD_DTYPE)
    idx["size"] = (100, 200, 0)
    idx["end"] = (1100, 1300, 1300)
    bo = np.array([0, 1, 2], dtype=np.uint32)
    status = np.zeros(4, dtype=np.uint8)
    st = _lib.DecodeStats()
    f = L.pbsgpu_blob_decode_device

    def call(eng=fake, bptr=buf, nbytes=1024, bl=blobs, nblob=3, ix=idx, nidx=3, of=bo, rs=1000, re_=1300, dptr=dst, cap=300,
             stat=status):
        return f(eng, bptr, nbytes, None if bl is None else bl.ctypes.data, nblob, None if ix is None else ix.ctypes.data, nidx,
                 None if of is None else of.ctypes.data, rs, re_, 1, dptr, cap, None if stat is None else stat.ctypes.data,
                 C.byref(st))

    assert call(eng=None) == E
    assert call(bptr=None) == E                      # bytes without a buffer
    assert call(bl=None) == E
    assert call(ix=None) == E
    assert call(stat=None) == E
    assert call(dptr=None) == E                      # a range without a destination
    assert call(nidx=1 << 32) == E
    assert call(of=None, nblob=2) == E               # the identity needs nblob == nidx
    assert call(nblob=0) == E
    assert call(nbytes=411) == E                     # the last blob ends at 412
    far = blobs.copy()
    far[1] = (1 << 63, 1 << 63)
    assert call(bl=far) == E                         # offset + length wraps
    assert call(of=np.array([0, 3, 2], dtype=np.uint32)) == E
    gap = idx.copy()
    gap["end"][1] = 1301
    assert call(ix=gap, re_=1300) == E               # entry 2 does not begin where entry 1 ends
    under = idx.copy()
    under["size"][0] = 1101
    assert call(ix=under) == E                       # an entry that begins before 0
    assert call(rs=999) == E
    assert call(re_=1301) == E
    assert call(rs=1200, re_=1100) == E
    assert call(bptr=dst - 1000, dptr=dst, nbytes=1024) == E   # dst begins inside the blob buffer
    assert call(bptr=dst + 299, dptr=dst, nbytes=1024) == E    # dst's last byte is the buffer's first
    assert st.out_bytes == 0 and sum(st.count) == 0
    assert not status.any()
    # nothing to do is no error, whatever else is passed
    assert call(nidx=0, ix=None, stat=None, bl=None, nblob=0, of=None, dptr=None, cap=0) == _lib.OK


def test_blob_index_by_digest():
    from pbs_plus_amd import RECORD_DTYPE, blob_index

    rng = np.random.default_rng(5)
    dg = rng.integers(0, 256, size=(6, 32), dtype=np.uint8)
    dg[4] = dg[1]                                    # two blobs carry one digest: the first is taken
    idx = np.zeros(9, dtype=RECORD_DTYPE)
    order = [3, 0, 0, 5, 1, 4, 2, 1, 3]
    idx["digest"] = dg[order]
    got = blob_index(dg, idx)
    assert got.dtype == np.uint32
    assert got.tolist() == [3, 0, 0, 5, 1, 1, 2, 1, 3]
    assert blob_index(dg, idx[:0]).size == 0
    idx["digest"][6][31] ^= 1
    with pytest.raises(KeyError):
        blob_index(dg, idx)
    with pytest.raises(KeyError):
        blob_index(dg[:0], idx[:1])


def _compile(tmp_path, name):
    """the method of tests/test_upload_new_surface.py: (resource usage per kernel, assembly text)"""
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


def test_decode_kernels_do_not_spill_and_use_no_flat_memory_instructions(tmp_path):
    usage, text = _compile(tmp_path, "blob")
    for k in NEW_KERNELS + OLD_KERNELS:
        names = [n for n in usage if k in n]
        assert len(names) == 1, (k, list(usage))
    for k in NEW_KERNELS:
        assert not [e for e in OLD_KERNELS if e in k], k
        name = [n for n in usage if k in n][0]
        r = usage[name]
        assert r.get("scratch", -1) == 0 and r.get("sgpr_spill", -1) == 0 and r.get("vgpr_spill", -1) == 0, (k, r)
        body = _body(text, name)
        assert not [ln for ln in body if re.match(r"\s+flat_", ln)], k
        assert not [ln for ln in body if re.match(r"\s+scratch_", ln)], k
        assert [ln for ln in body if re.match(r"\s+global_", ln)], k
