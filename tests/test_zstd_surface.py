"""The zstd decoder's surfaces without a GPU: the C ABI additions (pbsgpu_zstd_frame_info, pbsgpu_zstd_decode_device), the
Python / C++ / Go bindings, the argument checks that come before any device work, frame_info on every golden frame, and
the build-quality guard for the kernel of zstd.hip (no spills, no scratch, no flat_* instructions) with every kernel of
blob.hip still there exactly once."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_inputs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pbsgpu_zstd_frame_info", "pbsgpu_zstd_decode_device", "pbsgpu_blob_decode2_device")
NEW_KERNELS = ("k_zstd_frames", "k_zr_select", "k_zr_ranges", "k_zr_copy", "k_zr_status")
BLOB_KERNELS = ("k_pagecrc_pieces", "k_pagecrc_fold", "k_page_copy", "k_crc_pieces", "k_crc_fold", "k_blob_heads",
                "k_upnew_count", "k_upnew_scan", "k_upnew_fill", "k_upnew_ppart", "k_dec_heads", "k_dec_pieces", "k_dec_fold",
                "k_dec_copy", "k_dec_status")


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
    for name in NAMES:
        assert re.search(r"^int %s\s*\(" % name, hdr, flags=re.M), name
        assert name in exported and name in _lib.SYMBOLS, name
        assert getattr(L, name).argtypes is not None
    assert len(_lib.SYMBOLS["pbsgpu_blob_decode2_device"][1]) == 15
    assert re.search(r"^typedef struct pbsgpu_decode_stats2 \{", hdr, flags=re.M) and C.sizeof(_lib.DecodeStats2) == 8 * 14
    assert C.sizeof(_lib.DecodeStats) == 80
    for name, val in (("PBSGPU_DECODE_F_DIGEST", "1u"), ("PBSGPU_DECODE_F_ZSTD", "2u"), ("PBSGPU_BLOB_BAD_DATA", "6")):
        assert re.search(r"^#define %s %s\b" % (name, val), hdr, flags=re.M), name
    d2 = hdr[hdr.index("Restore with the compressed blobs decoded"):hdr.index("int pbsgpu_blob_decode2_device")]
    assert "magic, header, CRC, frame, size, digest" in d2 and "ONE synchronisation" in d2 and "backup/command.go" in d2
    assert len(_lib.SYMBOLS["pbsgpu_zstd_frame_info"][1]) == 6 and len(_lib.SYMBOLS["pbsgpu_zstd_decode_device"][1]) == 10
    assert re.search(r"^#define PBSGPU_HAS_ZSTD_DECODE 1\b", hdr, flags=re.M)
    assert re.search(r"^#define PBSGPU_ABI_VERSION 5\b", hdr, flags=re.M) and L.pbsgpu_abi_version() == 5
    assert re.search(r"^#define PBSGPU_BLOB_NSTATUS 6\b", hdr, flags=re.M)
    for k, name in enumerate(("OK", "BAD_FRAME", "BAD_SIZE", "UNSUPPORTED")):
        assert re.search(r"^#define PBSGPU_ZSTD_%s %d\b" % (name, k), hdr, flags=re.M), name
    assert (_lib.ZSTD_OK, _lib.ZSTD_BAD_FRAME, _lib.ZSTD_BAD_SIZE, _lib.ZSTD_UNSUPPORTED) == (0, 1, 2, 3)
    # the section names the reference call sites it stands behind, the decisions, and how often it synchronises
    sec = hdr[hdr.index("---- zstd frames on the device"):hdr.index("int pbsgpu_zstd_decode_device")]
    assert "backup/command.go" in sec and "verification/job.go:931" in sec and "pxar/format.go:101" in sec
    assert "NOT verified" in sec and "UNSUPPORTED" in sec and re.search(r"ONE synchronisation", sec)


def test_python_cpp_and_go_surfaces():
    import pbs_plus_amd
    from pbs_plus_amd import Engine

    sig = inspect.signature(Engine.zstd_decode).parameters
    assert list(sig)[:5] == ["self", "data", "frames", "out", "dst"]
    assert sig["out"].default is None and sig["dst"].default is None
    sig2 = inspect.signature(Engine.blob_decode2).parameters
    assert list(sig2)[:len(inspect.signature(Engine.blob_decode).parameters)] == list(inspect.signature(Engine.blob_decode).parameters)
    assert sig2["zstd"].default is True
    assert list(inspect.signature(pbs_plus_amd.zstd_frame_info).parameters) == ["frame"]
    assert "zstd_frame_info" in pbs_plus_amd.__all__
    hpp, go, fb = _read("include", "pbsgpu.hpp"), _read("go", "pbsgpu", "pbsgpu.go"), _read("go", "pbsgpu", "fallback.go")
    blob_ns = hpp[hpp.index("namespace blob {"):hpp.index("}  // namespace blob")]
    assert re.search(r"\bResult<ZstdDecoded> DecodeZstd\(", blob_ns) and "pbsgpu_zstd_decode_device(" in blob_ns
    for name in NAMES:
        assert re.search(r"\bC\.%s\(" % name, go), name
    assert re.search(r"\bResult<Decoded2> Decode2\(", blob_ns)
    for text in (go, fb):
        assert re.search(r"^func \(e \*Engine\) DecodeBlobs2\(", text, flags=re.M) and re.search(r"^type DecodeStats2 struct", text, flags=re.M)
        assert re.search(r"^func \(e \*Engine\) DecodeZstd\(", text, flags=re.M)
        assert re.search(r"^func ZstdFrameInfo\(", text, flags=re.M)
        assert re.search(r"^type ZstdFrame struct", text, flags=re.M)
    for fn in ("func (e *Engine) DecodeZstd(", "func ZstdFrameInfo(", "func (e *Engine) DecodeBlobs2("):
        body = fb[fb.index(fn):]
        assert "ErrNotBuilt" in body[:body.index("}\n")], fn


def test_argument_checks_that_need_no_device(L):
    """every PBSGPU_E_INVALID that is decided before the runtime is touched, on pointers that are never dereferenced"""
    from pbs_plus_amd import _lib

    E = _lib.E_INVALID
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)
    src, dst = 0x10000000, 0x20000000  # "device" addresses: the bad argument is found before they are looked at
    frames = np.array([[0, 100], [100, 50]], dtype=np.uint64)
    out = np.array([[0, 300], [300, 200]], dtype=np.uint64)
    status = np.full(2, 9, dtype=np.uint8)
    decoded = np.full(2, 9, dtype=np.uint64)
    f = L.pbsgpu_zstd_decode_device

    def call(eng=fake, sp=src, nbytes=1024, fr=frames, n=2, o=out, dp=dst, cap=500, stat=status, dec=decoded):
        return f(eng, sp, nbytes, None if fr is None else fr.ctypes.data, n, None if o is None else o.ctypes.data, dp, cap,
                 None if stat is None else stat.ctypes.data, None if dec is None else dec.ctypes.data)

    assert call(eng=None) == E
    assert call(sp=None) == E
    assert call(fr=None) == E
    assert call(o=None) == E
    assert call(stat=None) == E
    assert call(dp=None) == E
    assert call(nbytes=149) == E                                             # the second frame ends at 150
    assert call(fr=np.array([[1 << 63, 1 << 63], [0, 1]], dtype=np.uint64)) == E  # offset + length wraps
    assert call(cap=499) == E                                                # the second room ends at 500
    assert call(o=np.array([[0, 300], [299, 200]], dtype=np.uint64)) == E    # the rooms share byte 299
    assert call(o=np.array([[300, 200], [0, 301]], dtype=np.uint64)) == E    # in either order
    assert call(o=np.array([[0, 1 << 32], [0, 0]], dtype=np.uint64), cap=1 << 40) == E  # a room of 4 GiB
    assert call(sp=dst - 1000, dp=dst) == E                                  # dst begins inside the source
    assert call(sp=dst + 499, dp=dst) == E                                   # dst's last byte is the source's first
    assert np.all(status == 9) and np.all(decoded == 9)
    assert call(n=0, fr=None, o=None, stat=None, dec=None, dp=None, cap=0, sp=None, nbytes=0) == _lib.OK
    assert L.pbsgpu_zstd_frame_info(None, 5, None, None, None, None) == E


def test_decode2_argument_checks_that_need_no_device(L):
    """pbsgpu_blob_decode2_device refuses what pbsgpu_blob_decode_device refuses, before the runtime is touched, plus
    unknown flags and, with F_ZSTD, a blob of 4 GiB or more"""
    from pbs_plus_amd import RECORD_DTYPE, _lib

    E = _lib.E_INVALID
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)
    buf, dst = 0x10000000, 0x20000000
    blobs = np.array([[0, 112], [112, 212]], dtype=np.uint64)
    idx = np.zeros(2, dtype=RECORD_DTYPE)
    idx["size"] = (100, 200)
    idx["end"] = (1100, 1300)
    status = np.zeros(2, dtype=np.uint8)
    st = _lib.DecodeStats2()
    f = L.pbsgpu_blob_decode2_device

    def call(eng=fake, nbytes=1024, bl=blobs, ix=idx, nidx=2, rs=1000, re_=1300, flags=3, dptr=dst, cap=300, bptr=buf):
        return f(eng, bptr, nbytes, bl.ctypes.data, 2, ix.ctypes.data, nidx, None, rs, re_, flags, dptr, cap, status.ctypes.data, C.byref(st))

    assert call(eng=None) == E
    assert call(flags=4) == E and call(flags=7) == E
    assert call(nbytes=323) == E
    assert call(rs=999) == E and call(re_=1301) == E and call(dptr=None) == E
    assert call(bptr=dst - 1000) == E
    big = np.array([[0, 112], [112, 1 << 32]], dtype=np.uint64)
    assert call(bl=big, nbytes=1 << 33, flags=2) == E
    assert call(nidx=0) == _lib.OK
    assert sum(st.count) == 0 and st.zstd_in_bytes == 0 and not status.any()


def test_frame_info_on_every_fixture(L):
    from pbs_plus_amd import zstd_frame_info

    cases = zstd_inputs.golden().load()
    assert len(cases) >= 30
    seen = set()
    for c in cases:
        st, size, window, hb, ck = c["info"]
        got = zstd_frame_info(c["frame"])
        assert got["status"] == st, c["name"]
        if st == 0:
            assert got["content_size"] == (None if size < 0 else size), c["name"]
            assert (got["window_size"], got["header_bytes"], got["has_checksum"]) == (max(window, 0) if size >= 0 or window else 0, hb, bool(ck)), c["name"]
            seen.add((size < 0, bool(ck), hb))
            if c["status"] == 0 and size >= 0:
                assert size == c["length"], c["name"]
    assert {True, False} == {s[0] for s in seen} == {s[1] for s in seen} and len({s[2] for s in seen}) >= 4
    # every out pointer may be NULL, and a header cut anywhere is BAD_FRAME, never a read past the end
    frame = np.frombuffer(next(c for c in cases if c["name"] == "hand-fcs8")["frame"], np.uint8)
    for cut in range(13):
        assert L.pbsgpu_zstd_frame_info(frame[:cut].copy().ctypes.data if cut else None, cut, None, None, None, None) == 1
    assert L.pbsgpu_zstd_frame_info(frame.ctypes.data, 13, None, None, None, None) == 0


def _compile(tmp_path, name):
    """the method of tests/test_blob_decode_surface.py: (resource usage per kernel, assembly text)"""
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
                         ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            mm = re.search(pat, line)
            if mm:
                cur[key] = int(mm.group(1))
    return usage, open(asm).read()


def _body(text, name):
    m = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape(name), text, flags=re.S | re.M)
    assert m, name
    return m.group(1).splitlines()


def test_the_decode_kernel_does_not_spill_and_uses_no_flat_memory_instructions(tmp_path):
    usage, text = _compile(tmp_path, "zstd")
    for k in NEW_KERNELS:
        names = [n for n in usage if k in n]
        assert len(names) == 1, (k, list(usage))
        r = usage[names[0]]
        assert r.get("scratch", -1) == 0 and r.get("sgpr_spill", -1) == 0 and r.get("vgpr_spill", -1) == 0, (k, r)
        assert r.get("lds", 0) <= 20 << 10 and (k != "k_zstd_frames" or r.get("lds", 0) > 0), r  # the tables are in LDS (16 244 bytes today); at 20 KiB eight workgroups still fit a CU
        body = _body(text, names[0])
        assert not [ln for ln in body if re.match(r"\s+flat_", ln)], k
        assert not [ln for ln in body if re.match(r"\s+scratch_", ln)], k
        assert [ln for ln in body if re.match(r"\s+global_", ln)], k
        assert k != "k_zstd_frames" or [ln for ln in body if re.match(r"\s+ds_", ln)], k


def test_every_kernel_of_blob_hip_is_still_there_once(tmp_path):
    usage, _ = _compile(tmp_path, "blob")
    for k in BLOB_KERNELS:
        assert len([n for n in usage if k in n]) == 1, (k, list(usage))
    assert not [n for n in usage if "zstd" in n]
    mk = _read("pbs_plus_amd", "csrc", "Makefile")
    assert re.search(r"^\$\(OBJ\)/zstd\.o: zstd\.hip zstd_decode\.h", mk, flags=re.M) and "$(OBJ)/zstd.o" in mk.split("OBJS :=")[1].split("\n")[0]
