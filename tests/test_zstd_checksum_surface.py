"""The surfaces of the zstd content checksum and of whole streams without a GPU: the C ABI additions
(pbsgpu_xxh64_many_device, pbsgpu_zstd_decode2_device, pbsgpu_zstd_stream_info, pbsgpu_zstd_encode_bound2,
pbsgpu_zstd_encode2_device), their bindings, the refusals that come before any device work, bound2 and stream_info against
Python arithmetic, and the build-quality guard for the kernels of zstd_checksum.hip (no spills, no scratch, no flat_*
instructions) with the older translation units still reporting the kernels they reported."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_checksum_inputs as zi  # noqa: E402
import zstd_inputs  # noqa: E402
from test_zstd_surface import _body, _compile  # noqa: E402  (resource usage per kernel and assembly text of a translation unit)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pbsgpu_xxh64_many_device", "pbsgpu_zstd_decode2_device", "pbsgpu_zstd_stream_info", "pbsgpu_zstd_encode2_device")
NARGS = {"pbsgpu_xxh64_many_device": 7, "pbsgpu_zstd_decode2_device": 11, "pbsgpu_zstd_stream_info": 6,
         "pbsgpu_zstd_encode_bound2": 2, "pbsgpu_zstd_encode2_device": 11}
OLDER = {"zstd": ("k_zstd_frames", "k_zr_select", "k_zr_ranges", "k_zr_copy", "k_zr_status"),
         "zstd_encode": ("k_zenc_blocks", "k_zenc_assemble"), "zstd_encode_tables": ("k_zenc_tblocks",),
         "zstd_encode_window": ("k_zenc_wblocks", "k_zenc_wtblocks")}


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
    assert re.search(r"^uint64_t pbsgpu_zstd_encode_bound2\s*\(", hdr, flags=re.M)
    for name, n in NARGS.items():
        assert name in exported and name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == n, name
        assert getattr(L, name).argtypes is not None
    for name, val in (("PBSGPU_HAS_ZSTD_CHECKSUM", "1"), ("PBSGPU_ZSTD_BAD_CHECKSUM", "4"), ("PBSGPU_ZSTD_F_CHECKSUM", "1u"),
                      ("PBSGPU_ZSTD_F_STREAM", "2u")):
        assert re.search(r"^#define %s %s\b" % (name, val), hdr, flags=re.M), name
    assert (_lib.ZSTD_BAD_CHECKSUM, _lib.ZSTD_F_CHECKSUM, _lib.ZSTD_F_STREAM) == (4, 1, 2)
    # no new engine option and no ABI bump: the options struct and the version are what they were
    assert re.search(r"^#define PBSGPU_ABI_VERSION 5\b", hdr, flags=re.M) and L.pbsgpu_abi_version() == 5
    assert C.sizeof(_lib.EngineOptions) == 96
    # the section names the reference call sites of the old calls, the decisions, and how often it synchronises
    sec = hdr[hdr.index("---- zstd content checksums and whole streams"):hdr.index("int pbsgpu_zstd_stream_info")]
    assert "verification/job.go:931" in sec and "pxar/format.go:101" in sec and "commit_orchestrate.go:356" in sec
    assert "pbsgpu_blob_decode2_device are unchanged" in sec and "ONE synchronisation" in sec and "ZSTD_decompress" in sec
    assert "ITS OWN frame" in sec and "libzstd's order" in sec
    enc = hdr[hdr.index("pbsgpu_zstd_encode_device with flags"):hdr.index("int pbsgpu_zstd_encode2_device")]
    assert "converter.go:399" in enc and "bit 2" in enc and "XXH64(content, 0)" in enc and "write no\n * checksum" in enc


def test_python_cpp_and_go_surfaces():
    import pbs_plus_amd
    from pbs_plus_amd import Engine

    sig = inspect.signature(Engine.zstd_decode2).parameters
    assert list(sig)[:5] == ["self", "data", "frames", "out", "dst"]
    assert sig["checksum"].default is False and sig["stream"].default is False
    sig = inspect.signature(Engine.zstd_encode2).parameters
    assert list(sig)[:5] == ["self", "data", "chunks", "out", "dst"] and sig["checksum"].default is False
    sig = inspect.signature(Engine.xxh64_many).parameters
    assert list(sig)[:3] == ["self", "data", "segments"] and sig["seed"].default == 0
    assert "zstd_stream_info" in pbs_plus_amd.__all__ and "zstd_encode_bound2" in pbs_plus_amd.__all__
    hpp, go, fb = _read("include", "pbsgpu.hpp"), _read("go", "pbsgpu", "pbsgpu.go"), _read("go", "pbsgpu", "fallback.go")
    blob_ns = hpp[hpp.index("namespace blob {"):hpp.index("}  // namespace blob")]
    assert re.search(r"\bResult<ZstdDecoded> DecodeZstd2\(", blob_ns) and "pbsgpu_zstd_decode2_device(" in blob_ns
    assert re.search(r"\bResult<ZstdEncoded> EncodeZstd2\(", blob_ns) and "pbsgpu_zstd_encode2_device(" in blob_ns
    assert "pbsgpu_xxh64_many_device(" in blob_ns and "pbsgpu_zstd_stream_info(" in blob_ns
    for name in NARGS:
        assert re.search(r"\bC\.%s\(" % name, go), name
    for text in (go, fb):
        for pat in (r"^func \(e \*Engine\) DecodeZstd2\(", r"^func \(e \*Engine\) EncodeZstd2\(", r"^func \(e \*Engine\) XXH64Device\(",
                    r"^func ZstdStreamInfo\(", r"^func ZstdEncodeBound2\(", r"^type ZstdStream struct", r"^const ZstdBadChecksum = 4$"):
            assert re.search(pat, text, flags=re.M), pat
    for fn in ("func (e *Engine) DecodeZstd2(", "func (e *Engine) EncodeZstd2(", "func (e *Engine) XXH64Device(", "func ZstdStreamInfo("):
        body = fb[fb.index(fn):]
        assert "ErrNotBuilt" in body[:body.index("}\n")], fn


def test_the_cpp_mirror_compiles():
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), "-x", "c++",
                          os.path.join(ROOT, "include", "pbsgpu.hpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]


def test_refusals_that_need_no_device(L):
    """every PBSGPU_E_INVALID of the new calls that is decided before the runtime is touched, on pointers that are never
    dereferenced: the old calls' refusals, and an unknown flag bit"""
    from pbs_plus_amd import _lib

    E = _lib.E_INVALID
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)
    src, dst = 0x10000000, 0x20000000
    segs = np.array([[0, 100], [100, 50]], dtype=np.uint64)
    out = np.array([[0, 300], [300, 200]], dtype=np.uint64)
    status = np.full(2, 9, dtype=np.uint8)
    lens = np.full(2, 9, dtype=np.uint64)

    for f, allowed in ((L.pbsgpu_zstd_decode2_device, 3), (L.pbsgpu_zstd_encode2_device, 1)):
        def call(eng=fake, sp=src, nbytes=1024, sg=segs, n=2, o=out, dp=dst, cap=500, stat=status, ln=lens, flags=allowed):
            return f(eng, sp, nbytes, None if sg is None else sg.ctypes.data, n, None if o is None else o.ctypes.data, dp, cap,
                     None if stat is None else stat.ctypes.data, None if ln is None else ln.ctypes.data, flags)

        for flags in (4, 8, 1 << 31, 0xFFFFFFFF) + ((2, 3) if allowed == 1 else ()):
            assert call(flags=flags) == E, (f, flags)
        for flags in range(allowed + 1):
            if flags & ~allowed:
                continue
            assert call(eng=None, flags=flags) == E
            assert call(sp=None, flags=flags) == E and call(sg=None, flags=flags) == E and call(o=None, flags=flags) == E
            assert call(stat=None, flags=flags) == E and call(dp=None, flags=flags) == E
            assert call(nbytes=149, flags=flags) == E and call(cap=499, flags=flags) == E
            assert call(o=np.array([[0, 300], [299, 200]], dtype=np.uint64), flags=flags) == E    # the rooms share byte 299
            big = np.array([[0, 1 << 32], [0, 1]], dtype=np.uint64)  # a frame, a chunk of 4 GiB
            assert call(sg=big, nbytes=1 << 40, flags=flags) == E
            assert call(sp=dst - 1000, dp=dst, flags=flags) == E                                   # dst begins inside the source
            assert call(n=0, sg=None, o=None, stat=None, ln=None, dp=None, cap=0, sp=None, nbytes=0, flags=flags) == _lib.OK
    assert np.all(status == 9) and np.all(lens == 9)
    x = L.pbsgpu_xxh64_many_device
    hashes = np.full(2, 9, dtype=np.uint64)
    assert x(None, src, 1024, segs.ctypes.data, 2, 0, hashes.ctypes.data) == E
    assert x(fake, None, 1024, segs.ctypes.data, 2, 0, hashes.ctypes.data) == E
    assert x(fake, src, 1024, None, 2, 0, hashes.ctypes.data) == E and x(fake, src, 1024, segs.ctypes.data, 2, 0, None) == E
    assert x(fake, src, 149, segs.ctypes.data, 2, 0, hashes.ctypes.data) == E
    assert x(fake, src, 1024, None, 0, 0, None) == _lib.OK
    assert np.all(hashes == 9)
    assert L.pbsgpu_zstd_stream_info(None, 5, None, None, None, None) == E


def test_bound2_against_python_arithmetic():
    from pbs_plus_amd import zstd_encode_bound, zstd_encode_bound2

    for n in (0, 1, 255, 256, 65_791, 65_792, 131_072, 131_073, 300_000, (1 << 32) - 1, 1 << 40):
        want = 5 + (1 if n <= 255 else 2 if n <= 65_791 else 4) + 3 * max(1, -(-n // (128 << 10))) + n
        assert zstd_encode_bound(n) == want == zstd_encode_bound2(n) == zstd_encode_bound2(n, False)
        assert zstd_encode_bound2(n, True) == want + 4


def test_stream_info_against_python_arithmetic(L):
    from pbs_plus_amd import zstd_frame_info, zstd_stream_info

    for s in zi.streams():
        got = zstd_stream_info(s["stream"])
        if s["status"] == zi.OK:
            assert got["status"] == zi.OK and got["content_size"] == len(s["content"]), s["name"]
        elif s["status"] == zi.BAD_CHECKSUM:  # the headers are in order: the walk reaches the end
            assert got["status"] == zi.OK and got["frames"] == 2 and got["any_checksum"], s["name"]
        else:
            assert got["status"] == s["status"], (s["name"], got)
    info = {s["name"]: zstd_stream_info(s["stream"]) for s in zi.streams()}
    assert (info["three"]["frames"], info["three"]["skippable"], info["three"]["any_checksum"]) == (3, 0, True)
    assert (info["skip-everywhere"]["frames"], info["skip-everywhere"]["skippable"]) == (2, 4)
    assert (info["skip-alone"]["frames"], info["skip-alone"]["skippable"], info["skip-alone"]["content_size"]) == (0, 1, 0)
    assert info["empty"] == dict(status=0, content_size=0, frames=0, skippable=0, any_checksum=False)
    assert (info["middle-bad"]["frames"], info["middle-dictionary"]["frames"]) == (1, 1)  # the counts hold up to the failure
    # a frame that declares no size makes the sum unknown; a single frame agrees with frame_info
    cases = {c["name"]: c for c in zstd_inputs.golden().load()}
    nosize, sized = cases["text-50000-nosize"]["frame"], cases["lowsym-3000"]["frame"]
    got = zstd_stream_info(sized + nosize + sized)
    assert got["status"] == 0 and got["content_size"] is None and got["frames"] == 3 and got["any_checksum"] is False
    for c in cases.values():
        one, st = zstd_frame_info(c["frame"]), zstd_stream_info(c["frame"])
        if c["status"] == 0:
            assert st["status"] == 0 and st["frames"] == 1 and st["content_size"] == one["content_size"], c["name"]
            assert st["any_checksum"] == one["has_checksum"]
    # cut anywhere inside its headers it is BAD_FRAME, never a read past the end (the copy is exact)
    two = next(s for s in zi.streams() if s["name"] == "skip-everywhere")["stream"]
    for cut in list(range(1, 40)) + [len(two) - 1]:
        a = np.frombuffer(two[:cut], np.uint8).copy()
        st = L.pbsgpu_zstd_stream_info(a.ctypes.data, cut, None, None, None, None)
        assert st == (zi.OK if cut == 9 else zi.BAD_FRAME), cut  # (9 bytes: the first skippable frame, whole)


def test_the_new_kernels_do_not_spill_and_use_no_flat_memory_instructions(tmp_path):
    usage, text = _compile(tmp_path, "zstd_checksum")
    assert len(usage) == 2, list(usage)
    for k in ("k_xxh64_ranges", "k_zstd_frames2"):
        names = [n for n in usage if k in n]
        assert len(names) == 1, (k, list(usage))
        r = usage[names[0]]
        assert r.get("scratch", -1) == 0 and r.get("sgpr_spill", -1) == 0 and r.get("vgpr_spill", -1) == 0, (k, r)
        assert 0 < r.get("lds", 0) <= 20 << 10, (k, r)  # k_zstd_frames2: State, the walk and the plan; eight workgroups fit a CU
        body = _body(text, names[0])
        assert not [ln for ln in body if re.match(r"\s+flat_", ln)], k
        assert not [ln for ln in body if re.match(r"\s+scratch_", ln)], k
        assert [ln for ln in body if re.match(r"\s+global_load", ln)], k
        assert [ln for ln in body if re.match(r"\s+ds_", ln)], k
    mk = _read("pbs_plus_amd", "csrc", "Makefile")
    assert "$(OBJ)/zstd_checksum.o" in mk.split("OBJS :=")[1].split("\n")[0] and "zstd_checksum.hip" in mk.split("SRCS :=")[1].split("\n")[0]


@pytest.mark.parametrize("unit", sorted(OLDER))
def test_the_older_translation_units_report_the_kernels_they_reported(tmp_path, unit):
    usage, _ = _compile(tmp_path, unit)  # (their own guards: tests/test_zstd_*surface.py)
    assert len(usage) == len(OLDER[unit]), (unit, list(usage))
    for k in OLDER[unit]:
        assert len([n for n in usage if re.search(r"\d%s[A-Z]" % k, n)]) == 1, (k, list(usage))
