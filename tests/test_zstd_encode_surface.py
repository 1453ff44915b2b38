"""The zstd encoder's surfaces without a GPU: the C ABI additions (pbsgpu_zstd_encode_bound, pbsgpu_zstd_encode_device,
pbsgpu_blob_encode2_device), the Python / C++ / Go bindings, the argument checks that come before any device work, the
bound against its formula, and the build-quality guard for the two kernels of zstd_encode.hip from the compiler's own
resource report (no scratch, no spills)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pbsgpu_zstd_encode_device", "pbsgpu_blob_encode2_device")
KERNELS = ("k_zenc_blocks", "k_zenc_assemble")


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
    assert re.search(r"^uint64_t pbsgpu_zstd_encode_bound\(uint64_t n\);", hdr, flags=re.M)
    assert "pbsgpu_zstd_encode_bound" in exported and _lib.SYMBOLS["pbsgpu_zstd_encode_bound"][0] is C.c_uint64
    assert len(_lib.SYMBOLS["pbsgpu_zstd_encode_device"][1]) == 10 and len(_lib.SYMBOLS["pbsgpu_blob_encode2_device"][1]) == 13
    assert re.search(r"^#define PBSGPU_HAS_ZSTD_ENCODE 1\b", hdr, flags=re.M)
    assert re.search(r"^#define PBSGPU_ENCODE_F_ZSTD 1u\b", hdr, flags=re.M) and _lib.ENCODE_F_ZSTD == 1
    assert re.search(r"^#define PBSGPU_ABI_VERSION 5\b", hdr, flags=re.M) and L.pbsgpu_abi_version() == 5
    assert re.search(r"^typedef struct pbsgpu_encode_stats \{", hdr, flags=re.M) and C.sizeof(_lib.EncodeStats) == 8 * 8
    # the section names the reference call sites it stands behind, the verdict rule and how often it synchronises
    sec = hdr[hdr.index("---- zstd frames written on the device"):hdr.index("int pbsgpu_blob_encode2_device")]
    assert "tapeio/converter.go:399" in sec and "converter.go:410-435" in sec and "cmd/bkf2pxar/main.go:33" in sec
    assert "strictly shorter" in sec and "data_blob.rs" in sec and "EXTERNAL" in sec and sec.count("ONE synchronisation") == 2


def test_the_bound_is_the_formula(L):
    from pbs_plus_amd import zstd_encode_bound

    def formula(n):
        return 5 + (1 if n <= 255 else 2 if n <= 65_791 else 4) + 3 * max(1, -(-n // (128 << 10))) + n

    for n in (0, 1, 255, 256, 65_791, 65_792, 131_071, 131_072, 131_073, 300_000, 4 << 20, (16 << 20) + 1, (1 << 32) - 1):
        assert zstd_encode_bound(n) == formula(n) == L.pbsgpu_zstd_encode_bound(n), n


def test_python_cpp_and_go_surfaces():
    import pbs_plus_amd
    from pbs_plus_amd import Engine

    sig = inspect.signature(Engine.zstd_encode).parameters
    assert list(sig)[:5] == ["self", "data", "chunks", "out", "dst"]
    assert sig["out"].default is None and sig["dst"].default is None
    sig2 = inspect.signature(Engine.blob_encode2).parameters
    assert list(sig2)[:3] == ["self", "src", "chunks"] and sig2["zstd"].default is True
    assert "zstd_encode_bound" in pbs_plus_amd.__all__
    hpp, go, fb = _read("include", "pbsgpu.hpp"), _read("go", "pbsgpu", "pbsgpu.go"), _read("go", "pbsgpu", "fallback.go")
    blob_ns = hpp[hpp.index("namespace blob {"):hpp.index("}  // namespace blob")]
    assert re.search(r"\bResult<ZstdEncoded> EncodeZstd\(", blob_ns) and "pbsgpu_zstd_encode_device(" in blob_ns
    assert re.search(r"\bResult<Encoded2> Encode2\(", blob_ns) and "pbsgpu_blob_encode2_device(" in blob_ns
    for name in NAMES + ("pbsgpu_zstd_encode_bound",):
        assert re.search(r"\bC\.%s\(" % name, go), name
    for text in (go, fb):
        assert re.search(r"^func \(e \*Engine\) EncodeZstd\(", text, flags=re.M)
        assert re.search(r"^func \(e \*Engine\) EncodeBlobs2\(", text, flags=re.M)
        assert re.search(r"^type EncodeStats struct", text, flags=re.M) and re.search(r"^type Encoded2 struct", text, flags=re.M)
        assert re.search(r"^func ZstdEncodeBound\(", text, flags=re.M)
    for fn in ("func (e *Engine) EncodeZstd(", "func (e *Engine) EncodeBlobs2("):
        body = fb[fb.index(fn):]
        assert "ErrNotBuilt" in body[:body.index("}\n")], fn


def test_the_cpp_surface_compiles(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "pbsgpu.hpp"\n'
                   "int main() {\n"
                   "    std::vector<pbsgpu_segment> c{{0, 10}}, o{{0, 32}};\n"
                   "    auto a = pbsgpu::datastore::blob::EncodeZstd(nullptr, nullptr, 0, c, o, nullptr, 0);\n"
                   "    auto b = pbsgpu::datastore::blob::Encode2(nullptr, nullptr, 0, c, true, nullptr, 0);\n"
                   "    return a.value.status.size() == 1 && b.value.lens.size() == 1 ? 0 : 1;\n"
                   "}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_encode_argument_checks_that_need_no_device(L):
    """every PBSGPU_E_INVALID that is decided before the runtime is touched, on pointers that are never dereferenced"""
    from pbs_plus_amd import _lib

    E = _lib.E_INVALID
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)
    src, dst = 0x10000000, 0x20000000
    chunks = np.array([[0, 100], [100, 50]], dtype=np.uint64)
    out = np.array([[0, 300], [300, 200]], dtype=np.uint64)
    status = np.full(2, 9, dtype=np.uint8)
    flen = np.full(2, 9, dtype=np.uint64)
    f = L.pbsgpu_zstd_encode_device

    def call(eng=fake, sp=src, nbytes=1024, ch=chunks, n=2, o=out, dp=dst, cap=500, stat=status, fl=flen):
        return f(eng, sp, nbytes, None if ch is None else ch.ctypes.data, n, None if o is None else o.ctypes.data, dp, cap,
                 None if stat is None else stat.ctypes.data, None if fl is None else fl.ctypes.data)

    assert call(eng=None) == E
    assert call(sp=None) == E
    assert call(ch=None) == E
    assert call(o=None) == E
    assert call(stat=None) == E
    assert call(dp=None) == E
    assert call(nbytes=149) == E                                             # the second chunk ends at 150
    assert call(ch=np.array([[1 << 63, 1 << 63], [0, 1]], dtype=np.uint64)) == E  # offset + length wraps
    assert call(ch=np.array([[0, 1 << 32], [0, 1]], dtype=np.uint64), nbytes=1 << 40) == E  # a chunk of 4 GiB
    assert call(cap=499) == E                                                # the second room ends at 500
    assert call(o=np.array([[0, 300], [299, 200]], dtype=np.uint64)) == E    # the rooms share byte 299
    assert call(o=np.array([[300, 200], [0, 301]], dtype=np.uint64)) == E    # in either order
    assert call(sp=dst - 1000, dp=dst) == E                                  # dst begins inside the source
    assert call(sp=dst + 499, dp=dst) == E                                   # dst's last byte is the source's first
    assert np.all(status == 9) and np.all(flen == 9)
    assert call(n=0, ch=None, o=None, stat=None, fl=None, dp=None, cap=0, sp=None, nbytes=0) == _lib.OK


def test_encode2_argument_checks_that_need_no_device(L):
    from pbs_plus_amd import _lib

    E = _lib.E_INVALID
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)
    src, dst = 0x10000000, 0x20000000
    segs = np.array([[0, 100], [100, 50]], dtype=np.uint64)
    offs = np.zeros(3, dtype=np.uint64)
    f = L.pbsgpu_blob_encode2_device

    def call(eng=fake, sp=src, nbytes=1024, sg=segs, n=2, flags=1, dp=dst, cap=174):
        return f(eng, sp, nbytes, None if sg is None else sg.ctypes.data, n, flags, dp, cap, offs.ctypes.data, None, None, None, None)

    assert call(eng=None) == E
    assert call(flags=2) == E and call(flags=3) == E
    assert call(sp=None) == E
    assert call(sg=None) == E
    assert call(nbytes=149) == E
    assert call(cap=173) == _lib.E_CAPACITY and list(offs) == [0, 112, 174]  # the slots of the uncompressed layout
    assert call(cap=173, flags=0) == _lib.E_CAPACITY
    assert call(sg=np.array([[0, 1 << 32], [0, 1]], dtype=np.uint64), nbytes=1 << 40, cap=1 << 41) == E  # 4 GiB with F_ZSTD


def test_the_kernels_use_no_scratch_and_spill_nothing():
    """from the compiler's own report for zstd_encode.hip (make usage-zstd-encode): the figures DESIGN.md §16 quotes"""
    csrc = os.path.join(ROOT, "pbs_plus_amd", "csrc")
    r = subprocess.run(["make", "-s", "-C", csrc, "usage-zstd-encode"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    report = r.stderr + r.stdout
    blocks = re.split(r"remark: Function Name: ", report)[1:]
    seen = {}
    for b in blocks:
        name = b.split()[0]
        for k in KERNELS:
            if k in name:
                seen[k] = {m.group(1): int(m.group(2)) for m in re.finditer(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", b)}
    assert sorted(seen) == sorted(KERNELS), sorted(seen)
    for k, v in seen.items():
        print(k, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["SGPRs Spill"] == 0 and v["VGPRs Spill"] == 0, (k, v)
    assert seen["k_zenc_blocks"]["LDS Size [bytes/block]"] * 7 <= 160 << 10  # seven workgroups per CU, as DESIGN.md says
