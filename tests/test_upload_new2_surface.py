"""The fused upload calls with the blob's kind decided on the device (pbsgpu_ring_upload_new2_device /
pbsgpu_known_upload_new2_device) without a GPU: the C ABI and the Python / C++ / Go surfaces, the argument checks that come
before any device work, the encoder's host block plan as a stand-alone program under ASan + UBSan, and the build-quality
guard for the kernels the feature adds or changes, from the compiler's own report (make usage-blob / usage-zstd-encode):
no scratch, no spills, and every earlier kernel of blob.hip, known.hip and zstd_encode.hip still there exactly once."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbs_plus_amd", "csrc")
SYMBOLS = ("pbsgpu_ring_upload_new2_device", "pbsgpu_known_upload_new2_device")
NEW_KERNELS = ("k_upz_pieces", "k_upz_fold")
CHANGED_KERNELS = ("k_upnew_fill", "k_pagecrc_pieces", "k_pagecrc_fold", "k_zenc_blocks", "k_zenc_assemble")
BLOB_BEFORE = ("k_crc_pieces", "k_crc_fold", "k_enc2_pieces", "k_enc2_fold", "k_blob_heads", "k_pagecrc_pieces", "k_pagecrc_fold",
               "k_page_copy", "k_upnew_count", "k_upnew_scan", "k_upnew_fill", "k_upnew_ppart", "k_dec_heads", "k_dec_pieces",
               "k_dec_fold", "k_dec_copy", "k_dec_status")
KNOWN_BEFORE = ("k_known_lookup", "k_known_keys", "k_known_mark", "k_known_insert", "k_known_rehash")
ZENC_BEFORE = ("k_zenc_blocks", "k_zenc_assemble")


@pytest.fixture(scope="module")
def L():
    from pbs_plus_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _params(hdr, name):
    """the parameter list of a declaration in the header, comments removed: ["pbsgpu_ring *ring", ...]"""
    m = re.search(r"^int %s\s*\((.*?)\);" % name, hdr, flags=re.M | re.S)
    assert m, name
    return [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]


def _ctype(param):
    if "*" in param:
        return "ptr"
    return {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int": C.c_int}[param.split()[0]]


def test_new_names_are_declared_exported_and_bound(L):
    from pbs_plus_amd import _lib

    hdr = _read("include", "pbsgpu.h")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (pbsgpu_[a-z0-9_]+)", out))
    assert re.search(r"^#define PBSGPU_HAS_UPLOAD_NEW2 1\b", hdr, flags=re.M)
    assert re.search(r"^#define PBSGPU_ABI_VERSION 5\b", hdr, flags=re.M) and L.pbsgpu_abi_version() == 5
    for name in SYMBOLS:
        assert name in exported and name in _lib.SYMBOLS, name
        res, args = _lib.SYMBOLS[name]
        params = _params(hdr, name)
        assert res is C.c_int and len(args) == len(params), (name, len(args), len(params))
        for a, p in zip(args, params):  # the prototype matches the header, parameter for parameter
            want = _ctype(p)
            if want == "ptr":
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert a is want, (name, p, a)
    assert len(_lib.SYMBOLS[SYMBOLS[0]][1]) == 17 and len(_lib.SYMBOLS[SYMBOLS[1]][1]) == 18
    # the old entry points are still there, with their old prototypes
    assert len(_lib.SYMBOLS["pbsgpu_ring_upload_new_device"][1]) == 13 and "pbsgpu_ring_upload_new_device" in exported
    assert len(_lib.SYMBOLS["pbsgpu_known_upload_new_device"][1]) == 14 and "pbsgpu_known_upload_new_device" in exported
    sec = hdr[hdr.index("---- the fused calls with the blob's kind decided on the device"):hdr.index("int pbsgpu_known_upload_new2_device")]
    assert "converter.go:399" in sec and "converter.go:410-435" in sec and "strictly shorter" in sec


def test_python_cpp_and_go_surfaces():
    from pbs_plus_amd import KnownChunks, PageRing

    sig = inspect.signature(PageRing.upload_new2).parameters
    assert list(sig)[:4] == ["self", "known", "stream", "recs"] and sig["insert"].default is True and sig["zstd"].default is False
    sig = inspect.signature(KnownChunks.upload_new2).parameters
    assert list(sig)[:4] == ["self", "src", "recs", "chunks"] and sig["insert"].default is True and sig["zstd"].default is False
    hpp, go, fb = _read("include", "pbsgpu.hpp"), _read("go", "pbsgpu", "pbsgpu.go"), _read("go", "pbsgpu", "fallback.go")
    for name in SYMBOLS:
        assert name + "(" in hpp, name
        assert re.search(r"\bC\.%s\(" % name, go), name
    assert len(re.findall(r"\bUploadNew2\(", hpp)) == 2 and len(re.findall(r"\bUploadNew\(", hpp)) == 2
    for sig in (r"^func \(r \*Ring\) UploadNew2\(", r"^func \(k \*KnownChunks\) UploadNew2\("):
        assert re.search(sig, go, flags=re.M), sig
        assert re.search(sig, fb, flags=re.M), sig
        body = fb[re.search(sig, fb, flags=re.M).start():]
        assert "ErrNotBuilt" in body[:body.index("}\n")], sig
    assert re.search(r"^type Uploaded2 struct", go, flags=re.M) and re.search(r"^\tUploaded2\s+struct", fb, flags=re.M)


def test_the_cpp_surface_compiles(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "pbsgpu.hpp"\n'
                   "int main() {\n"
                   "    std::vector<pbsgpu_record> recs(2);\n"
                   "    std::vector<pbsgpu_segment> chunks{{0, 10}, {10, 5}};\n"
                   "    pbsgpu::datastore::KnownChunks *k = nullptr;\n"
                   "    pbsgpu::transfer::PageRing *ring = nullptr;\n"
                   "    auto a = k->UploadNew2(nullptr, 0, recs, chunks, true, true, nullptr, 0);\n"
                   "    auto b = ring->UploadNew2(*k, 0, recs, true, true, nullptr, 0);\n"
                   "    if (b.value.encoded.frame_bytes) return 2;\n"
                   "    return a.value.lens.size() == 2 && a.value.kinds.size() == 2 ? 0 : 1;\n"
                   "}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_argument_checks_that_need_no_device(L):
    """an unknown flag bit, a NULL ring or set, NULL where a result must go, n >= 2^32, and in the contiguous form a
    destination that overlaps the source under F_ZSTD: PBSGPU_E_INVALID with every output as it was"""
    from pbs_plus_amd import RECORD_DTYPE, _lib

    E = _lib.E_INVALID
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)  # never dereferenced: the bad argument is found first
    recs = np.zeros(2, dtype=RECORD_DTYPE)
    chunks = np.array([[0, 100], [100, 50]], dtype=np.uint64)
    offs = np.full(2, 7, dtype=np.uint64)
    lens = np.full(2, 7, dtype=np.uint32)
    kinds = np.full(2, 7, dtype=np.uint8)
    used, st, enc = C.c_uint64(123), _lib.DedupStats(), _lib.EncodeStats()
    rp, op, lp, kp, up, sp, ep = recs.ctypes.data, offs.ctypes.data, lens.ctypes.data, kinds.ctypes.data, C.byref(used), C.byref(st), C.byref(enc)
    ring = L.pbsgpu_ring_upload_new2_device
    for flags in (2, 3, 4, 1 << 31):
        assert ring(fake, fake, 0, rp, 2, 1, flags, None, 0, None, op, lp, kp, None, up, sp, ep) == E
    assert ring(None, fake, 0, rp, 2, 1, 1, None, 0, None, op, lp, kp, None, up, sp, ep) == E
    assert ring(fake, None, 0, rp, 2, 1, 1, None, 0, None, op, lp, kp, None, up, sp, ep) == E
    assert ring(fake, fake, 0, rp, 2, 1, 1, None, 0, None, op, lp, kp, None, None, sp, ep) == E
    assert ring(fake, fake, 0, rp, 2, 1, 1, None, 0, None, None, lp, kp, None, up, sp, ep) == E
    assert ring(fake, fake, 0, None, 2, 1, 1, None, 0, None, op, lp, kp, None, up, sp, ep) == E
    assert ring(fake, fake, 0, rp, 2, 1, 1, None, 0, None, op, lp, kp, None, up, None, ep) == E
    assert ring(fake, fake, 0, rp, 1 << 32, 1, 1, None, 0, None, op, lp, kp, None, up, sp, ep) == E
    cont = L.pbsgpu_known_upload_new2_device
    cp = chunks.ctypes.data
    src, dst = 0x10000000, 0x20000000
    for flags in (2, 5):
        assert cont(fake, src, 1024, rp, cp, 2, 1, flags, dst, 4096, None, op, lp, kp, None, up, sp, ep) == E
    assert cont(None, src, 1024, rp, cp, 2, 1, 1, dst, 4096, None, op, lp, kp, None, up, sp, ep) == E
    assert cont(fake, src, 1024, rp, cp, 2, 1, 1, None, 64, None, op, lp, kp, None, up, sp, ep) == E      # room without a destination
    assert cont(fake, src, 149, rp, cp, 2, 1, 1, dst, 4096, None, op, lp, kp, None, up, sp, ep) == E       # the second chunk ends at 150
    assert cont(fake, src, 1024, rp, cp, 2, 1, 1, src, 4096, None, op, lp, kp, None, up, sp, ep) == E      # dst is src
    assert cont(fake, src, 1024, rp, cp, 2, 1, 1, src + 1023, 4096, None, op, lp, kp, None, up, sp, ep) == E   # dst begins at src's last byte
    assert cont(fake, src, 1024, rp, cp, 2, 1, 1, src - 4095, 4096, None, op, lp, kp, None, up, sp, ep) == E   # dst's last byte is src's first
    assert np.all(offs == 7) and np.all(lens == 7) and np.all(kinds == 7) and used.value == 123
    assert list(enc.blobs) == [0, 0] and st.nrecords == 0


def _usage(target):
    """{kernel's mangled name: {figure: value}} from the compiler's report of a usage-* make target"""
    r = subprocess.run(["make", "-s", "-C", CSRC, target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    seen = {}
    for b in re.split(r"remark: Function Name: ", r.stderr + r.stdout)[1:]:
        seen[b.split()[0]] = {m.group(1).strip(): int(m.group(2)) for m in re.finditer(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", b)}
    return seen


def _one(usage, kernel):
    names = [n for n in usage if kernel in n]
    assert len(names) == 1, (kernel, sorted(usage))
    return usage[names[0]]


def test_new_and_changed_kernels_use_no_scratch_and_spill_nothing():
    blob, zenc = _usage("usage-blob"), _usage("usage-zstd-encode")
    for k in BLOB_BEFORE:  # every kernel name blob.hip had before still matches exactly one kernel
        _one(blob, k)
    for k in ZENC_BEFORE:
        _one(zenc, k)
    assert len(zenc) == 2, sorted(zenc)
    for k in NEW_KERNELS:
        assert not [e for e in BLOB_BEFORE + KNOWN_BEFORE + ZENC_BEFORE if e in k or k in e], k
    for k in NEW_KERNELS + CHANGED_KERNELS:
        v = _one(zenc if k.startswith("k_zenc") else blob, k)
        print(k, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["SGPRs Spill"] == 0 and v["VGPRs Spill"] == 0, (k, v)
    assert _one(zenc, "k_zenc_blocks")["LDS Size [bytes/block]"] <= 21596  # seven workgroups still fit a CU


def test_known_kernels_are_still_one_each(tmp_path):
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S",
                          "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "known.hip"), "-o", str(tmp_path / "known.s")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    for k in KNOWN_BEFORE:
        assert len([n for n in names if k in n]) == 1, (k, names)


# ---- the encoder's host block plan (pbs_plus_amd/csrc/zstd_plan.h) as a stand-alone program ---------------------------

def _model(round_blocks, block, lens):
    """(nblocks, most, cuts, first) by the rule: rounds of whole chunks, round_blocks blocks at the most unless one chunk
    alone has more; a round is closed only when the next chunk would not fit"""
    nb = [-(-n // block) for n in lens]
    first = [sum(nb[:c]) for c in range(len(lens))]
    cuts, have = [0], 0
    for c, b in enumerate(nb):
        if have + b > round_blocks and c > cuts[-1]:
            cuts.append(c)
            have = 0
        have += b
    cuts.append(len(lens))
    most = max([sum(nb[a:b]) for a, b in zip(cuts, cuts[1:])], default=0)
    return sum(nb), most, cuts, first


@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "test_zstd_plan")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra"]
    subprocess.run(["g++", *flags, os.path.join(ROOT, "tests", "native", "test_zstd_plan.cpp"), "-o", exe], check=True)
    return exe


def test_the_host_block_plan_equals_the_model(plan_driver):
    """Chosen and seeded random length lists — zero-length chunks, lengths at the block's edges, chunks that alone exceed a
    round, rounds that fill exactly — through the program built with ASan + UBSan, which checks the plan's invariants
    itself; its output is compared with the model here. 2^32 blocks or more are refused."""
    block = 128 << 10
    cases = [(2048, block, []), (2048, block, [0]), (2048, block, [0, 0, 0]), (2048, block, [1]), (2048, block, [block, block + 1, block - 1, 0, 3 * block]),
             (4, block, [block] * 9), (4, block, [4 * block, 4 * block, 1]), (4, block, [5 * block, 1, 9 * block + 1, 0, 0, block]),
             (4, block, [3 * block, 2 * block, 2 * block, 4 * block + 1]), (1, block, [0, 1, 0, 2 * block, 0]),
             (2048, block, [(1 << 32) - 1] * 3), (3, 1, [1, 2, 3, 4, 0, 1, 1, 1])]
    rng = np.random.default_rng(17)
    for _ in range(60):
        n = int(rng.integers(0, 400))
        lens = rng.choice([0, 1, block - 1, block, block + 1, 2 * block, 5 * block + 7, 40 * block], size=n).tolist()
        lens = [int(v) if rng.integers(0, 3) else int(rng.integers(0, 6 * block)) for v in lens]
        cases.append((int(rng.choice([1, 2, 7, 64, 2048])), block, lens))
    refused = [(2048, 1, [(1 << 32) - 1, 1]), (2048, 1, [(1 << 32) - 1] * 2 + [5])]
    text = "".join("%d %d %s\n" % (r, b, " ".join(map(str, lens))) for r, b, lens in cases + refused)
    out = subprocess.run([plan_driver], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == "plan-ok" and len(lines) == len(cases) + len(refused) + 1
    for (r, b, lens), line in zip(cases, lines):
        nblocks, most, cuts, first = _model(r, b, lens)
        head, c, f = line.split("|")
        assert [int(x) for x in head.split()] == [nblocks, most], (r, lens[:8], line[:80])
        assert [int(x) for x in c.split()] == cuts and [int(x) for x in f.split()] == first, (r, lens[:8])
    assert lines[len(cases):-1] == ["refused"] * len(refused)
