"""Held ring pages and the ring-sourced blob encode (pbsgpu_ring_release / _held / _blob_encode_device / _copy_device,
PBSGPU_RING_F_HOLD_PAGES) without a GPU: the C ABI and the Python / C++ / Go surfaces, the argument checks that come
before any device work, the held-page bookkeeping (pbs_plus_amd/csrc/hold.h) against a model under random interleavings,
and the build-quality guard for the kernels the feature adds to blob.hip (no scratch, no spills, no flat_* instructions)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pbsgpu_ring_release", "pbsgpu_ring_held", "pbsgpu_ring_blob_encode_device", "pbsgpu_ring_copy_device")
NEW_KERNELS = ("k_pagecrc_pieces", "k_pagecrc_fold", "k_page_copy")


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
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in exported, name
        assert name in _lib.SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    # the fifth name is the flag; the feature macro; the ABI version stays (additive)
    assert re.search(r"^#define PBSGPU_RING_F_HOLD_PAGES 512u", hdr, flags=re.M)
    assert re.search(r"^#define PBSGPU_HAS_RING_UPLOAD 1\b", hdr, flags=re.M)
    assert re.search(r"^#define PBSGPU_RING_ANY_STREAM 0xffffffffu", hdr, flags=re.M)
    assert re.search(r"^#define PBSGPU_ABI_VERSION 5\b", hdr, flags=re.M)
    assert _lib.RING_F_HOLD_PAGES == 512 and _lib.RING_ANY_STREAM == 0xFFFFFFFF


def test_python_cpp_and_go_surfaces():
    from pbs_plus_amd import PageRing

    for m in ("release", "held", "blob_encode", "copy"):
        assert callable(getattr(PageRing, m)), m
    import inspect

    assert "hold" in inspect.signature(PageRing.__init__).parameters
    hpp = _read("include", "pbsgpu.hpp")
    go = _read("go", "pbsgpu", "pbsgpu.go")
    fb = _read("go", "pbsgpu", "fallback.go")
    for name in SYMBOLS:
        assert name + "(" in hpp, name
        assert re.search(r"\bC\.%s\(" % name, go), name
    assert "C.PBSGPU_RING_F_HOLD_PAGES" in go and re.search(r"^\tHoldPages\s+bool", go, flags=re.M)
    for sig in (r"^func \(r \*Ring\) Release\(", r"^func \(r \*Ring\) Held\(", r"^func \(r \*Ring\) EncodeBlobs\(",
                r"^func \(r \*Ring\) Copy\("):
        assert re.search(sig, go, flags=re.M), sig
        assert re.search(sig, fb, flags=re.M), sig
    assert re.search(r"HoldPages\s+bool", fb)


def test_null_handles_and_null_outputs_are_invalid(L):
    """The checks that come before the ring is looked at: a NULL ring, and NULL where a result must go."""
    from pbs_plus_amd import RECORD_DTYPE, _lib

    E = _lib.E_INVALID
    fake = C.cast(C.create_string_buffer(256), C.c_void_p)  # never dereferenced: the NULL output is found first
    recs = np.zeros(2, dtype=RECORD_DTYPE)
    offs = np.zeros(2, dtype=np.uint64)
    first, pages, used = C.c_uint64(), C.c_uint32(), C.c_uint64()
    assert L.pbsgpu_ring_release(None, 0, 0) == E
    assert L.pbsgpu_ring_held(None, 0, C.byref(first), C.byref(pages)) == E
    assert L.pbsgpu_ring_held(fake, 0, None, C.byref(pages)) == E
    assert L.pbsgpu_ring_held(fake, 0, C.byref(first), None) == E
    enc = L.pbsgpu_ring_blob_encode_device
    assert enc(None, 0, recs.ctypes.data, 2, None, None, 0, offs.ctypes.data, None, C.byref(used)) == E
    assert enc(fake, 0, recs.ctypes.data, 2, None, None, 0, offs.ctypes.data, None, None) == E
    assert enc(fake, 0, None, 2, None, None, 0, offs.ctypes.data, None, C.byref(used)) == E
    assert enc(fake, 0, recs.ctypes.data, 2, None, None, 0, None, None, C.byref(used)) == E
    assert L.pbsgpu_ring_copy_device(None, 0, 0, 16, fake) == E
    assert L.pbsgpu_ring_copy_device(fake, 0, 0, 16, None) == E


# ---- the held-page bookkeeping against a model ----

class _Model:
    """A page goes back to the free list when BOTH hold: the services have handed it back, and it lies wholly below its
    stream's watermark — or its stream was closed."""

    def __init__(self, npages, nstreams, page):
        self.page = page
        self.free = set(range(npages))
        self.owner = {}                      # phys -> [slot, k, handed_back]; an orphan (closed stream) has slot None
        self.mark = [0] * nstreams
        self.next_k = [0] * nstreams
        self.is_open = [False] * nstreams

    def _free(self, phys, freed):
        assert phys not in self.free, "freed twice"
        self.free.add(phys)
        del self.owner[phys]
        freed.append(phys)

    def open(self, s):
        self.mark[s], self.next_k[s], self.is_open[s] = 0, 0, True
        return []

    def assign(self, s, k, phys):
        assert phys in self.free and k == self.next_k[s]
        self.free.discard(phys)
        self.next_k[s] += 1
        self.owner[phys] = [s, k, False]
        return []

    def back(self, phys):
        freed = []
        s, k, handed = self.owner[phys]
        assert not handed
        self.owner[phys][2] = True
        if s is None or (k + 1) * self.page <= self.mark[s]:
            self._free(phys, freed)
        return freed

    def release(self, s, upto):
        freed = []
        self.mark[s] = max(self.mark[s], upto)
        for phys, (os_, k, handed) in sorted(self.owner.items()):
            if os_ == s and handed and (k + 1) * self.page <= self.mark[s]:
                self._free(phys, freed)
        return freed

    def close(self, s):
        freed = []
        for phys, (os_, k, handed) in sorted(self.owner.items()):
            if os_ != s:
                continue
            if handed:
                self._free(phys, freed)
            else:
                self.owner[phys][0] = None
        self.is_open[s] = False
        self.mark[s] = 0
        return freed

    def state(self):
        out = []
        for s in range(len(self.mark)):
            held = sum(1 for os_, _, handed in self.owner.values() if os_ == s and handed)
            out += [self.mark[s] // self.page * self.page, held]
        return out

    def phys_of(self, s, k):
        for phys, (os_, kk, _) in self.owner.items():
            if os_ == s and kk == k and k >= self.mark[s] // self.page:
                return phys
        return -1


def _interleaving(seed, npages, nstreams, page, steps):
    """(operations as driver lines, the model's answer to each)"""
    rng = np.random.default_rng(seed)
    m = _Model(npages, nstreams, page)
    ops, want = ["init %d %d %d" % (npages, nstreams, page)], [([], m.state())]
    for _ in range(steps):
        s = int(rng.integers(0, nstreams))
        out = [p for p, o in m.owner.items() if not o[2]]
        kind = rng.choice(["assign", "assign", "assign", "back", "back", "back", "release", "release", "close", "phys"])
        if not m.is_open[s]:
            ops.append("open %d" % s)
            want.append((m.open(s), m.state()))
        elif kind == "assign" and m.free:
            phys = int(rng.choice(sorted(m.free)))
            k = m.next_k[s]
            ops.append("assign %d %d %d" % (s, k, phys))
            want.append((m.assign(s, k, phys), m.state()))
        elif kind == "back" and out:
            phys = int(rng.choice(sorted(out)))
            ops.append("back %d" % phys)
            want.append((m.back(phys), m.state()))
        elif kind == "release":
            hi = m.next_k[s] * page
            # forward by bytes, to a page edge, one short of / one past an edge, or BACKWARDS (a no-op)
            upto = int(rng.choice([int(rng.integers(0, hi + 1)), hi, max(hi - 1, 0), hi // page // 2 * page + 1,
                                   m.mark[s] // 2]))
            ops.append("release %d %d" % (s, upto))
            want.append((m.release(s, upto), m.state()))
        elif kind == "close" and rng.integers(0, 3) == 0:
            ops.append("close %d" % s)
            want.append((m.close(s), m.state()))
        else:
            k = int(rng.integers(0, m.next_k[s] + 2))
            ops.append("phys %d %d" % (s, k))
            want.append(m.phys_of(s, k))
    return ops, want


@pytest.fixture(scope="module")
def hold_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hold") / "test_hold")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra"]
    subprocess.run(["g++", *flags, os.path.join(ROOT, "tests", "native", "test_hold.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("seed,npages,nstreams,page", [(1, 8, 1, 4096), (2, 24, 3, 65536), (3, 64, 5, 1 << 24),
                                                       (4, 5, 4, 512), (5, 200, 16, 262144)])
def test_held_page_bookkeeping_equals_the_model(hold_driver, seed, npages, nstreams, page):
    """Seeded random interleavings of "page (stream, k) handed back", release(stream, upto) and close: after every step
    the pages freed by that step and every stream's (first available offset, pages held) equal the model's; the model
    itself asserts that no page is freed twice, and frees a page only once it was handed back AND lies wholly below the
    watermark (or its stream is closed). Built with ASan + UBSan."""
    ops, want = _interleaving(seed, npages, nstreams, page, 6000)
    out = subprocess.run([hold_driver], input="\n".join(ops) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == "hold-ok" and len(lines) == len(ops) + 1
    nfreed = 0
    for i, (op, line, w) in enumerate(zip(ops, lines, want)):
        if op.startswith("phys"):
            assert line == "phys %d" % w, (i, op, line, w)
            continue
        left, right = line.split("|")
        freed = sorted(int(x) for x in left.split()[1:])
        assert freed == sorted(w[0]), (i, op, freed, w[0])
        assert [int(x) for x in right.split()] == w[1], (i, op, right, w[1])
        nfreed += len(freed)
    assert nfreed > npages  # pages went round more than once


def test_new_kernels_do_not_spill_and_use_no_flat_memory_instructions(tmp_path):
    """The method of tests/test_blob_surface.py on the kernels this feature adds to blob.hip."""
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
    for k in NEW_KERNELS:
        names = [n for n in usage if k in n]
        assert len(names) == 1, (k, list(usage))
        r = usage[names[0]]
        assert r.get("scratch", -1) == 0 and r.get("sgpr_spill", -1) == 0 and r.get("vgpr_spill", -1) == 0, (k, r)
        m = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape(names[0]), text, flags=re.S | re.M)
        assert m, k
        body = m.group(1).splitlines()
        assert not [ln for ln in body if re.match(r"\s+flat_", ln)], k
        assert not [ln for ln in body if re.match(r"\s+scratch_", ln)], k
        assert [ln for ln in body if re.match(r"\s+global_", ln)], k
    # the piece kernel reads its tables from LDS and stores what it loads: every source byte read once, written once
    m = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape([n for n in usage if "k_pagecrc_pieces" in n][0]), text,
                  flags=re.S | re.M)
    body = m.group(1).splitlines()
    assert [ln for ln in body if re.match(r"\s+ds_read", ln)]
    assert [ln for ln in body if re.match(r"\s+global_load_dwordx4", ln)]
    assert [ln for ln in body if re.match(r"\s+global_store_dwordx4", ln)]
