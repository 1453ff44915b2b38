"""The surfaces of the zstd encoder's long-range mode without a GPU: the engine option zstd_window_log in the header, its
place in the struct against a C compiler, the Python / Go / C++ bindings, the override table's row, the refusal of every
value outside {0, 17, 18, 19} before any device work, and the compiler's resource report for the mode's two block
kernels, which live in a translation unit of their own so that the other two stay the kernels they were."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbs_plus_amd", "csrc")

# every field of pbsgpu_engine_options before this option, with the offset it has always had
BEFORE = dict(inflight=0, sha_form=4, sha_slack_pct=8, sha_dense_pct=12, resolve_par_min=16, sha_many_files_per_core=24,
              stream_sha_cus=28, stream_express_cus=32, stream_ring_slots=36, stream_ctx_pool=40, zstd_seq_tables=44,
              stream_ring_gib=48, stream_page_bytes=56)


@pytest.fixture(scope="module")
def L():
    from pbs_plus_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_header_declares_the_option_where_the_first_reserved_word_was():
    hdr = _read("include", "pbsgpu.h")
    assert re.search(r"^#define PBSGPU_HAS_ZSTD_WINDOW 1\b", hdr, flags=re.M)
    assert re.search(r"^#define PBSGPU_ABI_VERSION 5\b", hdr, flags=re.M)
    opts = hdr[hdr.index("typedef struct pbsgpu_engine_options {"):hdr.index("} pbsgpu_engine_options;")]
    assert re.search(r"uint64_t stream_page_bytes;.*?\n\s*uint32_t zstd_window_log;.*?\n\s*uint32_t reserved1;\s*\n\s*uint64_t reserved\[3\];",
                     opts, flags=re.S)
    assert "PBSGPU_ZSTD_WINDOW_LOG" in opts and "PBSGPU_E_INVALID" in opts and "17, 18, 19" in opts
    sec = hdr[hdr.index("---- zstd frames written on the device"):hdr.index("#define PBSGPU_HAS_ZSTD_ENCODE 1")]
    assert "zstd_window_log" in sec and "never before the chunk's first byte" in sec
    assert re.search(r"slightly\s+LONGER\s+frame\s+than\s+window\s+0", sec)
    assert re.search(r"strictly\s+shorter\s+than\s+the\s+chunk\"\s+is\s+unaffected", sec)


def test_the_option_has_the_place_the_bindings_assume(tmp_path):
    """size and every offset against what gcc makes of include/pbsgpu.h: the struct is 96 bytes as before, the option
    lies where reserved[0] began, and no other field has moved"""
    from pbs_plus_amd import _lib

    names = list(BEFORE) + ["zstd_window_log", "reserved1", "reserved"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pbsgpu.h"\nint main(void) {\n'
                   '    pbsgpu_engine_options o;\n    printf("%zu %zu", sizeof(o), sizeof(o.zstd_window_log));\n'
                   + "".join('    printf(" %%zu", offsetof(pbsgpu_engine_options, %s));\n' % n for n in names)
                   + '    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    size, width, offs = got[0], got[1], dict(zip(names, got[2:]))
    assert (size, width) == (C.sizeof(_lib.EngineOptions), _lib.EngineOptions.zstd_window_log.size) == (96, 4)
    assert {n: offs[n] for n in BEFORE} == BEFORE
    assert (offs["zstd_window_log"], offs["reserved1"], offs["reserved"]) == (64, 68, 72)
    assert [n for n, _ in _lib.EngineOptions._fields_] == names
    for n in names:
        assert getattr(_lib.EngineOptions, n).offset == offs[n], n


def test_python_go_and_cpp_sources_carry_the_option():
    from pbs_plus_amd import Engine

    go, fb, hpp = _read("go", "pbsgpu", "pbsgpu.go"), _read("go", "pbsgpu", "fallback.go"), _read("include", "pbsgpu.hpp")
    assert re.search(r"^\tZstdWindowLog\s+uint32\b", go, flags=re.M) and "zstd_window_log: C.uint32_t(o.ZstdWindowLog)" in go
    opts = fb[fb.index("EngineOptions struct {"):]
    assert re.search(r"\bZstdWindowLog\s+uint32\b", opts[:opts.index("}")])
    assert "zstd_window_log = 17, 18 or 19" in hpp
    assert "zstd_window_log=17" in Engine.__init__.__doc__
    engine = _read("pbs_plus_amd", "csrc", "engine.cpp")
    table = engine[engine.index("static void engine_env_overrides("):engine.index("int pbsgpu_engine_create(")]
    assert '{"PBSGPU_ZSTD_WINDOW_LOG", U32, &o.zstd_window_log},' in table and table.count("getenv(") == 1
    # the launch site picks one of four block kernels by the engine's two options; the new ones are in their own file
    enc, tab, win = (_read("pbs_plus_amd", "csrc", n) for n in ("zstd_encode.hip", "zstd_encode_tables.hip", "zstd_encode_window.hip"))
    assert "launch_blocks_window(" in enc and "e->opt.zstd_seq_tables" in enc and enc.count("__global__") == 2
    assert tab.count("__global__") == 1
    assert win.count("__global__") == 2 and "k_zenc_wblocks" in win and "k_zenc_wtblocks" in win
    assert "ze::WState" in win and "ze::WTState" in win
    tool = _read("tools", "zstd_encode_rate.py")
    assert "--window-log" in tool and "zstd_window_log" in tool


def test_every_value_outside_0_17_18_19_is_refused_before_any_device_work(L, monkeypatch):
    """on a machine without a GPU the valid values get as far as the device count (PBSGPU_E_NO_DEVICE or, with one,
    PBSGPU_OK); any other value is PBSGPU_E_INVALID either way, from the option and from the override row alike"""
    from pbs_plus_amd import _lib, buzhash

    monkeypatch.delenv("PBSGPU_ZSTD_WINDOW_LOG", raising=False)
    monkeypatch.delenv("PBSGPU_ZSTD_SEQ_TABLES", raising=False)
    cfg = buzhash.NewConfig(4096)

    def create(value, tables=0):
        o = _lib.EngineOptions()
        o.zstd_window_log = value
        o.zstd_seq_tables = tables
        h = C.c_void_p()
        rc = L.pbsgpu_engine_create_opt(0, C.byref(cfg._c), C.byref(o), C.byref(h))
        if rc == _lib.OK:
            L.pbsgpu_engine_destroy(h)
        else:
            assert not h.value
        return rc

    valid = create(0)
    assert valid != _lib.E_INVALID
    for good in (17, 18, 19):
        assert create(good) == valid and create(good, 1) == valid, good
    bad_values = [v for v in range(1, 40) if v not in (17, 18, 19)] + [131072, 1 << 17 | 17, 1 << 31, 0xffffffff]
    for bad in bad_values:
        assert create(bad) == _lib.E_INVALID, bad
    for bad in ("1", "16", "20", "131072"):
        monkeypatch.setenv("PBSGPU_ZSTD_WINDOW_LOG", bad)
        assert create(0) == _lib.E_INVALID and create(17) == _lib.E_INVALID, bad
    for good in ("0", "17", "18", "19"):
        monkeypatch.setenv("PBSGPU_ZSTD_WINDOW_LOG", good)
        assert create(0) == valid and create(23) == valid, good  # the row overrides what the caller passed


def _usage(target):
    r = subprocess.run(["make", "-s", "-C", CSRC, target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    seen = {}
    for b in re.split(r"remark: Function Name: ", r.stderr + r.stdout)[1:]:
        seen[b.split()[0]] = {m.group(1).strip(): int(m.group(2)) for m in re.finditer(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", b)}
    return seen


def test_the_new_kernels_use_no_scratch_spill_nothing_and_take_no_more_lds():
    """from the compiler's own report (make usage-zstd-encode-window): the rows DESIGN.md §18 quotes. The table lies in
    global memory, so a workgroup's LDS is not above k_zenc_tblocks' 26 364 bytes; the other two translation units still
    report the kernels they did."""
    win, tab, enc = _usage("usage-zstd-encode-window"), _usage("usage-zstd-encode-tables"), _usage("usage-zstd-encode")
    assert len(win) == 2 and sorted(k for k in ("k_zenc_wblocks", "k_zenc_wtblocks") for n in win if k in n) == \
        ["k_zenc_wblocks", "k_zenc_wtblocks"], sorted(win)
    for name, v in win.items():
        print(name, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["SGPRs Spill"] == 0 and v["VGPRs Spill"] == 0, (name, v)
        assert v["LDS Size [bytes/block]"] <= 26364, (name, v)
    assert len(tab) == 1 and "k_zenc_tblocks" in next(iter(tab))
    (tv,) = tab.values()
    assert tv["LDS Size [bytes/block]"] == 26364 and tv["ScratchSize [bytes/lane]"] == 0
    assert tv["SGPRs Spill"] == 0 and tv["VGPRs Spill"] == 0
    assert len(enc) == 2 and sorted(k for k in ("k_zenc_blocks", "k_zenc_assemble") for n in enc if k in n) == \
        ["k_zenc_assemble", "k_zenc_blocks"], sorted(enc)
    for name, v in enc.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["SGPRs Spill"] == 0 and v["VGPRs Spill"] == 0, (name, v)


def test_the_new_kernels_address_global_memory_only():
    """the device ISA of zstd_encode_window.hip, compiled as the Makefile compiles it: the table, both parts of a two-part
    source and the scratch are reached through global_* instructions; no flat_* access and no scratch_* access"""
    line = subprocess.run(["make", "-n", "-C", CSRC, "usage-zstd-encode-window"], capture_output=True, text=True, check=True).stdout
    cmd = [ln for ln in line.splitlines() if "zstd_encode_window.hip" in ln][0].split()
    cmd = [w for w in cmd if not w.startswith("-Rpass")]
    cmd[cmd.index("-c")] = "-S"
    cmd[cmd.index("-o") + 1] = "-"
    r = subprocess.run(cmd + ["--offload-device-only"], capture_output=True, text=True, cwd=CSRC, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    isa = r.stdout
    assert "k_zenc_wblocks" in isa and "k_zenc_wtblocks" in isa
    assert len(re.findall(r"^\s+global_atomic_u?max", isa, flags=re.M)) >= 2  # the table's insertions
    assert not re.findall(r"^\s+(flat_(?:load|store|atomic)\w*|scratch_(?:load|store)\w*)", isa, flags=re.M)
