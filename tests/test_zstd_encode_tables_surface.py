"""The surfaces of the zstd encoder's second mode without a GPU: the engine option zstd_seq_tables in the header, its place
in the struct against a C compiler, the Python / Go / C++ bindings, the override table's row, and the compiler's resource
report for the mode's block kernel, which lives in a translation unit of its own so that zstd_encode.hip stays the two
kernels it was."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbs_plus_amd", "csrc")


@pytest.fixture(scope="module")
def L():
    from pbs_plus_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_header_declares_the_option_where_reserved0_was():
    hdr = _read("include", "pbsgpu.h")
    assert re.search(r"^#define PBSGPU_HAS_ZSTD_SEQ_TABLES 1\b", hdr, flags=re.M)
    assert re.search(r"^#define PBSGPU_ABI_VERSION 5\b", hdr, flags=re.M)
    opts = hdr[hdr.index("typedef struct pbsgpu_engine_options {"):hdr.index("} pbsgpu_engine_options;")]
    assert "reserved0;" not in opts
    assert re.search(r"uint32_t stream_ctx_pool;.*?\n\s*uint32_t zstd_seq_tables;.*?\n\s*double stream_ring_gib;", opts, flags=re.S)
    assert "PBSGPU_ZSTD_SEQ_TABLES" in opts and "PBSGPU_E_INVALID" in opts
    # the encoder's section no longer promises predefined tables for every frame, and says what does not change
    sec = hdr[hdr.index("---- zstd frames written on the device"):hdr.index("#define PBSGPU_HAS_ZSTD_ENCODE 1")]
    assert "zstd_seq_tables" in sec and "never Repeat_Mode" in sec and "never longer" in sec
    assert "starts unknown in every block" in sec


def test_the_option_has_the_place_the_bindings_assume(tmp_path):
    """offset and size against what gcc makes of include/pbsgpu.h, and the struct's size unchanged by the rename"""
    from pbs_plus_amd import _lib

    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pbsgpu.h"\nint main(void) {\n'
                   '    pbsgpu_engine_options o;\n'
                   '    printf("%zu %zu %zu %zu %zu\\n", sizeof(o), offsetof(pbsgpu_engine_options, zstd_seq_tables),\n'
                   '           sizeof(o.zstd_seq_tables), offsetof(pbsgpu_engine_options, stream_ctx_pool),\n'
                   '           offsetof(pbsgpu_engine_options, stream_ring_gib));\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, off, width, before, after = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    f = _lib.EngineOptions.zstd_seq_tables
    assert (size, off, width) == (C.sizeof(_lib.EngineOptions), f.offset, f.size) == (96, 44, 4)
    assert before == off - 4 and after == off + 4  # where reserved0 was: nothing moved
    assert "reserved0" not in [n for n, _ in _lib.EngineOptions._fields_]


def test_python_go_and_cpp_sources_carry_the_option():
    go, fb, hpp = _read("go", "pbsgpu", "pbsgpu.go"), _read("go", "pbsgpu", "fallback.go"), _read("include", "pbsgpu.hpp")
    assert re.search(r"^\tZstdSeqTables\s+uint32\b", go, flags=re.M) and "zstd_seq_tables: C.uint32_t(o.ZstdSeqTables)" in go
    opts = fb[fb.index("EngineOptions struct {"):]
    assert re.search(r"\bZstdSeqTables\s+uint32\b", opts[:opts.index("}")])
    assert "zstd_seq_tables = 1" in hpp
    engine = _read("pbs_plus_amd", "csrc", "engine.cpp")
    table = engine[engine.index("static void engine_env_overrides("):engine.index("int pbsgpu_engine_create(")]
    assert '{"PBSGPU_ZSTD_SEQ_TABLES", U32, &o.zstd_seq_tables},' in table and table.count("getenv(") == 1
    assert "o.zstd_seq_tables > 1" in engine
    # the launch site picks the block kernel by the engine's option; the new kernel is not in zstd_encode.hip
    enc, tab = _read("pbs_plus_amd", "csrc", "zstd_encode.hip"), _read("pbs_plus_amd", "csrc", "zstd_encode_tables.hip")
    assert "e->opt.zstd_seq_tables" in enc and "launch_blocks_tables(" in enc and enc.count("__global__") == 2
    assert tab.count("__global__") == 1 and "k_zenc_tblocks" in tab and "ze::TState" in tab


def test_a_value_other_than_0_and_1_is_refused_before_any_device_work(L, monkeypatch):
    """on a machine without a GPU the valid values get as far as the device count (PBSGPU_E_NO_DEVICE or, with one,
    PBSGPU_OK); 2 is PBSGPU_E_INVALID either way, from the option and from the override row alike"""
    from pbs_plus_amd import _lib, buzhash

    monkeypatch.delenv("PBSGPU_ZSTD_SEQ_TABLES", raising=False)
    cfg = buzhash.NewConfig(4096)

    def create(value):
        o = _lib.EngineOptions()
        o.zstd_seq_tables = value
        h = C.c_void_p()
        rc = L.pbsgpu_engine_create_opt(0, C.byref(cfg._c), C.byref(o), C.byref(h))
        if rc == _lib.OK:
            L.pbsgpu_engine_destroy(h)
        else:
            assert not h.value
        return rc

    valid = create(0)
    assert valid != _lib.E_INVALID and create(1) == valid
    for bad in (2, 3, 1 << 31, 0xffffffff):
        assert create(bad) == _lib.E_INVALID, bad
    monkeypatch.setenv("PBSGPU_ZSTD_SEQ_TABLES", "2")
    assert create(0) == _lib.E_INVALID
    monkeypatch.setenv("PBSGPU_ZSTD_SEQ_TABLES", "1")
    assert create(0) == valid


def _usage(target):
    r = subprocess.run(["make", "-s", "-C", CSRC, target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    seen = {}
    for b in re.split(r"remark: Function Name: ", r.stderr + r.stdout)[1:]:
        seen[b.split()[0]] = {m.group(1).strip(): int(m.group(2)) for m in re.finditer(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", b)}
    return seen


def test_the_new_kernel_uses_no_scratch_spills_nothing_and_four_fit_a_cu():
    """from the compiler's own report (make usage-zstd-encode-tables): the row DESIGN.md §16 quotes. The grid runs four
    workgroups per CU, so four States must fit a CU's 160 KiB of LDS; zstd_encode.hip still reports its two kernels."""
    tab, enc = _usage("usage-zstd-encode-tables"), _usage("usage-zstd-encode")
    assert len(tab) == 1, sorted(tab)
    (name, v), = tab.items()
    print(name, v)
    assert "k_zenc_tblocks" in name and "k_zenc_blocks" not in name and "k_zenc_assemble" not in name
    assert v["ScratchSize [bytes/lane]"] == 0 and v["SGPRs Spill"] == 0 and v["VGPRs Spill"] == 0, v
    assert v["LDS Size [bytes/block]"] * 4 <= 160 << 10, v
    assert len(enc) == 2 and sorted(k for k in ("k_zenc_blocks", "k_zenc_assemble") for n in enc if k in n) == \
        ["k_zenc_assemble", "k_zenc_blocks"], sorted(enc)
