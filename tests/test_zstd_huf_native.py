"""The frames of tests/zstd_huf_inputs.py through the CPU build of the zstd format core under AddressSanitizer + UBSan: the
stand-alone program of tests/test_zstd_core_native.py (tests/native/test_zstd_core.cpp, its own main, nothing preloaded),
over this family alone, run as tests/test_zstd_seq_native.py runs it. Every OK case has to come back bit-exact and every
other with its status, through the cuts, the 2 000 mutations per case and the room one byte too small without a sanitizer
report; the family alone has to reach the coverage bits of the Huffman literals, of all four modes of all three sequence
tables, and the six bits that name what only crafted frames reach. Where libzstd loads, every case, cut and mutated frame
it accepts decodes to the same bytes here, but for the reviewed list tests/golden/zstd_huf_v1_refused_here.json (`python
tests/test_zstd_huf_native.py` rewrites it), frames of the kind that the docstring in tests/test_zstd_core_native.py
explains. Every frame that tests/test_gpu_zstd_huf.py expects to be refused has passed this run first."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_huf_inputs  # noqa: E402
import zstd_inputs  # noqa: E402
from test_zstd_core_native import BRANCHES, CRAFTED, _against_libzstd  # noqa: E402
from test_zstd_seq_native import _coverage, _write_cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPROC = 4
GOLDEN = os.path.join(ROOT, "tests", "golden", "zstd_huf_v1.json")
RECORDED = os.path.join(ROOT, "tests", "golden", "zstd_huf_v1_refused_here.json")
REACHED = ("huf_1stream", "huf_4stream_3", "huf_4stream_4", "huf_4stream_5", "huf_treeless", "weights_direct", "weights_fse",
           "ll_predef", "ll_rle", "ll_fse", "ll_repeat", "of_predef", "of_rle", "of_fse", "of_repeat", "ml_predef", "ml_rle", "ml_fse", "ml_repeat")


def _golden_module():
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_zstd_huf_golden", os.path.join(ROOT, "tests", "golden", "make_zstd_huf_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """builds the program and runs it once over the family: (golden module, cases, (exit code, stdout, stderr) per process,
    result lines)"""
    import subprocess

    tmp = tmp_path_factory.mktemp("zstd_huf")
    cases = [dict(c, info=[0, c["length"], c["length"], 9, 0]) for c in zstd_huf_inputs.cases()]
    path = str(tmp / "cases.bin")
    _write_cases(path, cases)
    exe, res = str(tmp / "test_zstd_core"), str(tmp / "results.txt")
    flags = ["-std=c++17", "-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
             "-Wall", "-Wextra"]
    subprocess.run(["g++", *flags, os.path.join(ROOT, "tests", "native", "test_zstd_core.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    procs = [subprocess.Popen([exe, path, "%s.%d" % (res, k), str(NPROC), str(k)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True, env=env) for k in range(NPROC)]
    outs, lines = [], []
    for k, p in enumerate(procs):
        so, se = p.communicate(timeout=900)
        outs.append((p.returncode, so, se))
        if os.path.exists("%s.%d" % (res, k)):
            lines += [ln.split() for ln in open("%s.%d" % (res, k))]
    return zstd_inputs.golden(), cases, outs, lines


def test_the_frames_are_the_recorded_ones():
    """regenerated here byte for byte; set against libzstd when the file was written (tests/golden/make_zstd_huf_golden.py) and,
    where libzstd loads, here again"""
    recorded = json.load(open(GOLDEN))
    cases = zstd_huf_inputs.cases()
    z = zstd_inputs.golden().load_libzstd()
    rows = _golden_module().rows(cases, z)
    if z is None:
        print("libzstd does not load on this machine: its column is taken as recorded")
        rows = [dict(r, libzstd=rec.get("libzstd")) for r, rec in zip(rows, recorded)]
    assert rows == recorded, [r["name"] for r, rec in zip(rows, recorded) if r != rec][:10]
    assert "[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n" == open(GOLDEN).read()
    assert {zstd_huf_inputs.family(c["name"]) for c in cases} == set(zstd_huf_inputs.FAMILIES)
    # libzstd accepts nothing that is refused here; what is OK here alone is the reviewed list and nothing else
    for r in recorded:
        assert r["libzstd"] == ("same" if r["status"] == 0 and not zstd_huf_inputs.ok_here_only(r["name"]) else "error"), r["name"]
    here_only = [r["name"] for r in recorded if r["status"] == 0 and r["libzstd"] == "error"]
    assert len(here_only) == 24 and all(n.startswith(("hufmax-12-", "hufend-", "hufsyms-fse256-max12", "treeless-after-max12")) for n in here_only)
    assert all(c["status"] in (zstd_huf_inputs.OK, zstd_huf_inputs.BAD_FRAME) for c in cases)
    assert all(len(c["frame"]) <= 9 + 4096 + 64 for c in cases if c["status"] != 0)  # (small, whatever they declare)
    assert os.path.getsize(GOLDEN) < 256 << 10 and os.path.getsize(RECORDED) < 256 << 10


def test_every_case_decodes_bit_exact_and_no_mutation_escapes(run):
    g, cases, outs, lines = run
    for code, so, se in outs:
        assert code == 0 and "zstd-core-ok" in so, so[-4000:] + se[-4000:]  # every case's status and bytes, every guard
        assert "runtime error" not in se and "AddressSanitizer" not in se
    per_case = {}
    for ci, kind, *_ in lines:
        per_case.setdefault(int(ci), {}).setdefault(kind, 0)
        per_case[int(ci)][kind] += 1
    for ci, c in enumerate(cases):
        n = len(c["frame"])
        assert per_case[ci]["fixture"] == 1, c["name"]
        assert per_case[ci]["cut"] == min(65, n) + 97 and per_case[ci]["mut"] == 2000, c["name"]
        assert per_case[ci].get("small", 0) == (1 if c["status"] == 0 and c["length"] else 0)
    fixture = {int(ln[0]): [int(v) for v in ln[3:5]] for ln in lines if ln[1] == "fixture"}
    for ci, c in enumerate(cases):  # said once more from the result lines: the program's own comparison passed above
        assert fixture[ci] == [c["status"], c["length"]], c["name"]


def test_the_family_alone_reaches_what_it_is_built_for(run):
    g, cases, outs, lines = run
    reached = _coverage(outs)
    print("reached", sorted(reached))
    assert len(CRAFTED) == 6 and set(CRAFTED) <= set(BRANCHES)
    assert not [b for b in REACHED + CRAFTED if b not in reached]


def test_what_libzstd_decodes_decodes_the_same_here(run):
    g, cases, outs, lines = run
    res = _against_libzstd((g, cases, outs, lines))
    if res is None:
        print("libzstd does not load on this machine: nothing to compare against")
        return
    compared, accepted, differ, checksum_only, ok_here_only = res
    print("compared", compared, "accepted by libzstd", accepted, "of them refused here", len(differ), "ok here and an error there", ok_here_only)
    recorded = json.load(open(RECORDED))
    assert all(row[3] == zstd_inputs.BAD_FRAME for row in recorded)
    assert differ == recorded, ([r for r in differ if r not in recorded][:10], [r for r in recorded if r not in differ][:10])
    assert compared > 400_000 and accepted > 0


if __name__ == "__main__":  # records the list: run where libzstd loads, then review the diff of the file
    import tempfile
    from pathlib import Path

    class _Factory:
        def mktemp(self, name):
            return Path(tempfile.mkdtemp(prefix=name))

    r = run.__wrapped__(_Factory())
    for code, so, se in r[2]:
        print(code, so[-600:], se[-2000:])
    res = _against_libzstd(r)
    print("compared %d, accepted by libzstd %d, refused here %d, ok here only %d" % (res[0], res[1], len(res[2]), res[4]))
    with open(RECORDED, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in res[2]) + "\n]\n")
