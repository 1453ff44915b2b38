"""The frames of tests/zstd_seq_inputs.py through the CPU build of the zstd format core under AddressSanitizer + UBSan: the
stand-alone program of tests/test_zstd_core_native.py (tests/native/test_zstd_core.cpp, its own main, nothing preloaded),
over this family alone. Every OK case has to come back bit-exact and every stale-* case BAD_FRAME, through the cuts, the
2 000 mutations per case and the room one byte too small without a sanitizer report; the family alone has to reach every
coverage bit of the cooperation paths (which the one CPU lane walks as branches; the lanes themselves exist only on the
device, tests/test_gpu_zstd_seq.py); where libzstd loads, every cut or mutated frame it accepts decodes to the same bytes
here, but for the reviewed list tests/golden/zstd_seq_v1_refused_here.json (`python tests/test_zstd_seq_native.py` rewrites
it), frames of the kind that the docstring in tests/test_zstd_core_native.py explains. Any frame the GPU test expects to be
refused has passed this run first."""
import hashlib
import json
import os
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_inputs  # noqa: E402
import zstd_seq_inputs  # noqa: E402
from test_zstd_core_native import BRANCHES, CRAFTED, _against_libzstd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPROC = 4
COOPERATION = ("match_wait", "match_no_wait", "match_src_in_prev_match", "match_src_own_literals", "lit_short", "lit_long",
               "batch_follows_batch")
GOLDEN = os.path.join(ROOT, "tests", "golden", "zstd_seq_v1.json")
RECORDED = os.path.join(ROOT, "tests", "golden", "zstd_seq_v1_refused_here.json")


def _write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            name = c["name"].encode()
            f.write(struct.pack("<I", len(name)) + name + struct.pack("<BQ", c["status"], len(c["frame"])) + c["frame"])
            f.write(struct.pack("<Q", len(c["content"])) + c["content"])


def _coverage(outs):
    cov = 0
    for code, so, se in outs:
        word = [w for w in so.split() if w.startswith("0x")]
        assert word and "of %d bits" % len(BRANCHES) in so, so[-2000:]
        cov |= int(word[0], 16)
    return {b for i, b in enumerate(BRANCHES) if cov >> i & 1}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """builds the program and runs it once over the family and once over the table-leaving fixture alone: (golden module,
    cases, (exit code, stdout, stderr) per process, result lines, the same three of the fixture's run)"""
    tmp = tmp_path_factory.mktemp("zstd_seq")
    cases = [dict(c, info=[0, c["length"], c["length"], 9, 0]) for c in zstd_seq_inputs.cases()]
    path, one = str(tmp / "cases.bin"), str(tmp / "one.bin")
    _write_cases(path, cases)
    _write_cases(one, [c for c in zstd_inputs.cases() if c["name"] == zstd_seq_inputs.TABLE_LEAVING])
    exe, res = str(tmp / "test_zstd_core"), str(tmp / "results.txt")
    flags = ["-std=c++17", "-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
             "-Wall", "-Wextra"]
    subprocess.run(["g++", *flags, os.path.join(ROOT, "tests", "native", "test_zstd_core.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    procs = [subprocess.Popen([exe, path, "%s.%d" % (res, k), str(NPROC), str(k)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True, env=env) for k in range(NPROC)]
    procs.append(subprocess.Popen([exe, one, res + ".one", "1", "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env))
    outs, lines = [], []
    for k, p in enumerate(procs):
        so, se = p.communicate(timeout=900)
        outs.append((p.returncode, so, se))
        if k < NPROC and os.path.exists("%s.%d" % (res, k)):
            lines += [ln.split() for ln in open("%s.%d" % (res, k))]
    return zstd_inputs.golden(), cases, outs[:NPROC], lines, outs[NPROC]


def test_the_frames_are_the_recorded_ones():
    """regenerated here, set against libzstd when the file was written (tests/golden/make_zstd_seq_golden.py)"""
    recorded = json.load(open(GOLDEN))
    cases = zstd_seq_inputs.cases()
    assert [r["name"] for r in recorded] == [c["name"] for c in cases]
    for r, c in zip(recorded, cases):
        assert (r["status"], r["frame_length"], r["length"]) == (c["status"], len(c["frame"]), c["length"]), c["name"]
        assert r["frame_sha256"] == hashlib.sha256(c["frame"]).hexdigest() and r["sha256"] == c["sha256"].hex(), c["name"]
    fams = {zstd_seq_inputs.family(c["name"]) for c in cases}
    assert fams == {"seen", "chain", "overlap", "own", "lit", "batch", "blocks", "rep", "stale", "seeded"}
    assert sorted(c["name"] for c in cases if c["status"] != 0) == ["stale-ll-repeat", "stale-ml-repeat", "stale-of-repeat", "stale-treeless"]
    assert os.path.getsize(GOLDEN) < 256 << 10 and os.path.getsize(RECORDED) < 256 << 10


def test_every_case_decodes_bit_exact_and_no_mutation_escapes(run):
    g, cases, outs, lines, one = run
    for code, so, se in outs + [one]:
        assert code == 0 and "zstd-core-ok" in so, so[-4000:] + se[-4000:]  # every fixture's status and bytes, every guard
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


def test_the_family_alone_reaches_every_cooperation_branch(run):
    g, cases, outs, lines, one = run
    reached = _coverage(outs)
    print("reached", sorted(reached))
    assert set(COOPERATION) <= set(BRANCHES[-len(COOPERATION) - len(CRAFTED):-len(CRAFTED)])
    assert not [b for b in COOPERATION if b not in reached]
    # ... and what else the family is built for
    for b in ("block_raw", "block_rle", "many_blocks", "lit_raw_1", "lit_raw_2", "lit_raw_3", "lit_rle_1", "lit_rle_2", "huf_treeless",
              "nseq_1", "nseq_2", "ll_repeat", "of_repeat", "ml_repeat", "rep_1", "rep_2", "rep_3", "rep_shifted", "rep_1_minus_1",
              "match_overlap", "match_offset_1", "match_across_blocks"):
        assert b in reached, b


def test_the_table_leaving_fixture_leaves_a_huffman_table_and_three_described_tables(run):
    """what tests/test_gpu_zstd_seq.py puts in front of the stale-* frames, by the coverage of that case alone"""
    g, cases, outs, lines, one = run
    reached = _coverage([one])
    assert all(b in reached for b in zstd_seq_inputs.TABLE_LEAVING_BRANCHES), sorted(reached)
    assert any(b in reached for b in ("huf_1stream", "huf_4stream_3", "huf_4stream_4", "huf_4stream_5"))
    assert not any(b in reached for b in zstd_seq_inputs.TABLE_LEAVING_NOT), sorted(reached)


def test_what_libzstd_decodes_decodes_the_same_here(run):
    g, cases, outs, lines, one = run
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
    res = _against_libzstd(r[:4])
    print("compared %d, accepted by libzstd %d, refused here %d, ok here only %d" % (res[0], res[1], len(res[2]), res[4]))
    with open(RECORDED, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in res[2]) + "\n]\n")
