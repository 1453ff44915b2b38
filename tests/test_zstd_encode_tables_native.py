"""The zstd encoder's format core (pbs_plus_amd/csrc/zstd_encode.h) in both modes of its sequences section, as a CPU
program under AddressSanitizer + UBSan: a stand-alone program with its own main (tests/native/test_zstd_encode_tables.cpp),
nothing loaded into Python, nothing preloaded. Mode 0 is predefined tables and explicit offsets, the frames of
zstd_enc_v1.json; mode 1 adds repeat codes against a history that starts unknown in every block and per-block tables
(pbsgpu_engine_options.zstd_seq_tables = 1), the frames of zstd_enc_tables_v1.json. Per case and mode the program encodes
into a room of exactly encode_bound(n) between guards, decodes the frame again with zstd_decode.h, and encodes into rooms
too small. Here: the golden files, libzstd where it loads (a frame that leaned on the block before would decode wrongly
there), mode 1 never longer and on the named cases strictly shorter, the same sequences in both modes, and the branches."""
import ctypes as C
import hashlib
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_enc_tables_inputs as ti  # noqa: E402

zi = ti.zi
BIT = {b: i for i, b in enumerate(ti.BRANCHES)}


@pytest.fixture(scope="module")
def run():
    code, out, err, frames, rows = ti.run_native()
    return code, out, err, frames, rows, ti.cases()


def test_every_case_round_trips_in_both_modes_and_small_rooms_are_refused(run):
    code, out, err, frames, rows, cases = run
    assert code == 0 and "zstd-encode-tables-ok" in out, out[-4000:] + err[-4000:]
    assert "runtime error" not in err and "AddressSanitizer" not in err
    for mode in (0, 1):
        assert len(frames[mode]) == len(cases) == len(rows[mode])
        for (name, data), frame, row in zip(cases, frames[mode], rows[mode]):
            assert 0 < len(frame) == row[0] <= zi.bound(len(data)), (name, mode)
            assert frame[:4] == b"\x28\xb5\x2f\xfd" and frame[4] & 0x2f == 0x20, (name, mode)


def test_mode_0_writes_the_frames_it_always_wrote(run):
    """the first cases are zstd_enc_inputs.cases(): their mode-0 frames are the golden ones of the encoder's first tests"""
    code, out, err, frames, rows, cases = run
    golden = zi.golden()
    base = zi.cases()
    assert [name for name, _ in cases[:len(base)]] == [name for name, _ in base] and sorted(golden) == sorted(n for n, _ in base)
    for (name, _), frame in zip(base, frames[0]):
        assert [len(frame), hashlib.sha256(frame).hexdigest()] == golden[name], name


def test_mode_1_writes_the_golden_frames(run):
    code, out, err, frames, rows, cases = run
    golden = ti.golden()
    assert sorted(golden) == sorted(name for name, _ in cases)
    for (name, _), frame in zip(cases, frames[1]):
        assert [len(frame), hashlib.sha256(frame).hexdigest()] == golden[name], name


def test_libzstd_decodes_every_mode_1_frame_to_the_content(run):
    code, out, err, frames, rows, cases = run
    g = zi.zstd_inputs.golden()
    z = g.load_libzstd()
    if z is None:
        pytest.skip("libzstd.so.1 does not load on this machine")
    z.ZSTD_getFrameContentSize.restype = C.c_ulonglong
    z.ZSTD_getFrameContentSize.argtypes = [C.c_void_p, C.c_size_t]
    for (name, data), frame in zip(cases, frames[1]):
        assert z.ZSTD_getFrameContentSize(frame, len(frame)) == len(data), name
        got, errc = g.decompress(z, frame, len(data))
        assert errc is None and got == data, name
    print("libzstd decoded %d frames" % len(frames[1]))


def test_mode_1_is_never_longer_and_shorter_where_sequences_weigh(run):
    code, out, err, frames, rows, cases = run
    by_name = {}
    for (name, data), f0, f1 in zip(cases, frames[0], frames[1]):
        print("%-20s %8d bytes: %8d -> %8d (%.3f)" % (name, len(data), len(f0), len(f1), len(f1) / len(f0)))
        assert len(f1) <= len(f0), name
        by_name[name] = (len(f0), len(f1))
    for name in ti.SHORTER:
        assert by_name[name][1] < by_name[name][0], name


def test_both_modes_find_the_same_sequences(run):
    """the match finder is one: the literals and sequences of the last block are equal, and so is all but the new bits"""
    code, out, err, frames, rows, cases = run
    old = (1 << len(zi.BRANCHES)) - 1
    for (name, _), r0, r1 in zip(cases, rows[0], rows[1]):
        assert r0[2:4] == r1[2:4], name
        assert r0[1] & ~old == 0 and r0[1] == r1[1] & old, name
    by_name = {name: row for (name, _), row in zip(cases, rows[1])}
    for n in (1, 2, 127, 128):
        assert by_name["seqs-%d" % n][3] == n, n
    assert by_name["ofrle"][3] == 16


def test_the_cases_reach_every_branch_of_mode_1(run):
    code, out, err, frames, rows, cases = run
    assert "of %d bits" % len(ti.BRANCHES) in out, out[-2000:]
    cov = 0
    for row in rows[1]:
        cov |= row[1]
    missing = [b for i, b in enumerate(ti.BRANCHES) if not cov >> i & 1]
    print("coverage", hex(cov), "missing", missing)
    assert sorted(missing) == sorted(ti.UNREACHED)


def test_the_crafted_contents_take_the_paths_they_are_built_for(run):
    code, out, err, frames, rows, cases = run
    by_name = {name: row[1] for (name, _), row in zip(cases, rows[1])}
    has = lambda name, *bits: all(by_name[name] >> BIT[b] & 1 for b in bits)  # noqa: E731
    assert has("records-20000", "rep_1", "rep_2", "rep_3") and has("reps-20000", "rep_1", "rep_2", "rep_3")
    for n in (20000, 131072, 131073, 300000):
        assert has("touch-%d" % n, "rep0_1", "rep0_2", "rep0_3"), n
    # a later block's first matches repeat the offsets of the block before, which it does not know
    assert has("touch-300000", "rep_unknown") and not has("touch-131072", "rep_unknown")
    assert has("ofrle", "of_rle") and has("llrle", "ll_rle", "ml_rle")
    for n in (1, 2):  # a description does not pay for one or two sequences ...
        assert has("seqs-%d" % n, "ll_predef", "of_predef", "ml_predef"), n
    for n in (127, 128):  # ... and does for these
        assert has("seqs-%d" % n, "ll_fse", "ml_fse"), n
    assert has("text-131072", "ll_fse", "of_fse", "ml_fse", "ll_log_max", "of_log_max", "ml_log_max")
