"""The zstd encoder's format core (pbs_plus_amd/csrc/zstd_encode.h) with both match finders, as a CPU program under
AddressSanitizer + UBSan: a stand-alone program with its own main (tests/native/test_zstd_encode_window.cpp), nothing
loaded into Python, nothing preloaded. Window 0 is the match finder that never leaves its block, the frames of
zstd_enc_v1.json and zstd_enc_tables_v1.json; window log 17 and 19 (pbsgpu_engine_options.zstd_window_log) let a block's
matches start in the chunk's bytes in front of it, the frames of zstd_enc_window_v1.json. Per case and mode the program
encodes into a room of exactly encode_bound(n) between guards, decodes the frame again with zstd_decode.h, encodes into
rooms too small, and in the window modes encodes the content from two parts as well. Here: the golden files, libzstd where
it loads, the sizes where far repeats are, the window's edges, and the branches."""
import ctypes as C
import hashlib
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_enc_window_inputs as wi  # noqa: E402

ti, zi = wi.ti, wi.zi
BIT = {b: i for i, b in enumerate(wi.BRANCHES)}


@pytest.fixture(scope="module")
def run():
    code, out, err, frames, rows = wi.run_native()
    return code, out, err, frames, rows, wi.cases()


def _sizes(run):
    code, out, err, frames, rows, cases = run
    return {name: {m: len(frames[m][i]) for m in wi.MODES} for i, (name, _) in enumerate(cases)}


def test_every_case_round_trips_in_every_mode_from_one_part_and_from_two_and_small_rooms_are_refused(run):
    code, out, err, frames, rows, cases = run
    assert code == 0 and "zstd-encode-window-ok" in out, out[-4000:] + err[-4000:]
    assert "runtime error" not in err and "AddressSanitizer" not in err
    assert int(out.split("two-part encodes ")[1].split()[0]) > 100
    for m in wi.MODES:
        assert len(frames[m]) == len(cases) == len(rows[m])
        for (name, data), frame, row in zip(cases, frames[m], rows[m]):
            assert 0 < len(frame) == row[0] <= zi.bound(len(data)), (name, m)
            assert frame[:4] == b"\x28\xb5\x2f\xfd" and frame[4] & 0x2f == 0x20, (name, m)


def test_window_0_writes_the_frames_it_always_wrote(run):
    """the same binary, the existing modes: zstd_enc_v1.json without tables, zstd_enc_tables_v1.json with"""
    code, out, err, frames, rows, cases = run
    g0, g1 = zi.golden(), ti.golden()
    base, tables = zi.cases(), ti.cases()
    assert [n for n, _ in cases[:len(tables)]] == [n for n, _ in tables]
    for (name, _), frame in zip(base, frames[(0, 0)]):
        assert [len(frame), hashlib.sha256(frame).hexdigest()] == g0[name], name
    for (name, _), frame in zip(tables, frames[(0, 1)]):
        assert [len(frame), hashlib.sha256(frame).hexdigest()] == g1[name], name


def test_the_window_modes_write_the_golden_frames(run):
    code, out, err, frames, rows, cases = run
    golden = wi.golden()
    assert sorted(golden) == sorted(name for name, _ in cases)
    for m in wi.WINDOW_MODES:
        for (name, _), frame in zip(cases, frames[m]):
            assert [len(frame), hashlib.sha256(frame).hexdigest()] == golden[name][wi.KEY[m]], (name, m)


def test_libzstd_decodes_every_window_frame_to_the_content(run):
    code, out, err, frames, rows, cases = run
    g = zi.zstd_inputs.golden()
    z = g.load_libzstd()
    if z is None:
        pytest.skip("libzstd.so.1 does not load on this machine")
    z.ZSTD_getFrameContentSize.restype = C.c_ulonglong
    z.ZSTD_getFrameContentSize.argtypes = [C.c_void_p, C.c_size_t]
    count = 0
    for m in wi.WINDOW_MODES:
        for (name, data), frame in zip(cases, frames[m]):
            assert z.ZSTD_getFrameContentSize(frame, len(frame)) == len(data), (name, m)
            got, errc = g.decompress(z, frame, len(data))
            assert errc is None and got == data, (name, m)
            count += 1
    print("libzstd decoded %d frames" % count)


def test_far_repeats_are_found(run):
    """strictly shorter than window 0 of the same tables mode where the content repeats further than a block away (or, for
    period70000, further than the small table remembers)"""
    size = _sizes(run)
    for t in (0, 1):
        p = size["period70000-300000"]
        assert p[(17, t)] < p[(0, t)] and 2 * p[(17, t)] < p[(0, t)], p
        mx = size["mixed-1048576"]
        assert mx[(19, t)] < mx[(17, t)] < mx[(0, t)], mx
        d = size["dup200000x3"]
        assert d[(19, t)] < d[(0, t)], d


def test_with_tables_never_longer_than_without_at_the_same_window(run):
    size = _sizes(run)
    for name, s in size.items():
        for w in (0, 17, 19):
            assert s[(w, 1)] <= s[(w, 0)], (name, w)


def test_sizes_per_case_beside_libzstd(run):
    """printed for DESIGN.md §18, not asserted: the mode is not "never longer than window 0" (content without far repeats
    moves by a few dozen bytes either way)"""
    code, out, err, frames, rows, cases = run
    size = _sizes(run)
    g = zi.zstd_inputs.golden()
    z = g.load_libzstd()
    total = {m: 0 for m in wi.MODES}
    lv = {1: 0, 3: 0}
    longer = []
    for name, data in cases:
        s = size[name]
        l1, l3 = (len(g.compress(z, data, level=k)) for k in (1, 3)) if z is not None else (0, 0)
        lv[1] += l1
        lv[3] += l3
        for m in wi.MODES:
            total[m] += s[m]
        if s[(17, 0)] > s[(0, 0)] or s[(19, 0)] > s[(0, 0)]:
            longer.append((name, s[(17, 0)] - s[(0, 0)], s[(19, 0)] - s[(0, 0)]))
        print("%-22s %8d | %s | level 1 %8d level 3 %8d" % (name, len(data), " ".join("%8d" % s[m] for m in wi.MODES), l1, l3))
    print("%-22s %8s | %s | level 1 %8d level 3 %8d" % ("sum", "", " ".join("%8d" % total[m] for m in wi.MODES), lv[1], lv[3]))
    print("longer than window 0 (bytes at 17, at 19):", longer)


def test_the_cases_reach_every_branch(run):
    """lit_rle, which no case reaches at window 0 (a byte value's first occurrence in a block is a literal), is reached
    here: a block's only literals may be of one value when the rest of it matches its history"""
    code, out, err, frames, rows, cases = run
    assert "of %d bits" % len(wi.BRANCHES) in out, out[-2000:]
    cov = 0
    for m in wi.WINDOW_MODES:
        if m[1]:
            for row in rows[m]:
                cov |= row[1]
    missing = [b for i, b in enumerate(wi.BRANCHES) if not cov >> i & 1]
    print("coverage", hex(cov), "missing", missing)
    assert missing == []
    for m in wi.MODES[:2]:  # the match finder that never leaves its block sets none of the new bits
        for row in rows[m]:
            assert not any(row[1] >> BIT[b] & 1 for b in wi.NEW)


def test_the_windows_edges(run):
    """literals and sequences of the last block, and the branches, of the crafted contents: the pattern is one sequence
    when the window holds its first occurrence and 24 literals when not"""
    code, out, err, frames, rows, cases = run
    idx = {name: i for i, (name, _) in enumerate(cases)}
    last = lambda name, m: tuple(rows[m][idx[name]][2:4])  # noqa: E731
    has = lambda name, m, *bits: all(rows[m][idx[name]][1] >> BIT[b] & 1 for b in bits)  # noqa: E731
    for t in (0, 1):
        w0, w17, w19 = (0, t), (17, t), (19, t)
        # window 0: the first batch of 64 zeros, the pattern and the byte behind it are literals
        for name in ("edge-far", "edge-beyond", "edge-off131072", "edge-code19"):
            assert last(name, w0)[0] == 64 + 24 + 1, name
        # exactly at the far edge: taken at 17; one byte beyond: the pattern's first byte is a literal at 17 and not at 19
        assert last("edge-far", w17) == last("edge-far", w19) == (1, 4)
        assert last("edge-beyond", w17) == (2, 4) and last("edge-beyond", w19) == (1, 4)
        assert has("edge-beyond", w17, "w_beyond") and not has("edge-beyond", w19, "w_beyond")
        # from the last three history bytes into the block
        assert has("edge-cross", w17, "w_cand_history", "w_cross") and last("edge-cross", w17)[0] == last("edge-cross", w0)[0] - 41
        # offset 131 072 exactly
        assert last("edge-off131072", w17) == (1, 4) and not has("edge-off131072", w17, "w_of_18")
        # an offset above 1 << 19: offset code 19, found by window 19 alone
        assert last("edge-code19", w17) == (24 + 1, 3) and not has("edge-code19", w17, "w_of_18")
        assert last("edge-code19", w19) == (1, 4) and has("edge-code19", w19, "w_of_18", "w_chunk_start")
        # a second block of one byte, and of two, behind a history the chunk's start cuts
        assert has("text-131073", w17, "w_chunk_start", "block_rle") and has("text-131074", w17, "w_chunk_start")
        assert last("text-131074", w17) == (2, 0)
