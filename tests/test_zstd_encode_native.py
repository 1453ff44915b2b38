"""The zstd encoder's format core (pbs_plus_amd/csrc/zstd_encode.h) as a CPU program under AddressSanitizer + UBSan: a
stand-alone program with its own main (tests/native/test_zstd_encode.cpp), nothing loaded into Python, nothing preloaded.
Per case it encodes into a room of exactly encode_bound(n) between guards, decodes the frame again with zstd_decode.h,
and encodes into rooms too small. Here its frames are set against the golden file, against libzstd where it loads (the
frames are zstd, not merely what our own decoder accepts), and against what a raw-only encoder would write."""
import ctypes as C
import hashlib
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_enc_inputs as zi  # noqa: E402

BIT = {b: i for i, b in enumerate(zi.BRANCHES)}


@pytest.fixture(scope="module")
def run():
    code, out, err, frames, rows = zi.run_native()
    return code, out, err, frames, rows, zi.cases()


def test_every_case_round_trips_within_the_bound_and_small_rooms_are_refused(run):
    code, out, err, frames, rows, cases = run
    assert code == 0 and "zstd-encode-ok" in out, out[-4000:] + err[-4000:]
    assert "runtime error" not in err and "AddressSanitizer" not in err
    assert len(frames) == len(cases) == len(rows)
    for (name, data), frame, row in zip(cases, frames, rows):
        assert 0 < len(frame) == row[1] <= zi.bound(len(data)), name
        assert frame[:4] == b"\x28\xb5\x2f\xfd" and frame[4] & 0x2f == 0x20, name  # single segment, no dictionary, no checksum


def test_the_frames_are_the_golden_ones(run):
    code, out, err, frames, rows, cases = run
    golden = zi.golden()
    assert sorted(golden) == sorted(name for name, _ in cases)
    for (name, _), frame in zip(cases, frames):
        assert [len(frame), hashlib.sha256(frame).hexdigest()] == golden[name], name


def test_the_cases_reach_every_branch(run):
    code, out, err, frames, rows, cases = run
    assert "of %d bits" % len(zi.BRANCHES) in out, out[-2000:]
    cov = 0
    for row in rows:
        cov |= row[2]
    missing = [b for i, b in enumerate(zi.BRANCHES) if not cov >> i & 1]
    print("coverage", hex(cov), "missing", missing)
    assert sorted(missing) == sorted(zi.UNREACHED)


def test_the_crafted_contents_have_the_counts_they_are_built_for(run):
    code, out, err, frames, rows, cases = run
    by_name = {name: row for (name, _), row in zip(cases, rows)}
    for n in (31, 32, 1023, 1024, 4095, 4096, 16383, 16384):
        assert by_name["lits-%d" % n][3:5] == [n, 0], n  # literals, sequences of the (only) block
    for n in (127, 128):
        assert by_name["seqs-%d" % n][4] == n, n
    assert by_name["cap"][4] == zi.SEQ_CAP and by_name["cap"][2] >> BIT["seq_cap"] & 1


def test_libzstd_decodes_every_frame_to_the_content(run):
    """ZSTD_decompress returns the content and ZSTD_getFrameContentSize the length, for every frame the program wrote"""
    code, out, err, frames, rows, cases = run
    g = zi.zstd_inputs.golden()
    z = g.load_libzstd()
    if z is None:
        pytest.skip("libzstd.so.1 does not load on this machine")
    z.ZSTD_getFrameContentSize.restype = C.c_ulonglong
    z.ZSTD_getFrameContentSize.argtypes = [C.c_void_p, C.c_size_t]
    for (name, data), frame in zip(cases, frames):
        assert z.ZSTD_getFrameContentSize(frame, len(frame)) == len(data), name
        got, errc = g.decompress(z, frame, len(data))
        assert errc is None and got == data, name
    print("libzstd decoded %d frames" % len(frames))


def test_against_a_raw_only_encoder(run):
    code, out, err, frames, rows, cases = run
    seen = set()
    for (name, data), frame, row in zip(cases, frames, rows):
        kind, n, cov = name.split("-")[0], len(data), row[2]
        has = lambda b: cov >> BIT[b] & 1  # noqa: E731
        if kind in ("byte", "zeros"):
            assert len(frame) < 64, name
        elif kind == "period3":
            assert n < 6400 or len(frame) * 100 < n, name  # below 1 % (a frame is never below its 9 bytes)
        elif kind in ("text", "mixed") and n >= 4096:
            assert len(frame) < n, name
            assert has("block_compressed") and has("huf_4stream") and (has("nseq_below_128") or has("nseq_2_bytes")), name
        elif kind == "rand" and n:
            assert n < len(frame) <= zi.bound(n), name
        else:
            continue
        seen.add(kind)
    assert seen == {"byte", "zeros", "period3", "text", "mixed", "rand"}
