"""The literal half of the device zstd decoder (k_zstd_frames: zstd.hip; decode_block, huf_read_table and huf_stream of
zstd_decode.h) and its table builds (fse_read_norm, fse_build as compiled for the device) against the frames of
tests/zstd_huf_inputs.py: Huffman literals in one and in four streams at the edges of the table, of a stream's end and of
the section's geometry, treeless blocks, and sequence tables that are described, RLE or repeated. Expected contents are
known by construction in that module; nothing here needs libzstd. The four streams run on four lanes only on the device,
so a stream that fails alone, and the State a workgroup keeps from one frame to the next, are tested nowhere else. The
destinations are the guarded ones of tests/test_gpu_zstd.py. Every frame that must be refused here is refused by an
explicit bound of the decoder and went through the sanitizer run of tests/test_zstd_huf_native.py first (the stale-*
frames: tests/test_zstd_seq_native.py)."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_huf_inputs  # noqa: E402
import zstd_inputs  # noqa: E402
import zstd_seq_inputs  # noqa: E402
from test_gpu_blob_decode2 import _Guarded as _RestoreGuarded  # noqa: E402
from test_gpu_blob_decode2 import BAD_DATA, _blob  # noqa: E402
from test_gpu_zstd import FILL, _Guarded  # noqa: E402
from test_gpu_zstd_seq import OUT_MAX, _check, _check_all, _cus, _laid_out, _room  # noqa: E402

pytestmark = pytest.mark.gpu

STALE_REPEAT = ("stale-ll-repeat", "stale-of-repeat", "stale-ml-repeat")
FAILURES = ("short1", "spare11", "empty")  # a stream one bit short, one with as many spare bits as the table is deep, one of no bytes
BAD_FRAME = zstd_inputs.BAD_FRAME


def _failing(s, kind):
    return "hufgeom-empty-s%d" % s if kind == "empty" else "hufend-11-4stream-s%d-%s" % (s, kind)


@pytest.fixture(scope="module")
def world():
    """(engine, cases by name, device buffer of all frames 0-6 bytes apart, frame range by name, guarded destination): the
    family and the stale-*-repeat frames of tests/zstd_seq_inputs.py"""
    from pbs_plus_amd import Engine, buzhash

    eng = Engine(buzhash.NewConfig(4096), device=0)
    allc = list(zstd_huf_inputs.cases()) + [c for c in zstd_seq_inputs.cases() if c["name"] in STALE_REPEAT]
    rng = np.random.default_rng(43)
    parts, ranges, pos = [], {}, 0
    for c in allc:
        gap = int(rng.integers(0, 7))
        parts.append(bytes(gap) + c["frame"])
        ranges[c["name"]] = (pos + gap, len(c["frame"]))
        pos += gap + len(c["frame"])
    host = np.frombuffer(b"".join(parts), np.uint8)
    dev = eng.alloc(host.size)
    dev.upload(host)
    g = _Guarded(eng, OUT_MAX)
    yield eng, {c["name"]: c for c in allc}, dev, ranges, g
    g.free()
    dev.free()
    eng.close()


def _run(world, cs, seed):
    eng, by_name, dev, ranges, g = world
    out, need = _laid_out(cs, np.random.default_rng(seed))
    assert need <= OUT_MAX
    got, status, decoded = g.run(dev, np.array([ranges[c["name"]] for c in cs], np.uint64), out, need)
    _check_all(cs, out, got, status, decoded)
    return out, got, status, decoded


@pytest.mark.parametrize("fam", zstd_huf_inputs.FAMILIES)
def test_every_case_alone(world, fam):
    eng, by_name, dev, ranges, g = world
    names = [c["name"] for c in zstd_huf_inputs.cases() if zstd_huf_inputs.family(c["name"]) == fam]
    assert names
    for name in names:  # every case in a call of its own, into a room of exactly its size
        c = by_name[name]
        got, status, decoded = g.run(dev, np.array([ranges[name]], np.uint64), [(0, _room(c))], _room(c))
        _check(c, int(status[0]), int(decoded[0]), got[:c["length"]])
        if c["status"] != 0 and c["stores_nothing"]:
            assert np.all(got == FILL), name


def test_all_cases_in_one_call_with_scrambled_destinations(world):
    """the jump table and the 3-, 4- and 5-byte headers are unaligned loads: the frames start at every residue mod 8"""
    eng, by_name, dev, ranges, g = world
    cs = list(zstd_huf_inputs.cases())
    assert {ranges[c["name"]][0] % 8 for c in cs} == set(range(8))
    out, got, status, decoded = _run(world, cs, 47)
    assert {int(v) % 8 for v in out[:, 0]} == set(range(8))


@pytest.mark.parametrize("kind", FAILURES)
def test_one_stream_of_the_four_fails_alone(world, kind):
    """stream s fails on lane s while the other three lanes decode theirs: the frame is BAD_FRAME with nothing decoded and
    nothing stored, whichever lane it was, and the good frames around it in the same call are what they are alone"""
    eng, by_name, dev, ranges, g = world
    good = ("hufend-11-4stream-exact", "hufgeom-regen8", "hufmax-12-4stream")
    cs = []
    for s in range(4):
        c = by_name[_failing(s, kind)]
        assert c["status"] == BAD_FRAME and c["stores_nothing"] and len(c["blocks"]) == 1
        cs += [by_name[good[s % 3]], c, by_name[good[(s + 1) % 3]]]
    out, got, status, decoded = _run(world, cs, 53)
    for i, c in enumerate(cs):
        if c["status"] != 0:
            a, n = int(out[i, 0]), int(out[i, 1])
            assert int(status[i]) == BAD_FRAME and int(decoded[i]) == 0 and np.all(got[a:a + n] == FILL), c["name"]
    for s in range(4):  # and alone in a call
        c = by_name[_failing(s, kind)]
        got, status, decoded = g.run(dev, np.array([ranges[c["name"]]], np.uint64), [(0, _room(c))], _room(c))
        assert int(status[0]) == BAD_FRAME and int(decoded[0]) == 0 and np.all(got == FILL), c["name"]


def _successions(by_name):
    """what one workgroup decodes one after the other, as case names: every workgroup gets one of these"""
    stale4 = "treeless-stale-4streams"
    t12 = zstd_huf_inputs.table12()
    assert t12.log == 12 and len(t12.symbols) == 256 and by_name["hufsyms-fse256-max12"]["status"] == 0
    rows = []
    # 1. a frame that leaves a table of 256 symbols and 12 bits, then a frame whose first block is treeless in four streams
    #    and decodes completely under exactly that table: a decoder that kept the table would call it OK
    rows.append(("hufsyms-fse256-max12", stale4, "hufmax-11-4stream"))
    rows.append(("treeless-after-max12", stale4, "hufmax-12-1stream"))
    # 2. a frame that dies inside huf_read_table (the weights are refused before a table entry is stored: what it leaves is
    #    huf_valid = 0 over whatever table was there, and rewritten weights and ranks), then the same treeless frame, then a
    #    good one
    for bad, good in (("hufbad-incomplete", "hufmax-8-4stream"), ("hufbad-incomplete-fse", "hufmax-1-4stream"), ("hufbad-weight13", "hufmax-2-1stream")):
        rows.append((bad, stale4, good))
    # 3. a frame that fails on stream 3, a good frame of four streams, a frame that fails on stream 1
    rows.append(("hufend-11-4stream-s3-short1", "hufend-11-4stream-exact", "hufend-11-4stream-s1-spare11"))
    # 4. a full literal buffer, then four streams of one symbol, then a fourth stream of none
    rows.append(("hufgeom-regen131072", "hufgeom-regen4", "hufgeom-regen6"))
    # 5. a frame whose last block sets three RLE tables (accuracy log 0: a state is read with read(0)), then each frame that
    #    asks for a table of "the block before"; and the same behind a frame that ends on three described tables
    left = [b for b in by_name["seqtab-rle-left"]["blocks"] if b.get("seqs")][-1]
    assert left["seq_logs"] == (0, 0, 0) and by_name["seqtab-rle-left"]["blocks"][-1] is left and by_name["seqtab-rle-left"]["status"] == 0
    assert [b for b in by_name["seqtab-modes-rle-rle-rle"]["blocks"] if b.get("seqs")][-1]["seq_logs"] == (6, 6, 6)
    for k, s in enumerate(STALE_REPEAT):
        rows.append(("seqtab-rle-left", s, STALE_REPEAT[(k + 1) % 3]))
    rows.append(("seqtab-modes-rle-rle-rle", STALE_REPEAT[0], STALE_REPEAT[1]))
    #    ... and a frame that repeats all three tables and is coded under exactly the RLE tables left: a decoder that kept the
    #    flags of the frame before would call it OK
    assert zstd_huf_inputs._RLE_LEFT == (("rle", 7), ("rle", 5), ("rle", 9)) and by_name["seqtab-stale-rle-repeat"]["status"] == BAD_FRAME
    rows.append(("seqtab-rle-left", "seqtab-stale-rle-repeat", "seqtab-rle-left"))
    for row in rows:
        assert all(n in by_name for n in row), row
    return rows


def test_a_workgroup_decodes_a_second_and_a_third_frame(world):
    """2 * grid + 37 frames for a grid of 4 * CUs workgroups, as tests/test_gpu_zstd_seq.py lays them out: the workgroup of
    frame f also decodes f + grid and, 37 of them, f + 2 * grid, with the State in LDS and the literal buffer that the frame
    before left. Every frame's expectation is its own and depends on no neighbour."""
    eng, by_name, dev, ranges, g = world
    grid = 4 * _cus()
    rows = _successions(by_name)
    n = 2 * grid + 37
    cs = [by_name[rows[(f % grid) % len(rows)][f // grid]] for f in range(n)]
    out, got, status, decoded = _run(world, cs, 59)
    assert sum(int(s) != 0 for s in status) == sum(c["status"] != 0 for c in cs) >= grid // 2


def test_the_cases_through_the_restore(world):
    """blob_decode2(zstd=True) over the OK cases of less than 3 000 bytes and every refused one, each twice, one index entry
    per blob: status 0 and the content, or BAD_DATA. A refused frame of one block is refused before a byte is stored, so its
    entry's part of dst is as it was; the one refused frame of two blocks (treeless-overrun) has decoded its first block,
    and what its entry's part holds is unspecified (include/pbsgpu.h): nothing outside it is written, which the
    neighbours and the guards show."""
    from pbs_plus_amd import RECORD_DTYPE

    eng, by_name, dev_frames, ranges, g = world
    rng = np.random.default_rng(61)
    pick = [c for c in zstd_huf_inputs.cases() if c["status"] != 0 or 0 < c["length"] < 3000]
    refused = sum(c["status"] != 0 for c in pick)
    assert refused >= 60 and len(pick) - refused >= 60
    ents = [pick[i] for i in rng.permutation(len(pick))] + [pick[i] for i in rng.permutation(len(pick))]
    n = len(ents)
    assert 200 <= n <= 600
    sizes = [c["length"] if c["status"] == 0 else int.from_bytes(c["frame"][5:9], "little") for c in ents]
    parts, branges, pos = [], [], 0
    for c in ents:
        gap = int(rng.integers(0, 7))
        blob = _blob(c["frame"], 1)
        parts.append(bytes(gap) + blob)
        branges.append((pos + gap, len(blob)))
        pos += gap + len(blob)
    host = np.frombuffer(b"".join(parts), np.uint8)
    dev = eng.alloc(host.size)
    dev.upload(host)
    idx = np.zeros(n, dtype=RECORD_DTYPE)
    idx["size"] = sizes
    idx["end"] = 1000 + np.cumsum(np.asarray(sizes, dtype=np.uint64))
    idx["digest"] = [np.frombuffer(hashlib.sha256(c["content"]).digest(), np.uint8) for c in ents]
    start, end = 1000, int(idx["end"][-1])
    rg = _RestoreGuarded(eng, end - start)
    try:
        got, status, stats = rg.run(lambda view: eng.blob_decode2(dev, np.array(branges, np.uint64), idx, np.arange(n, dtype=np.uint32),
                                                                  start, end, True, dst=view, zstd=True), end - start)
    finally:
        rg.buf.free()
        dev.free()
    assert status.tolist() == [BAD_DATA if c["status"] != 0 else 0 for c in ents]
    a = 0
    for c, size in zip(ents, sizes):
        if c["status"] == 0:
            assert got[a:a + size].tobytes() == c["content"], c["name"]
            assert hashlib.sha256(got[a:a + size].tobytes()).digest() == c["sha256"]
        elif c["stores_nothing"]:
            assert np.all(got[a:a + size] == FILL), c["name"]
        a += size
    assert stats["bad_data"] == 2 * refused
