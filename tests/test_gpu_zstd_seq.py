"""The lane cooperation of the device zstd decoder (k_zstd_frames: zstd.hip, decode_block and decode_frame of zstd_decode.h)
against the frames of tests/zstd_seq_inputs.py, which place every match, literal run and batch edge on purpose, and the
reuse of one workgroup's State and literal buffer for a second and a third frame. Expected contents come from the
byte-at-a-time executor of that module alone; nothing here needs libzstd. The CPU build of the same format core has one
lane and no barrier, so what is tested here is tested nowhere else. The destinations are the guarded ones of
tests/test_gpu_zstd.py; the stale-* frames, which must be refused, went through the sanitizer run of
tests/test_zstd_seq_native.py first, and the truncated fixture through that of tests/test_zstd_core_native.py."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_inputs  # noqa: E402
import zstd_seq_inputs  # noqa: E402
from test_gpu_blob_decode2 import _Guarded as _RestoreGuarded  # noqa: E402
from test_gpu_blob_decode2 import BAD_CRC, BAD_DATA, _blob  # noqa: E402
from test_gpu_zstd import BAD_ROOM, FILL, _Guarded  # noqa: E402

pytestmark = pytest.mark.gpu

FAMILIES = ("seen", "chain", "overlap", "own", "lit", "batch", "blocks", "rep", "stale", "seeded")
STALE = ("stale-treeless", "stale-ll-repeat", "stale-of-repeat", "stale-ml-repeat")
# a recorded truncation of the table-leaving fixture that ends inside the sequences of its one block (they begin at byte
# 4311 of the frame): lane 0 gives up in the middle of a batch and leaves the batch, the states and the tables behind
CUT = (zstd_seq_inputs.TABLE_LEAVING, 8033, zstd_inputs.BAD_FRAME)
OUT_MAX = 64 << 20


def _room(c):
    return c.get("room", c["length"] if c["status"] == 0 else BAD_ROOM)


def _check(c, status, decoded, got):
    assert status == c["status"], (c["name"], status)
    if c["status"] != 0:
        assert decoded == 0, c["name"]
        return
    assert decoded == c["length"], (c["name"], decoded)
    if got.tobytes() != c["content"]:
        want = np.frombuffer(c["content"], np.uint8)
        at = np.flatnonzero(got != want)
        raise AssertionError("%s: %d bytes differ, the first at %s" % (c["name"], at.size, at[:8].tolist()))


def _cus():
    """the device's CU count from the device properties of the runtime instance libpbsgpu.so is linked against: what the
    engine reads (hipDeviceProp_t.multiProcessorCount)"""
    import ctypes as C

    hip = C.CDLL("libamdhip64.so.7", mode=os.RTLD_NOLOAD)
    hip.hipDeviceGetAttribute.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int]
    hip.hipDeviceGetAttribute.restype = C.c_int
    v = C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(v), 63, 0) == 0  # hipDeviceAttributeMultiprocessorCount
    assert 16 <= v.value <= 1024, v.value
    return int(v.value)


@pytest.fixture(scope="module")
def world():
    """(engine, cases by name, device buffer of all frames 0-6 bytes apart, frame range by name, guarded destination):
    the crafted cases, the table-leaving fixture and its recorded truncation"""
    from pbs_plus_amd import Engine, buzhash

    eng = Engine(buzhash.NewConfig(4096), device=0)
    allc = list(zstd_seq_inputs.cases())
    fix = next(c for c in zstd_inputs.cases() if c["name"] == zstd_seq_inputs.TABLE_LEAVING)
    assert CUT in zstd_inputs.CUTS
    allc.append(fix)
    allc.append(dict(name="cut", frame=fix["frame"][:CUT[1]], status=CUT[2], length=0, content=b"", room=fix["length"]))
    rng = np.random.default_rng(29)
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


@pytest.mark.parametrize("fam", FAMILIES)
def test_every_case_alone(world, fam):
    eng, by_name, dev, ranges, g = world
    names = [c["name"] for c in zstd_seq_inputs.cases() if zstd_seq_inputs.family(c["name"]) == fam]
    assert names
    for name in names:  # every case in a call of its own
        c = by_name[name]
        got, status, decoded = g.run(dev, np.array([ranges[name]], np.uint64), [(0, _room(c))], _room(c))
        _check(c, int(status[0]), int(decoded[0]), got[:c["length"]])


def _laid_out(cs, rng):
    """rooms in a seeded permutation with 1-7 untouchable bytes between them: (out per frame, bytes needed)"""
    out, pos = np.zeros((len(cs), 2), dtype=np.uint64), 0
    for i in rng.permutation(len(cs)):
        out[i] = (pos, _room(cs[i]))
        pos += _room(cs[i]) + int(rng.integers(1, 8))
    return out, pos


def _check_all(cs, out, got, status, decoded):
    used = np.zeros(got.size, dtype=bool)
    for i, c in enumerate(cs):
        a, n = int(out[i, 0]), int(out[i, 1])
        used[a:a + n] = True
        _check(c, int(status[i]), int(decoded[i]), got[a:a + c["length"]])
    assert np.all(got[~used] == FILL), "bytes between the rooms"


def test_all_cases_in_one_call_with_scrambled_destinations(world):
    eng, by_name, dev, ranges, g = world
    cs = list(zstd_seq_inputs.cases())
    out, need = _laid_out(cs, np.random.default_rng(31))
    assert {int(v) % 8 for v in out[:, 0]} == set(range(8))
    got, status, decoded = g.run(dev, np.array([ranges[c["name"]] for c in cs], np.uint64), out, need)
    _check_all(cs, out, got, status, decoded)


def _successions(by_name):
    """what one workgroup decodes one after the other, as case names: every workgroup gets one of these"""
    fix, rle_big = zstd_seq_inputs.TABLE_LEAVING, "lit-edge-pairs-rle"
    assert len(by_name[rle_big]["blocks"][-1]["lit"]) > 4096 and by_name[rle_big]["blocks"][-1]["rle"]
    assert by_name["chain-200-ml65-off7"]["blocks"][0]["seqs"][-1][2] == 7 + 3  # its repeat offsets end far from 1, 4, 8
    rows = []
    # 1. a frame that leaves a Huffman table and three described FSE tables, then each frame that asks for a table of
    #    "the block before" in its first block. With a table kept from the frame before, every stale-* frame would
    #    decode: stale-treeless takes one symbol of the shortest code under any table, the others are coded under the
    #    predefined tables, which the crafted frames of the second group leave in the State
    for k, s in enumerate(STALE):
        rows.append((fix, s, STALE[(k + 1) % 4]))
    for k, s in enumerate(STALE[1:]):
        rows.append(("batch-n65-ll3", s, STALE[1 + (k + 1) % 3]))
    # 2. a truncation that fails inside the sequences, then good crafted frames
    rows.append(("cut", "seeded-03", "chain-64-ml64-off63"))
    rows.append(("cut", "batch-n129-ll0", "cut"))
    # 3. a frame that ends with changed repeat offsets, then one that takes the initial ones
    rows.append(("chain-200-ml65-off7", "rep-fresh", "rep-fresh"))
    # 4. a block with a large literal buffer (an RLE fill of one value; Huffman streams), then short RLE literal sections
    rows.append((rle_big, "lit-edge-tail1-rle", "lit-edge-64x16-rle"))
    rows.append((fix, "lit-edge-tail0-rle", "lit-edge-one-long-at31-rle"))
    return rows


def test_a_workgroup_decodes_a_second_and_a_third_frame(world):
    """2 * grid + 37 frames for a grid of 4 * CUs workgroups: the workgroup of frame f also decodes f + grid and, 37 of
    them, f + 2 * grid, with the State in LDS and the literal buffer that the frame before left. The source is a handful
    of frames named many times; only the rooms are disjoint. Every frame's expectation is its own and depends on no
    neighbour, so the test is correct for any grid; it is sharp (every workgroup walks one of the successions) for the
    grid the code uses today, min(nframe, 4 * CUs)."""
    eng, by_name, dev, ranges, g = world
    grid = 4 * _cus()
    rows = _successions(by_name)
    n = 2 * grid + 37
    cs = [by_name[rows[(f % grid) % len(rows)][f // grid]] for f in range(n)]
    out, need = _laid_out(cs, np.random.default_rng(37))
    assert need <= OUT_MAX
    got, status, decoded = g.run(dev, np.array([ranges[c["name"]] for c in cs], np.uint64), out, need)
    _check_all(cs, out, got, status, decoded)
    assert sum(int(s) != 0 for s in status) == sum(c["status"] != 0 for c in cs) > grid // 2


def test_the_restore_hands_a_workgroup_a_second_blob(world):
    """blob_decode2(zstd=True) over 2 * grid + 37 distinct blobs, one index entry each: the decode kernel's workgroups
    stride over the distinct blobs as they do over frames, skipped descriptors (plain blobs, compressed blobs with a bad
    CRC) included. The stale-* blobs follow table-leaving frames on their workgroup and must be BAD_DATA."""
    from pbs_plus_amd import RECORD_DTYPE

    eng, by_name, dev_frames, ranges, g = world
    grid = 4 * _cus()
    rng = np.random.default_rng(41)
    small = [c["name"] for c in zstd_seq_inputs.cases() if c["status"] == 0 and c["length"] < 3000]
    assert len(small) > 40
    n = 2 * grid + 37
    made = {}  # (kind, name) -> blob bytes, entry size, digest, status, expected bytes or None
    plain = rng.integers(0, 256, 333, dtype=np.uint8).tobytes()

    def entry(kind, name):
        if (kind, name) not in made:
            if kind == "plain":
                made[kind, name] = (_blob(plain), len(plain), hashlib.sha256(plain).digest(), 0, plain)
            else:
                c = by_name[name]
                # (a stale-* frame gets an entry of the size it declares in its 4-byte field: it would fit)
                size = c["length"] if c["status"] == 0 else int.from_bytes(c["frame"][5:9], "little")
                crc = 0x1234567 if kind == "badcrc" else None
                st = BAD_CRC if kind == "badcrc" else BAD_DATA if c["status"] != 0 else 0
                made[kind, name] = (_blob(c["frame"], 1, crc), size, hashlib.sha256(c["content"]).digest(), st,
                                    c["content"] if st == 0 else None)
        return made[kind, name]

    ents = []
    for u in range(n):
        w, turn = u % grid, u // grid
        lane = w % 8
        if turn == 0:  # what a workgroup decodes first: every 8th the fixture, else crafted frames, plain and bad-CRC blobs
            ents.append(entry("comp", zstd_seq_inputs.TABLE_LEAVING) if lane == 0 else entry("plain", "") if lane == 5 else
                        entry("badcrc", small[w % len(small)]) if lane == 6 else entry("comp", small[w % len(small)]))
        elif lane in (0, 1, 2, 3):  # ... then: a stale frame after a table-leaving one,
            ents.append(entry("comp", STALE[(w // 8 + lane) % 4]))
        else:  # a good frame after a good one, after a plain blob and after a skipped one
            ents.append(entry("comp", small[(w * 7 + turn) % len(small)]))
    # distinct blobs: every entry has a blob of its own in the source, though many hold the same bytes
    parts, branges, pos = [], [], 0
    for blob, *_ in ents:
        gap = int(rng.integers(0, 7))
        parts.append(bytes(gap) + blob)
        branges.append((pos + gap, len(blob)))
        pos += gap + len(blob)
    host = np.frombuffer(b"".join(parts), np.uint8)
    dev = eng.alloc(host.size)
    dev.upload(host)
    idx = np.zeros(n, dtype=RECORD_DTYPE)
    idx["size"] = [e[1] for e in ents]
    idx["end"] = 1000 + np.cumsum(np.asarray([e[1] for e in ents], dtype=np.uint64))
    idx["digest"] = [np.frombuffer(e[2], np.uint8) for e in ents]
    start, end = 1000, int(idx["end"][-1])
    assert end - start <= OUT_MAX
    rg = _RestoreGuarded(eng, end - start)
    try:
        got, status, stats = rg.run(lambda view: eng.blob_decode2(dev, np.array(branges, np.uint64), idx, np.arange(n, dtype=np.uint32),
                                                                  start, end, True, dst=view, zstd=True), end - start)
    finally:
        rg.buf.free()
        dev.free()
    assert status.tolist() == [e[3] for e in ents]
    a = 0
    for blob, size, dig, st, data in ents:
        if st == 0:
            assert hashlib.sha256(got[a:a + size].tobytes()).digest() == dig and got[a:a + size].tobytes() == data
        elif st == BAD_CRC:
            assert np.all(got[a:a + size] == FILL), "a blob with a bad CRC is not decoded"
        a += size
    assert stats["bad_data"] == sum(e[3] == BAD_DATA for e in ents) >= grid // 4
    assert stats["bad_crc"] == sum(e[3] == BAD_CRC for e in ents) >= grid // 8
