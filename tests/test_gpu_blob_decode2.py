"""Restore with the zstd-compressed blobs decoded on the device (pbsgpu_blob_decode2_device, Engine.blob_decode2) against a
Python model: zlib.crc32, hashlib.sha256, slicing, and the golden frames of tests/golden/zstd_v1*.npz as the compressed
chunks (nothing here needs libzstd). Every call writes into a destination pre-filled with a guard pattern, with 64 guard
bytes in front and behind and a capacity that reaches over the rear guard."""
import hashlib
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
MAGIC_NAMES = ("uncompressed", "zstd compressed", "encrypted", "zstd compressed encrypted")
OK, BAD_MAGIC, BAD_CRC, BAD_SIZE, BAD_DIGEST, CRC_ONLY, BAD_DATA = range(7)
NAMES = ("ok", "bad_magic", "bad_crc", "bad_size", "bad_digest", "crc_only", "bad_data")
DATA, KEEP, ANY = 0, 1, 2  # what an entry's part of dst holds afterwards: its bytes, what was there, unspecified


def _magic(kind):
    return hashlib.sha256(f"Proxmox Backup {MAGIC_NAMES[kind]} blob v1.0".encode()).digest()[:8]


def _blob(data: bytes, kind=0, crc=None) -> bytes:
    crc = zlib.crc32(data) if crc is None else crc
    return _magic(kind) + crc.to_bytes(4, "little") + (bytes(32) if kind >= 2 else b"") + data


class _View:
    def __init__(self, ptr, nbytes):
        self.ptr, self.nbytes = ptr, nbytes


class _Guarded:
    """one allocation that serves as the guarded destination of many calls"""

    def __init__(self, eng, cap):
        self.eng, self.buf = eng, eng.alloc(cap + 2 * GUARD)

    def run(self, fn, need, cap=None):
        total = need + 2 * GUARD
        assert total <= self.buf.nbytes
        self.buf.upload(np.full(total, FILL, np.uint8))
        view = _View(self.buf.ptr + GUARD, need + GUARD if cap is None else cap)
        try:
            _, status, stats = fn(view)
        finally:
            got = self.buf.download(0, total)
            assert np.all(got[:GUARD] == FILL), "guard in front of dst"
            assert np.all(got[GUARD + need:] == FILL), "guard behind dst"
        return got[GUARD:GUARD + need], status, stats


@pytest.fixture(scope="module")
def world():
    """a mixed index of 40 entries over 38 blobs: (engine, device blobs, blob ranges, idx, blob_of, per entry: status with
    F_ZSTD, status without, the entry's true bytes, what its part of dst holds), and the byte counts the stats must show"""
    from pbs_plus_amd import RECORD_DTYPE, Engine, buzhash

    eng = Engine(buzhash.NewConfig(4096), device=0)
    cases = {c["name"]: c for c in zstd_inputs.cases()}
    rng = np.random.default_rng(21)
    blobs, ents = [], []  # blob bytes; (blob, size, digest, status2, status1, bytes or None, dst rule)

    def sha(b):
        return hashlib.sha256(b).digest()

    def plain(n):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        blobs.append(_blob(data))
        ents.append((len(blobs) - 1, n, sha(data), OK, OK, data, DATA))

    def comp(name, **kw):
        c = cases[name]
        blobs.append(_blob(c["frame"], 1, kw.get("crc")))
        b = len(blobs) - 1
        size = c["length"] + kw.get("dsize", 0)
        dig = sha(c["content"]) if not kw.get("bad_digest") else sha(b"x")
        st = kw.get("status", OK)
        ents.append((b, size, dig, st, kw.get("status1", CRC_ONLY), c["content"], kw.get("rule", DATA)))
        return b

    zin = zout = 0
    for name in ("text-131073", "text-3", "lowsym-3000"):
        comp(name)
    for n in (1, 700, 4096):
        plain(n)
    for name in ("text-60000-level1", "hand-raw-block", "many-30000-checksum-level19", "byte-300000", "text-1"):
        comp(name)
    for kind in (2, 3):  # encrypted kinds: CRC only, untouched
        data = rng.integers(0, 256, 500, dtype=np.uint8).tobytes()
        blobs.append(_blob(data, kind))
        ents.append((len(blobs) - 1, 500, sha(data), CRC_ONLY, CRC_ONLY, None, KEEP))
    shared = comp("text-40000-checksum")  # one compressed blob behind three entries, apart from one another
    plain(33)
    comp("period3-50000")
    ents.append((shared,) + ents[[e[0] for e in ents].index(shared)][1:])
    comp("hand-literal-forms")
    comp("text-50000-nosize")
    comp("text-2", crc=12345, status=BAD_CRC, status1=BAD_CRC, rule=KEEP)       # a compressed blob with a bad CRC
    comp("text-131072", dsize=+1, status=BAD_SIZE, rule=ANY)                     # decodes, to one byte less than the entry
    comp("text-131071", dsize=-1, status=BAD_SIZE, rule=ANY)                     # declares more than the entry has room for
    comp("bad-two-frames", dsize=78, status=BAD_DATA, rule=ANY)                  # unsupported
    mname, at, xor = zstd_inputs.MUTATIONS[0][:3]                                 # malformed (a recorded mutation)
    blobs.append(_blob(zstd_inputs.mutated(cases[mname]["frame"], at, xor), 1))
    ents.append((len(blobs) - 1, cases[mname]["length"], bytes(32), BAD_DATA, CRC_ONLY, None, ANY))
    comp("many-90000", bad_digest=True, status=BAD_DIGEST)                       # the bytes are written, the digest is not theirs
    ents.append((shared,) + ents[[e[0] for e in ents].index(shared)][1:])
    for n in (5, 1300):
        plain(n)
    for name in ("hand-nseq-3-bytes", "mixed-300000-streamed-checksum", "text-0", "hand-rle-block", "hand-empty-last-block",
                 "hand-fcs8", "rand-140000", "text-400000-streamed-level7", "byte-200-nosize", "period70000-300000"):
        comp(name)
    plain(64)
    comp("mixed-1048576-level3")
    assert len(ents) == 40 and len(blobs) == 38
    seen = set()
    for b, size, dig, st2, st1, data, rule in ents:  # the decoder's byte counts: once per distinct compressed blob with a good CRC
        if blobs[b][:8] == _magic(1) and st2 != BAD_CRC and b not in seen:
            seen.add(b)
            zin += len(blobs[b]) - 12
            if st2 in (OK, BAD_DIGEST) or (st2 == BAD_SIZE and size > len(data)):
                zout += len(data)
    place = rng.permutation(len(blobs))
    parts, ranges, pos = [], [None] * len(blobs), 0
    for b in place:
        gap = int(rng.integers(0, 7))
        parts.append(bytes(gap) + blobs[b])
        ranges[b] = (pos + gap, len(blobs[b]))
        pos += gap + len(blobs[b])
    host = np.frombuffer(b"".join(parts), np.uint8)
    dev = eng.alloc(host.size)
    dev.upload(host)
    idx = np.zeros(len(ents), dtype=RECORD_DTYPE)
    idx["size"] = [e[1] for e in ents]
    idx["end"] = 1000 + np.cumsum(np.asarray([e[1] for e in ents], dtype=np.uint64))
    idx["digest"] = [np.frombuffer(e[2], np.uint8) for e in ents]
    blob_of = np.array([e[0] for e in ents], dtype=np.uint32)
    g = _Guarded(eng, int(idx["end"][-1]) - 1000)
    yield eng, dev, np.array(ranges, dtype=np.uint64), idx, blob_of, ents, g, (zin, zout)
    g.buf.free()
    dev.free()
    eng.close()


def _expect(idx, ents, start, end, zstd):
    """(bytes of the range with FILL where nothing may be written, mask of the bytes that are specified, bytes written)"""
    want = np.full(end - start, FILL, np.uint8)
    known = np.ones(end - start, dtype=bool)
    written = 0
    for i, (b, size, dig, st2, st1, data, rule) in enumerate(ents):
        s0 = int(idx["end"][i]) - size
        lo, hi = max(s0, start), min(s0 + size, end)
        if hi <= lo:
            continue
        compressed = st1 in (CRC_ONLY, BAD_CRC) and rule != KEEP or st2 == BAD_DATA
        if compressed and not zstd:
            continue  # untouched
        if rule == DATA:
            want[lo - start:hi - start] = np.frombuffer(data, np.uint8)[lo - s0:hi - s0]
            written += hi - lo
        elif rule == ANY:
            known[lo - start:hi - start] = False
    return want, known, written


def _run(world, start, end, zstd=True, digest=True):
    eng, dev, ranges, idx, blob_of, ents, g, _ = world
    got, status, stats = g.run(lambda view: eng.blob_decode2(dev, ranges, idx, blob_of, start, end, digest, dst=view, zstd=zstd),
                               end - start)
    want, known, written = _expect(idx, ents, start, end, zstd)
    assert np.array_equal(got[known], want[known]), np.flatnonzero(got[known] != want[known])[:8]
    return got, status, stats, written


def test_without_the_flag_it_is_blob_decode(world):
    eng, dev, ranges, idx, blob_of, ents, g, _ = world
    S, E = 1000, int(idx["end"][-1])
    for digest in (True, False):
        for a, b in ((S, E), (S + 7, E - 9), (S + 131073 + 2, S + 131073 + 3), (E, E)):
            old, st_old, stats_old = g.run(lambda v: eng.blob_decode(dev, ranges, idx, blob_of, a, b, digest, dst=v), b - a)
            new, st_new, stats_new = g.run(lambda v: eng.blob_decode2(dev, ranges, idx, blob_of, a, b, digest, dst=v, zstd=False), b - a)
            assert np.array_equal(old, new) and np.array_equal(st_old, st_new)
            assert all(stats_new[k] == v for k, v in stats_old.items())
            assert stats_new["bad_data"] == stats_new["zstd_in_bytes"] == stats_new["zstd_out_bytes"] == 0
    assert st_new.tolist() == [e[4] for e in ents]


def test_the_whole_range_with_every_kind_of_entry(world):
    eng, dev, ranges, idx, blob_of, ents, g, (zin, zout) = world
    S, E = 1000, int(idx["end"][-1])
    for digest in (True, False):
        got, status, stats, written = _run(world, S, E, digest=digest)
        want = [OK if (st == BAD_DIGEST and not digest) else st for st in (e[3] for e in ents)]
        assert status.tolist() == want
        assert [stats[n] for n in NAMES] == [want.count(k) for k in range(7)]
        assert stats["zstd_in_bytes"] == zin and stats["zstd_out_bytes"] == zout
        assert stats["out_bytes"] == written
        assert stats["blob_bytes"] == int(ranges[:, 1].sum())
    assert {OK, BAD_CRC, BAD_SIZE, BAD_DIGEST, CRC_ONLY, BAD_DATA} <= set(status.tolist()) | {BAD_DIGEST}


def test_ranges_that_clip_compressed_entries(world):
    eng, dev, ranges, idx, blob_of, ents, g, _ = world
    S, E = 1000, int(idx["end"][-1])
    ends = [int(v) for v in idx["end"]]
    full = [e[3] for e in ents]
    first = S + 131073            # entry 0 is compressed and 131 073 bytes long
    last0 = ends[-2]              # the last entry is compressed, 1 MiB
    calls = [(S + 5, E - 11),                         # clips a compressed entry at each end
             (S + 131072, last0 + 1),                 # one byte of each
             (S + 1000, S + 1001), (S + 70000, S + 131000),   # inside one compressed entry
             (last0 + 300000, last0 + 300007),
             (ends[13] - 40000 + 17, ends[15] - 3),   # begins inside the shared blob's first entry
             (first, first), (E, E), (S, S)]          # empty
    for a, b in calls:
        got, status, stats, written = _run(world, a, b)
        assert status.tolist() == full, (a, b)        # entries outside the range are checked all the same
        assert stats["out_bytes"] == written, (a, b)


def test_a_destination_that_is_too_small_stays_untouched(world):
    from pbs_plus_amd import PbsGpuError, _lib

    eng, dev, ranges, idx, blob_of, ents, g, _ = world
    S, E = 1000, int(idx["end"][-1])
    with pytest.raises(PbsGpuError) as e:
        g.run(lambda v: eng.blob_decode2(dev, ranges, idx, blob_of, S, E, True, dst=v), E - S - 1, cap=E - S - 1)
    assert e.value.status == _lib.E_CAPACITY
    assert np.all(g.buf.download(0, E - S + GUARD) == FILL)
