"""Every family of synchronous aux calls on ONE engine, in changing orders and at changing sizes: the calls take their
device scratch from the leased slot in call order (Slot::take / Slot::bulk), so a take that returns a buffer sized for
another family, a cursor that is not reset with the lease, or a helper that takes a position its caller still uses would
show as an output that depends on what ran before. Each family runs once per size (the smallest first, so that every
buffer also grows under a family's feet), its outputs are kept and checked against the host where the host can know
them; then all of them run again in two other fixed orders, the sizes stepping down and up again between the repeats,
and every output must be what it was.

Chunks: 64 of 1 to 5 000 bytes (text-like and random, two of them equal), one empty, one of 128 KiB + 1 (two zstd blocks).
The three sizes are prefixes of that list: 6, 25 and all 66 chunks."""
import hashlib
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEVELS = (66, 25, 6)  # chunks at size level 0, 1, 2
DUP = 10              # this chunk has the bytes of chunk 2
FAMILIES = ("crc32_many", "sha256_many", "xxh3_many", "blob_encode", "blob_encode2_zstd", "blob_verify", "blob_decode2",
            "zstd_encode", "zstd_decode", "known", "upload_new2", "upload_new2_zstd")
ORDER1 = tuple(reversed(FAMILIES))
ORDER2 = tuple(FAMILIES[(5 * i + 3) % len(FAMILIES)] for i in range(len(FAMILIES)))  # 5 and 12 are coprime: a permutation


def _chunks():
    rng = np.random.default_rng(77)
    words = [bytes(rng.integers(97, 123, int(rng.integers(2, 9)), dtype=np.uint8)) + b" " for _ in range(40)]

    def text(n):
        out = b"".join(words[int(i)] for i in rng.integers(0, len(words), n // 3 + 2))
        return out[:n]

    sizes = [5000, 1, 63, 4096, 257] + [int(v) for v in rng.integers(1, 5001, 59)]
    small = [text(n) if i % 3 != 1 else bytes(rng.integers(0, 256, n, dtype=np.uint8)) for i, n in enumerate(sizes)]
    small[9] = small[2]  # the same chunk twice: one digest, two records
    big = text((128 << 10) + 1)
    return small[:5] + [b""] + small[5:] + [big]


class _Level:
    """what the calls of one size read: prefix ranges, records, and the blobs and frames made from them"""


def _world():
    from pbs_plus_amd import RECORD_DTYPE, Engine, buzhash

    eng = Engine(buzhash.NewConfig(4096), device=0)
    chunks = _chunks()
    assert len(chunks) == LEVELS[0] and max(len(c) for c in chunks[:-1]) <= 5000
    rng = np.random.default_rng(3)
    parts, ranges, pos = [], [], 0
    for data in chunks:
        gap = int(rng.integers(0, 7))
        parts.append(bytes(gap) + data)
        ranges.append((pos + gap, len(data)))
        pos += gap + len(data)
    host = np.frombuffer(b"".join(parts) + bytes(16), np.uint8)
    dev = eng.alloc(host.size)
    dev.upload(host)
    recs = np.zeros(len(chunks), RECORD_DTYPE)
    recs["size"] = [len(c) for c in chunks]
    recs["end"] = 1000 + np.cumsum(recs["size"].astype(np.uint64))
    recs["digest"] = [np.frombuffer(hashlib.sha256(c).digest(), np.uint8) for c in chunks]
    levels, bufs = [], [dev]
    for n in LEVELS:
        lv = _Level()
        lv.n, lv.chunks, lv.ranges, lv.recs = n, chunks[:n], np.array(ranges[:n], dtype=np.uint64), recs[:n].copy()
        lv.blobs_dev, offs, lens, lv.kinds, _, _ = eng.blob_encode2(dev, lv.ranges, zstd=True)
        lv.blobs = np.stack([offs[:-1], lens.astype(np.uint64)], axis=1)
        lv.frames_dev, st, flen, out = eng.zstd_encode(dev, lv.ranges)
        assert np.all(st == 0)
        lv.frames = np.stack([out[:, 0], flen], axis=1)
        # the restore's index: every chunk, then three entries that name earlier blobs again; the range cuts the first
        # entry in front and the last one behind
        lv.blob_of = np.array(list(range(n)) + [0, 1, 3], dtype=np.uint32)
        lv.idx = np.zeros(n + 3, RECORD_DTYPE)
        lv.idx["size"] = lv.recs["size"][lv.blob_of]
        lv.idx["digest"] = lv.recs["digest"][lv.blob_of]
        lv.idx["end"] = 1000 + np.cumsum(lv.idx["size"].astype(np.uint64))
        lv.stream = b"".join(chunks[int(b)] for b in lv.blob_of)
        bufs += [lv.blobs_dev, lv.frames_dev]
        levels.append(lv)
    assert sorted(set(int(k) for k in levels[0].kinds)) == [0, 1], "both kinds of blob"
    yield eng, dev, levels
    for b in bufs:
        b.free()
    eng.close()


@pytest.fixture(scope="module")
def world():
    yield from _world()


def _take(buf, nbytes=None):
    """a result buffer's bytes, and the buffer freed"""
    try:
        return buf.download(0, buf.nbytes if nbytes is None else nbytes).tobytes()
    finally:
        buf.free()


def _pieces(raw, offs, lens):
    return [raw[int(o):int(o) + int(n)] for o, n in zip(offs, lens)]


def _upload(eng, dev, lv, zstd):
    from pbs_plus_amd import KnownChunks

    with KnownChunks(eng) as known:
        known.add(lv.recs[: lv.n // 3])
        dst, flags, offs, lens, kinds, crcs, stats, enc = known.upload_new2(dev, lv.recs, lv.ranges, insert=True, zstd=zstd)
        raw = _take(dst)
        new = flags == 0
        out = (flags.copy(), offs.copy(), lens.copy(), kinds.copy(), crcs.copy(), stats, enc, dst.used,
               _pieces(raw, offs[new], lens[new]), len(known))
    return out


def _run(name, eng, dev, lv):
    """one call of the family (two for the known set) at one size: everything it returns, in a form == compares"""
    from pbs_plus_amd import KnownChunks

    if name == "crc32_many":
        return eng.crc32_many(dev, lv.ranges)
    if name == "sha256_many":
        return eng.sha256_many(dev, lv.ranges)
    if name == "xxh3_many":
        return eng.xxh3_many(dev, lv.ranges)
    if name == "blob_encode":
        dst, offs, crcs = eng.blob_encode(dev, lv.ranges)
        return _take(dst, int(offs[-1])), offs, crcs.copy()
    if name == "blob_encode2_zstd":
        dst, offs, lens, kinds, crcs, stats = eng.blob_encode2(dev, lv.ranges, zstd=True)
        return _pieces(_take(dst), offs[:-1], lens), offs, lens.copy(), kinds.copy(), crcs.copy(), stats
    if name == "blob_verify":
        status, stats = eng.blob_verify(lv.blobs_dev, lv.blobs, digests=lv.recs["digest"], sizes=lv.recs["size"])
        return status.copy(), stats
    if name == "blob_decode2":
        start, end = 1000 + 1, int(lv.idx["end"][-1]) - 1
        dst, status, stats = eng.blob_decode2(lv.blobs_dev, lv.blobs, lv.idx, blob_of=lv.blob_of, start=start, end=end,
                                              check_digest=True, zstd=True)
        return _take(dst, end - start), status.copy(), stats
    if name == "zstd_encode":
        dst, status, flen, out = eng.zstd_encode(dev, lv.ranges)
        return _pieces(_take(dst), out[:, 0], flen), status.copy(), flen.copy()
    if name == "zstd_decode":
        dst, status, decoded, out = eng.zstd_decode(lv.frames_dev, lv.frames, out=np.stack([lv.recs["end"] - lv.recs["size"] - 1000,
                                                                                           lv.recs["size"].astype(np.uint64)], axis=1))
        return _take(dst, int(lv.recs["end"][-1]) - 1000), status.copy(), decoded.copy()
    if name == "known":
        with KnownChunks(eng) as known:
            known.add(lv.recs[: lv.n // 2])
            first = known.classify(lv.recs, insert=True)
            again = known.classify(lv.recs, insert=False)
            out = (first[0].copy(), first[1], again[0].copy(), again[1], len(known))
        return out
    assert name in ("upload_new2", "upload_new2_zstd")
    return _upload(eng, dev, lv, name.endswith("zstd"))


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    return type(a) is type(b) and a == b


def _check_against_the_host(name, out, lv):
    """what the host knows of a family's outputs; the rest is pinned by the family's own tests"""
    data = b"".join(lv.chunks)
    distinct = lv.n - (lv.n > DUP)  # (chunk DUP repeats chunk 2)
    if name == "crc32_many":
        assert [int(v) for v in out] == [zlib.crc32(c) for c in lv.chunks]
    elif name == "sha256_many":
        assert np.array_equal(out, lv.recs["digest"])
    elif name == "blob_encode":
        assert len(out[0]) == len(data) + 12 * lv.n and [int(v) for v in out[2]] == [zlib.crc32(c) for c in lv.chunks]
    elif name == "blob_encode2_zstd":
        assert np.array_equal(out[3], lv.kinds) and all(zlib.crc32(p[12:]) == int(c) for p, c in zip(out[0], out[4]))
    elif name == "blob_verify":
        assert np.array_equal(out[0], np.where(lv.kinds == 1, 5, 0)) and out[1]["ok"] + out[1]["crc_only"] == lv.n
    elif name == "blob_decode2":
        assert out[0] == lv.stream[1:-1] and np.all(out[1] == 0) and out[2]["ok"] == lv.n + 3
        assert out[2]["out_bytes"] == len(lv.stream) - 2
    elif name == "zstd_decode":
        assert out[0] == data and np.all(out[1] == 0) and np.array_equal(out[2], lv.recs["size"].astype(np.uint64))
    elif name == "known":
        want = np.zeros(lv.n, np.uint8)
        want[: lv.n // 2] = 1
        if lv.n > DUP:
            want[DUP] = 1
        assert np.array_equal(out[0], want) and np.all(out[2] == 1) and out[4] == distinct
    elif name.startswith("upload_new2"):
        flags, offs, lens, kinds, crcs, stats, enc, used, blobs, count = out
        want = np.zeros(lv.n, np.uint8)
        want[: lv.n // 3] = 1
        if lv.n > DUP:
            want[DUP] = 1
        assert np.array_equal(flags, want) and count == distinct
        new = np.flatnonzero(flags == 0)
        assert used == sum(len(lv.chunks[i]) + 12 for i in new) and sum(enc["blobs"]) == len(new)
        assert all(zlib.crc32(b[12:]) == int(crcs[i]) for b, i in zip(blobs, new))
        if name.endswith("zstd"):
            assert np.array_equal(kinds[new], lv.kinds[new])
        else:
            assert np.all(kinds[new] == 0) and all(b[12:] == lv.chunks[i] for b, i in zip(blobs, new))


def test_every_aux_family_gives_the_same_outputs_in_any_order_and_at_any_size_before(world):
    eng, dev, levels = world
    kept = {}
    for level in (2, 1, 0):  # once each, the sizes growing
        for name in FAMILIES:
            kept[name, level] = _run(name, eng, dev, levels[level])
            _check_against_the_host(name, kept[name, level], levels[level])
    runs = 0
    for order in (ORDER1, ORDER2):
        assert sorted(order) == sorted(FAMILIES) and order != FAMILIES
        for level in (1, 2, 1, 0):  # down, and up again
            for name in order:
                assert _same(_run(name, eng, dev, levels[level]), kept[name, level]), (name, level, order.index(name))
                runs += 1
    print("%d calls repeated, all outputs as they were" % runs)
