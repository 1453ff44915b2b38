"""Restore a stream on the GPU from its index and data blobs (pbsgpu_blob_decode_device, Engine.blob_decode). The model is
Python: zlib.crc32, hashlib.sha256 and slicing; the statuses are checked against Engine.blob_verify on the same blob with
the entry's size and digest. Every call writes into a destination that is pre-filled with a guard pattern and has 64 guard
bytes in front of it and behind it: what must stay untouched is seen to be untouched."""
import hashlib
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PIECE = 1 << 16  # blob.hip kPiece
ROW = 1024       # blob.hip kRow
GUARD = 64
FILL = 0xA5
MAGIC_NAMES = ("uncompressed", "zstd compressed", "encrypted", "zstd compressed encrypted")


def _magic(kind):
    return hashlib.sha256(f"Proxmox Backup {MAGIC_NAMES[kind]} blob v1.0".encode()).digest()[:8]


MAGIC0 = _magic(0)


def _engine(avg=4096):
    from pbs_plus_amd import Engine, buzhash

    return Engine(buzhash.NewConfig(avg), device=0)


def _dev(eng, host):
    buf = eng.alloc(max(host.size, 1))
    if host.size:
        buf.upload(host)
    return buf


def _blob(data: bytes, kind=0) -> bytes:
    """a blob of `kind` around data; the encrypted kinds carry IV + tag (32 bytes) between the CRC and the data"""
    return _magic(kind) + zlib.crc32(data).to_bytes(4, "little") + (bytes(32) if kind >= 2 else b"") + data


def _index(sizes, digests, base=0):
    from pbs_plus_amd import RECORD_DTYPE

    idx = np.zeros(len(sizes), dtype=RECORD_DTYPE)
    idx["size"] = sizes
    idx["end"] = base + np.cumsum(np.asarray(sizes, dtype=np.uint64))
    idx["digest"] = digests
    idx["segment"] = 0xdead  # ignored
    return idx


def _sha(data) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(bytes(data)).digest(), np.uint8)


class _View:
    """a window of a device allocation: what blob_decode needs of a destination"""

    def __init__(self, ptr, nbytes):
        self.ptr, self.nbytes = ptr, nbytes


class _Guarded:
    """one allocation that serves as the guarded destination of many calls"""

    def __init__(self, eng, cap):
        self.eng, self.buf = eng, eng.alloc(cap + 2 * GUARD)

    def run(self, data, blobs, idx, blob_of, start, end, check_digest=True, nbytes=None, cap=None):
        need = end - start
        total = need + 2 * GUARD
        assert total <= self.buf.nbytes
        self.buf.upload(np.full(total, FILL, np.uint8))
        # the capacity reaches over the guard behind the range: room that must not be used
        view = _View(self.buf.ptr + GUARD, need + GUARD if cap is None else cap)
        try:
            _, status, stats = self.eng.blob_decode(data, blobs, idx, blob_of, start, end, check_digest, dst=view, nbytes=nbytes)
        finally:
            got = self.buf.download(0, total)
            assert np.all(got[:GUARD] == FILL), "guard in front of dst"
            assert np.all(got[GUARD + need:] == FILL), "guard behind dst"
        return got[GUARD:GUARD + need], status, stats

    def free(self):
        self.buf.free()


def _model(buf, blobs, idx, blob_of, start, end):
    """(dst as it must be after the call on a destination full of FILL, bytes written)"""
    out = np.full(end - start, FILL, np.uint8)
    written = 0
    for i in range(idx.size):
        o, n = (int(v) for v in blobs[int(blob_of[i])])
        size, e1 = int(idx["size"][i]), int(idx["end"][i])
        s0 = e1 - size
        lo, hi = max(s0, start), min(e1, end)
        if hi <= lo:
            continue
        if n >= 12 and buf[o:o + 8].tobytes() == MAGIC0 and n - 12 == size:
            out[lo - start:hi - start] = buf[o + 12 + lo - s0:o + 12 + hi - s0]
            written += hi - lo
    return out, written


def _verify_says(eng, dbuf, nbytes, blobs, idx, blob_of, check_digest=True):
    """the specification of the statuses: blob_verify on the entry's blob with the entry's size and digest"""
    segs = [tuple(int(v) for v in blobs[int(b)]) for b in blob_of]
    status, _ = eng.blob_verify(dbuf, segs, digests=idx["digest"] if check_digest else None, sizes=idx["size"], nbytes=nbytes)
    return status


def _same(got, want):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (int(bad[0]), int(bad.size), got[bad[:8]].tolist(), want[bad[:8]].tolist())


# ---- 1. lengths and alignments -------------------------------------------------------------------------------------------
LENGTHS = list(range(131)) + [1023, 1024, 1025, 4095, 4096, 4097, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 3]
# n = 1..3 mod 1024 above a row: the four inverted bytes reach into row 1 of the piece
LENGTHS += [1026, 1027, 1028, PIECE + 2, PIECE + 3, 2 * PIECE + 1, 2 * PIECE + 2]


def _aligned_corpus(make):
    """every length at every residue mod 16 of the blob offset: (buffer, blobs, data per blob)"""
    parts, blobs, datas, pos = [], [], [], 0
    for r in range(16):
        for n in LENGTHS:
            pad = (r - pos) % 16
            parts.append(bytes(pad))
            pos += pad
            data = make(n)
            b = _blob(data)
            blobs.append((pos, len(b)))
            datas.append(data)
            parts.append(b)
            pos += len(b)
    return np.frombuffer(b"".join(parts), np.uint8).copy(), blobs, datas


@pytest.mark.parametrize("pattern", ["random", "zeros", "ones"])
def test_every_length_at_every_source_and_destination_alignment(pattern):
    rng = np.random.default_rng(41)
    make = {"random": lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes(), "zeros": lambda n: bytes(n),
            "ones": lambda n: b"\xff" * n}[pattern]
    buf, blobs, datas = _aligned_corpus(make)
    assert all(o % 16 == i // len(LENGTHS) for i, (o, _) in enumerate(blobs))
    order = np.random.default_rng(42).permutation(len(blobs)).astype(np.uint32)
    base = 1000003
    idx = _index([len(datas[b]) for b in order], [_sha(datas[b]) for b in order], base)
    # every source residue mod 16 meets every destination residue mod 4, on chunks of more than one 16-byte unit
    pairs = {(blobs[b][0] % 16, (int(idx["end"][i]) - int(idx["size"][i]) - base) % 4)
             for i, b in enumerate(order) if idx["size"][i] >= 32}
    assert len(pairs) == 64
    eng = _engine()
    d = _dev(eng, buf)
    end = int(idx["end"][-1])
    g = _Guarded(eng, end - base)
    got, status, st = g.run(d, blobs, idx, order, base, end, nbytes=buf.size)
    want = np.frombuffer(b"".join(datas[b] for b in order), np.uint8)
    _same(got, want)
    assert np.all(status == 0) and st["ok"] == idx.size
    assert st["out_bytes"] == want.size == st["crc_bytes"] == st["sha_bytes"]
    assert st["blob_bytes"] == want.size + 12 * len(blobs)
    assert np.array_equal(status, _verify_says(eng, d, buf.size, blobs, idx, order))
    g.free()
    d.free()
    eng.close()


# ---- 2. range clipping ----------------------------------------------------------------------------------------------------
def test_ranges_that_begin_and_end_anywhere():
    rng = np.random.default_rng(43)
    sizes = [PIECE + 5] + [int(v) for v in rng.integers(1, 131, 12)] + [2 * PIECE + 3] + [int(v) for v in rng.integers(1, 131, 10)]
    sizes += [0] + [int(v) for v in rng.integers(1, 131, 12)] + [3 * PIECE - 7, 1, 130]
    assert len(sizes) == 40
    datas = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes]
    place = rng.permutation(len(sizes))  # the blobs lie in another order than the entries, 0-6 bytes apart
    parts, blobs, pos = [], [None] * len(sizes), 0
    for e in place:
        gap = int(rng.integers(0, 7))
        parts.append(bytes(gap))
        pos += gap
        b = _blob(datas[e])
        blobs[e] = (pos, len(b))
        parts.append(b)
        pos += len(b)
    buf = np.frombuffer(b"".join(parts), np.uint8).copy()
    S = 777
    idx = _index(sizes, [_sha(x) for x in datas], S)
    E = int(idx["end"][-1])
    stream = np.frombuffer(b"".join(datas), np.uint8)
    starts = [int(e) - int(s) for e, s in zip(idx["end"], idx["size"])]
    multi = [i for i, n in enumerate(sizes) if n > PIECE]
    pts = set()
    for s0 in starts + [E]:
        pts.update((s0 - 1, s0, s0 + 1))
    for i in (multi[0], multi[-1]):
        pts.update(starts[i] + 5000 + k for k in range(16))
    big = starts[multi[1]]
    pts.update((big + ROW - 1, big + ROW + 1, big + PIECE - 1, big + PIECE + 1, big + 3 + ROW, big + 3 + PIECE))
    pts = sorted(p for p in pts if S <= p <= E)
    calls = {(S, E)}
    for k, p in enumerate(pts):
        calls.add((p, E))
        calls.add((S, p))
        calls.add((p, pts[min(k + 9, len(pts) - 1)]))
        if k % 8 == 0:
            calls.add((p, p))  # the empty range
    inside = starts[multi[1]] + 12345
    calls.update({(inside, inside + 1), (inside, inside + 17), (starts[3], starts[3] + 1), (S, S), (E, E)})
    calls = sorted(calls)
    assert 300 <= len(calls) <= 900
    eng = _engine()
    d = _dev(eng, buf)
    g = _Guarded(eng, E - S)
    ident = np.arange(len(sizes), dtype=np.uint32)
    for k, (a, b) in enumerate(calls):
        got, status, st = g.run(d, blobs, idx, None if k % 2 else ident, a, b, check_digest=(k % 3 == 0), nbytes=buf.size)
        _same(got, stream[a - S:b - S])
        assert np.all(status == 0), (a, b)
        assert st["out_bytes"] == b - a, (a, b)
        assert st["ok"] == idx.size and st["crc_bytes"] == stream.size
        assert st["sha_bytes"] == (stream.size if k % 3 == 0 else 0)
    g.free()
    d.free()
    eng.close()


# ---- 3. fan-out -----------------------------------------------------------------------------------------------------------
def test_one_blob_behind_many_entries():
    rng = np.random.default_rng(44)
    sizes = {"big": 2 * PIECE + 3, "x3": 3, "m": 700, "s1": 100, "s2": 5000, "s3": 70000}
    names = list(sizes)
    datas = {k: rng.integers(0, 256, n, dtype=np.uint8).tobytes() for k, n in sizes.items()}
    parts, blobs, pos = [b"\x01\x02\x03"], [], 3
    for k in names:
        b = _blob(datas[k])
        blobs.append((pos, len(b)))
        parts.append(b)
        pos += len(b) + 1
        parts.append(b"\x00")
    junk = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()  # a corrupt blob that nothing references
    parts.append(junk)
    junk_blob = (pos, len(junk))
    buf = np.frombuffer(b"".join(parts), np.uint8).copy()
    # big x5 (first and last entry, two adjacent), x3 x64 (runs of 10, 20, 34), m x2, the others once
    order = ["big"] + ["x3"] * 10 + ["s1", "big", "m"] + ["x3"] * 20 + ["s2", "big", "big", "m"] + ["x3"] * 34 + ["s3", "big"]
    refs = {k: order.count(k) for k in names}
    assert sorted(refs.values()) == [1, 1, 1, 2, 5, 64]
    blob_of = np.array([names.index(k) for k in order], dtype=np.uint32)
    S = 5
    idx = _index([sizes[k] for k in order], [_sha(datas[k]) for k in order], S)
    E = int(idx["end"][-1])
    stream = np.frombuffer(b"".join(datas[k] for k in order), np.uint8)
    eng = _engine()
    d = _dev(eng, buf)
    g = _Guarded(eng, E - S)
    data_bytes = sum(sizes.values())
    for a, b in ((S, E), (S + 777, E - 12345), (S + PIECE + 1, E - 2 * PIECE - 2)):
        for bl in (blobs, blobs + [junk_blob]):
            got, status, st = g.run(d, bl, idx, blob_of, a, b, nbytes=buf.size)
            _same(got, stream[a - S:b - S])
            assert np.all(status == 0) and st["ok"] == idx.size
            assert st["crc_bytes"] == st["sha_bytes"] == data_bytes
            assert st["blob_bytes"] == data_bytes + 12 * len(names)
            assert st["out_bytes"] == b - a
    g.free()
    d.free()
    eng.close()


# ---- 4. statuses and what they leave in dst -------------------------------------------------------------------------------
def test_statuses_and_the_destination_of_bad_entries():
    from pbs_plus_amd import _lib

    rng = np.random.default_rng(45)

    def rnd(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def flip(b, at, bit=0x10):
        a = bytearray(b)
        a[at] ^= bit
        return bytes(a)

    OKs, MAGIC, CRC, SIZE, DIGEST, CRCONLY = range(6)
    # (blob bytes, the entry's size, the entry's digest, the status expected)
    cases = []

    def add(blob, size, digest, want, times=1):
        cases.extend([(blob, size, digest, want)] * times)

    def good(n):
        x = rnd(n)
        add(_blob(x), n, _sha(x), OKs)

    good(100)
    x = rnd(300)
    add(b"\x13" * 8 + _blob(x)[8:], 300, _sha(x), MAGIC)                       # an unknown magic
    good(PIECE + 9)
    x = rnd(50)
    for cut in (0, 7, 8, 11):                                                  # shorter than a header
        add(_blob(x)[:cut], 50, _sha(x), MAGIC)
    good(1)
    x = rnd(5000)
    add(flip(_blob(x), 12 + 4321), 5000, _sha(x), CRC)                         # a data byte
    x = rnd(77)
    add(flip(_blob(x), 9), 77, _sha(x), CRC)                                   # the stored CRC
    good(0)
    x = rnd(2000)
    add(_blob(x), 1999, _sha(x), SIZE)
    add(_blob(x), 2001, _sha(x), SIZE)
    x = rnd(640)
    add(_blob(x), 640, _sha(x) ^ np.uint8(1), DIGEST)                          # an altered entry digest
    good(4097)
    x = rnd(60)
    add(_blob(x, 1), 100, _sha(x), CRCONLY)                                    # compressed, good CRC
    add(_blob(x, 2), 60, _sha(x), CRCONLY)                                     # encrypted (44-byte header), good CRC
    add(_blob(rnd(PIECE - 10), 3), PIECE - 10, _sha(b""), CRCONLY)             # ... one piece, where 12 bytes of header mean two
    add(flip(_blob(x, 2), 44 + 7), 60, _sha(x), CRC)                           # encrypted, bad CRC
    x = rnd(900)
    add(flip(_blob(x), 12 + 5), 901, _sha(x), CRC)                             # a bad CRC that hides a size mismatch
    good(33)
    x = rnd(1500)
    add(flip(_blob(x), 12 + 1499), 1500, _sha(x), CRC, times=3)                # a bad blob behind three entries
    good(130)
    parts, blobs, blob_of, seen, pos = [], [], [], {}, 1
    parts.append(b"\x00")
    for blob, _, _, _ in cases:
        if id(blob) not in seen:
            seen[id(blob)] = len(blobs)
            blobs.append((pos, len(blob)))
            parts.append(blob + b"\xee\xee")
            pos += len(blob) + 2
        blob_of.append(seen[id(blob)])
    assert len(blobs) == len(cases) - 2
    buf = np.frombuffer(b"".join(parts), np.uint8).copy()
    blob_of = np.array(blob_of, dtype=np.uint32)
    S = 64
    idx = _index([c[1] for c in cases], [c[2] for c in cases], S)
    E = int(idx["end"][-1])
    want_status = np.array([c[3] for c in cases], dtype=np.uint8)
    eng = _engine()
    d = _dev(eng, buf)
    g = _Guarded(eng, E - S)
    for a, b in ((S, E), (S + 50, E - 70)):
        for chk in (True, False):
            want_dst, written = _model(buf, blobs, idx, blob_of, a, b)
            got, status, st = g.run(d, blobs, idx, blob_of, a, b, check_digest=chk, nbytes=buf.size)
            says = _verify_says(eng, d, buf.size, blobs, idx, blob_of, chk)
            assert np.array_equal(status, says), (status.tolist(), says.tolist())
            hand = want_status.copy()
            if not chk:
                hand[hand == DIGEST] = OKs
            assert np.array_equal(status, hand), (status.tolist(), hand.tolist())
            _same(got, want_dst)
            assert st["out_bytes"] == written
            for code, name in enumerate(_lib.BLOB_STATUS_NAMES):
                assert st[name] == int((hand == code).sum()), name
            unc = sum(n - 12 for (o, n) in blobs if n >= 12 and buf[o:o + 8].tobytes() == MAGIC0)
            assert st["sha_bytes"] == (unc if chk else 0)
            assert st["blob_bytes"] == sum(n for _, n in blobs)
    assert set(range(6)) <= set(want_status.tolist())
    # the bad entries left the guard pattern, or the blob's bytes as found
    full, _ = _model(buf, blobs, idx, blob_of, S, E)
    for i, c in enumerate(cases):
        part = full[int(idx["end"][i]) - c[1] - S:int(idx["end"][i]) - S]
        if c[3] in (MAGIC, SIZE, CRCONLY) or (c[3] == CRC and len(c[0]) - 12 != c[1]):
            assert np.all(part == FILL), i
        elif c[1]:
            assert part.tobytes() == c[0][12:], i
    g.free()
    d.free()
    eng.close()


# ---- 5. capacity ----------------------------------------------------------------------------------------------------------
def test_a_destination_one_byte_short_is_left_alone():
    from pbs_plus_amd import PbsGpuError, _lib

    rng = np.random.default_rng(46)
    datas = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (10, 5000, PIECE + 1)]
    buf = np.frombuffer(b"".join(_blob(x) for x in datas), np.uint8).copy()
    offs = np.cumsum([0] + [len(x) + 12 for x in datas])
    blobs = [(int(offs[i]), len(x) + 12) for i, x in enumerate(datas)]
    idx = _index([len(x) for x in datas], [_sha(x) for x in datas])
    E = int(idx["end"][-1])
    eng = _engine()
    d = _dev(eng, buf)
    g = _Guarded(eng, E)
    for a, b in ((0, E), (3, E - 3)):
        with pytest.raises(PbsGpuError) as err:
            g.run(d, blobs, idx, None, a, b, nbytes=buf.size, cap=b - a - 1)
        assert err.value.status == _lib.E_CAPACITY
        assert np.all(g.buf.download() == FILL)
    got, status, _ = g.run(d, blobs, idx, None, 0, E, nbytes=buf.size, cap=E)  # exactly enough
    assert got.tobytes() == b"".join(datas) and np.all(status == 0)
    g.free()
    d.free()
    eng.close()


# ---- 6. end to end --------------------------------------------------------------------------------------------------------
def _write_then_read(eng, host, min_dups):
    """the writer loop, then its inverse: (device source, restored device buffer, index, blob table, blob_of)"""
    from pbs_plus_amd import blob_index, chunk_ranges
    from pbs_plus_amd.engine import didx_decode

    src = _dev(eng, host)
    recs = eng.chunk_and_digest(src, nbytes=host.size)
    dup, _ = eng.dedup(recs)
    first = recs[dup == 0]
    enc, offs, _ = eng.blob_encode(src, chunk_ranges(recs, None, dup), nbytes=host.size)
    idx, _, _ = didx_decode(eng.didx_encode(recs))
    blob_of = blob_index(first["digest"], idx)
    # entries whose blob an earlier entry references: a condition on the corpus
    assert idx.size - np.unique(blob_of).size >= min_dups
    blobs = np.stack([offs[:-1], offs[1:] - offs[:-1]], axis=1)
    out = eng.alloc(host.size + 2 * GUARD)
    out.upload(np.full(GUARD, FILL, np.uint8))
    out.upload(np.full(GUARD, FILL, np.uint8), GUARD + host.size)
    _, status, st = eng.blob_decode(enc, blobs, idx, blob_of, dst=_View(out.ptr + GUARD, host.size + GUARD))
    assert np.all(status == 0) and st["ok"] == idx.size
    assert st["out_bytes"] == host.size and st["crc_bytes"] == st["sha_bytes"] == int(first["size"].sum())
    back = out.download()
    assert np.all(back[:GUARD] == FILL) and np.all(back[GUARD + host.size:] == FILL)
    assert np.array_equal(back[GUARD:GUARD + host.size], host)
    src.free()
    return enc, out, idx, blobs, blob_of


def test_write_a_stream_then_restore_it_whole_in_ranges_and_hash_its_files():
    rng = np.random.default_rng(47)
    size = 64 << 20
    host = rng.integers(0, 256, size, dtype=np.uint8)
    block = host[5 << 20:6 << 20].copy()
    host[(20 << 20) + 17:(21 << 20) + 17] = block
    host[(47 << 20) + 4001:(48 << 20) + 4001] = block
    eng = _engine(4096)
    enc, out, idx, blobs, blob_of = _write_then_read(eng, host, 100)
    ends = idx["end"].astype(np.int64)
    g = _Guarded(eng, 4 << 20)
    for _ in range(200):
        a = int(rng.integers(0, size))
        b = min(size, a + int(rng.integers(0, 4 << 20)))
        lo = int(np.searchsorted(ends, a, side="right"))
        hi = min(int(np.searchsorted(ends, b, side="left")) + 1, idx.size)
        got, status, st = g.run(enc, blobs, idx[lo:hi], blob_of[lo:hi], a, b)
        assert np.all(status == 0) and st["out_bytes"] == b - a
        assert np.array_equal(got, host[a:b]), (a, b)
    files = [(int(o), int(rng.integers(0, min(2 << 20, size - int(o)) + 1))) for o in rng.integers(0, size, 50)]
    digs = eng.sha256_many(out, [(o + GUARD, n) for o, n in files])
    for (o, n), dg in zip(files, digs):
        assert dg.tobytes() == hashlib.sha256(host[o:o + n].tobytes()).digest()
    g.free()
    enc.free()
    out.free()
    eng.close()


def test_write_then_restore_256_mib_of_4_mib_chunks():
    rng = np.random.default_rng(48)
    base = rng.integers(0, 256, 64 << 20, dtype=np.uint8)
    host = np.concatenate([base, (base ^ 0x5A)[:32 << 20], base, base ^ 0xC3, (base ^ 0x3C)[:32 << 20]])
    assert host.size == 256 << 20
    eng = _engine(4 << 20)
    enc, out, _, _, _ = _write_then_read(eng, host, 1)
    enc.free()
    out.free()
    eng.close()


# ---- 7. beside a running ring ---------------------------------------------------------------------------------------------
def test_decode_beside_a_running_ring(O):
    """A page ring ingests two synthetic streams; between its pumps, streams are restored from blobs on the same engine:
    exact, and the ring's records still equal the oracle's."""
    import time

    from pbs_plus_amd import PageRing

    eng = _engine(64 << 10)
    page = 262144
    ring = PageRing(eng, arena_bytes=48 * (page + 256), page_bytes=page, max_streams=2, sha_cus=16, round_pages=8)
    jobs = [(11, 0, (40 << 20) + 5), (12, 3, (24 << 20) + 77)]
    rng = np.random.default_rng(49)
    datas = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(1, 1 << 20, 24)]
    buf = np.frombuffer(b"".join(_blob(x) for x in datas), np.uint8).copy()
    offs = np.cumsum([0] + [len(x) + 12 for x in datas])
    blobs = [(int(offs[i]), len(x) + 12) for i, x in enumerate(datas)]
    order = rng.integers(0, len(datas), 40).astype(np.uint32)
    idx = _index([len(datas[b]) for b in order], [_sha(datas[b]) for b in order], 99)
    stream = np.frombuffer(b"".join(datas[b] for b in order), np.uint8)
    S, E = 99, int(idx["end"][-1])
    d = _dev(eng, buf)
    g = _Guarded(eng, E - S)
    res = [[] for _ in jobs]
    active, todo, runs = {}, list(range(len(jobs))), 0
    t0 = time.perf_counter()
    while todo or active:
        while todo:
            sid = ring.open()
            active[sid] = [todo.pop(0), None, False]
            active[sid][1] = int(jobs[active[sid][0]][2])
        for sid, a in active.items():
            j, left, fin = a
            if not fin:
                want = min(left, 16 * page)
                got = ring.fill(sid, jobs[j][0], jobs[j][1], want, final=(want == left))
                a[1] -= got
                a[2] = a[1] == 0 and got == want
        ring.pump()
        if runs < 6 and ring.stats()["service_launches"] >= 1:
            a, b = (S, E) if runs % 2 == 0 else (S + 1000 * runs + 1, E - 4097 * runs)
            out, status, st = g.run(d, blobs, idx, order, a, b, nbytes=buf.size)
            assert np.all(status == 0) and st["out_bytes"] == b - a
            assert np.array_equal(out, stream[a - S:b - S])
            runs += 1
        for sid in list(active):
            recs, fin = ring.poll(sid)
            if recs.size:
                res[active[sid][0]].append(recs.copy())
            if fin:
                ring.close_stream(sid)
                del active[sid]
        assert time.perf_counter() - t0 < 300
    assert runs >= 1
    ring.quiesce()
    for (seed, kind, n), r in zip(jobs, res):
        got = np.concatenate(r)
        w = O.chunk_and_digest(O.new_config(64 << 10), O.fill(n, seed, kind), [(0, n)])
        assert got.size == w.size and np.array_equal(got["end"], w["end"]) and np.array_equal(got["digest"], w["digest"])
    ring.close()
    g.free()
    d.free()
    eng.close()
