"""Data blobs on the GPU (pbsgpu_crc32_* / pbsgpu_blob_*, Engine.crc32_many / blob_encode / blob_verify): the CRC-32 against
zlib.crc32, the uncompressed blob against a byte-exact Python model, the encode of a classified corpus's new chunks, the
verifier's statuses, and all of it beside a running page ring."""
import hashlib
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from seam_inputs import BLOB_EDGE_LENS as EDGE_LENS  # noqa: E402

pytestmark = pytest.mark.gpu

PIECE = 1 << 16  # blob.hip kPiece
MAGIC_NAMES = ("uncompressed", "zstd compressed", "encrypted", "zstd compressed encrypted")


def _magic(kind):
    return hashlib.sha256(f"Proxmox Backup {MAGIC_NAMES[kind]} blob v1.0".encode()).digest()[:8]


def _engine(avg=4096):
    from pbs_plus_amd import Engine, buzhash

    return Engine(buzhash.NewConfig(avg), device=0)


def _dev(eng, host):
    buf = eng.alloc(max(host.size, 1))
    if host.size:
        buf.upload(host)
    return buf


def _model_blob(chunk: bytes, kind=0) -> bytes:
    return _magic(kind) + zlib.crc32(chunk).to_bytes(4, "little") + chunk


def _check_crc(eng, host, dbuf, segs):
    want = np.array([zlib.crc32(host[o:o + n].tobytes()) for o, n in segs], dtype=np.uint32)
    got_d = eng.crc32_many(dbuf, segs, nbytes=host.size)
    got_h = eng.crc32_many(host, segs)
    bad = np.nonzero(got_d != want)[0]
    assert bad.size == 0, [(segs[i], hex(int(got_d[i])), hex(int(want[i]))) for i in bad[:8]]
    assert np.array_equal(got_h, want)


def test_crc32_lengths_offsets_and_patterns():
    """Every length 0-130, the row and piece edges and EDGE_LENS, at every residue mod 16 of the offset; overlapping
    ranges."""
    eng = _engine()
    rng = np.random.default_rng(1)
    host = rng.integers(0, 256, 3 * PIECE + 4096, dtype=np.uint8)
    d = _dev(eng, host)
    lens = list(range(131)) + [1023, 1024, 1025, 4095, 4096, 4097, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 3]
    lens += [n for n in EDGE_LENS if n not in lens]
    segs = [(off, n) for n in lens for off in range(16) if off + n <= host.size]
    _check_crc(eng, host, d, segs)
    # overlapping ranges and the whole buffer
    segs = [(int(rng.integers(0, 2 * PIECE)), int(rng.integers(0, PIECE + 5000))) for _ in range(300)] + [(0, host.size)]
    _check_crc(eng, host, d, segs)
    d.free()
    for fill in (0x00, 0xFF):
        h = np.full(2 * PIECE + 17, fill, dtype=np.uint8)
        dd = _dev(eng, h)
        _check_crc(eng, h, dd, [(0, h.size), (3, 4), (1, PIECE), (5, 2 * PIECE + 12), (0, 0)])
        dd.free()
    eng.close()


def test_crc32_a_16_mib_chunk_and_the_check_value():
    eng = _engine()
    rng = np.random.default_rng(2)
    host = np.concatenate([np.frombuffer(b"123456789", np.uint8), rng.integers(0, 256, (16 << 20) + 64, dtype=np.uint8)])
    d = _dev(eng, host)
    got = eng.crc32_many(d, [(0, 9), (9, 16 << 20), (10, (16 << 20) - 1), (0, 0)], nbytes=host.size)
    assert int(got[0]) == 0xCBF43926
    assert int(got[1]) == zlib.crc32(host[9:9 + (16 << 20)].tobytes())
    assert int(got[2]) == zlib.crc32(host[10:9 + (16 << 20)].tobytes())
    assert int(got[3]) == 0
    d.free()
    eng.close()


def test_crc32_100k_small_segments_in_one_batch():
    eng = _engine()
    rng = np.random.default_rng(3)
    host = rng.integers(0, 256, 8 << 20, dtype=np.uint8)
    d = _dev(eng, host)
    lens = rng.integers(0, 200, 100_000)
    offs = rng.integers(0, host.size - 200, 100_000)
    segs = np.stack([offs, lens], axis=1).astype(np.uint64)
    long = segs[::1000].shape[0]  # a few multi-piece ones among them
    segs[::1000, 0] = rng.integers(0, host.size - 3 * PIECE, long)
    segs[::1000, 1] = rng.integers(PIECE - 3, 3 * PIECE, long)
    _check_crc(eng, host, d, [(int(o), int(n)) for o, n in segs])
    d.free()
    eng.close()


def _parse(buf: np.ndarray, offs, crcs, chunks, src: np.ndarray):
    """every blob of an encode against the Python model"""
    for i, (o, n) in enumerate(chunks):
        b = buf[int(offs[i]):int(offs[i + 1])].tobytes()
        want = _model_blob(src[o:o + n].tobytes())
        assert b == want, (i, o, n)
        assert int(crcs[i]) == zlib.crc32(src[o:o + n].tobytes())


def test_encode_is_byte_exact_and_respects_the_capacity():
    import ctypes as C

    from pbs_plus_amd import _lib

    eng = _engine()
    rng = np.random.default_rng(4)
    host = rng.integers(0, 256, 4 * PIECE, dtype=np.uint8)
    src = _dev(eng, host)
    chunks = [(0, 0), (1, 1), (2, 3), (5, 17), (7, 1024), (13, 1025), (0, PIECE + 1), (3, 2 * PIECE - 5), (11, 100), (0, 0)]
    chunks += [(int(rng.integers(0, PIECE)), int(rng.integers(0, 3000))) for _ in range(200)]
    # the edge rows' store: every length of EDGE_LENS at every source residue mod 16; the running blob offsets give every
    # one of them every destination residue mod 4
    edge0 = len(chunks)
    chunks += [(off, n) for off in range(16) for n in EDGE_LENS]
    dst, offs, crcs = eng.blob_encode(src, chunks, nbytes=host.size)
    assert int(offs[-1]) == sum(12 + n for _, n in chunks) == dst.nbytes
    assert {(n, (int(offs[i]) + 12) % 4) for i, (_, n) in enumerate(chunks) if i >= edge0} == \
        {(n, r) for n in EDGE_LENS for r in range(4)}
    _parse(dst.download(), offs, crcs, chunks, host)
    dst.free()
    # guard bytes past dst_cap stay untouched; a capacity one byte short is E_CAPACITY with the needed size
    L = _lib.lib()
    segs = np.array(chunks, dtype=np.uint64)
    total = int(offs[-1])
    guard = eng.alloc(total + 4096)
    guard.upload(np.full(total + 4096, 0xA5, np.uint8))
    n = C.c_uint64()
    st = L.pbsgpu_blob_encode_device(eng._h, src.ptr, host.size, segs.ctypes.data, len(chunks), guard.ptr, total - 1,
                                     C.byref(n), None, None)
    assert st == _lib.E_CAPACITY and n.value == total
    assert np.all(guard.download() == 0xA5)  # nothing written
    st = L.pbsgpu_blob_encode_device(eng._h, src.ptr, host.size, segs.ctypes.data, len(chunks), guard.ptr, total,
                                     C.byref(n), None, None)
    assert st == 0 and n.value == total
    out = guard.download()
    assert np.all(out[total:] == 0xA5)
    _parse(out, offs, crcs, chunks, host)
    guard.free()
    src.free()
    eng.close()


@pytest.mark.parametrize("avg,size", [(4 << 20, 1 << 30), (4096, 256 << 20)])
def test_end_to_end_classify_then_encode_the_new_chunks(avg, size):
    """chunk_and_digest -> classify against a set holding half of the digests -> encode the new chunks: every blob parses
    and its CRC, size and SHA-256 match zlib, hashlib and the record; the verifier says OK for every one of them."""
    from pbs_plus_amd import KnownChunks, chunk_ranges

    eng = _engine(avg)
    src = eng.alloc(size)
    eng.fill(src.ptr, size, seed=77, kind=3)
    segs = [(0, size // 2 + 13), (size // 2 + 13, size // 2 - 13)]
    recs = eng.chunk_and_digest(src, segs, nbytes=size)
    assert recs.size > 100
    k = KnownChunks(eng)
    k.add(recs[::2])
    known, st = k.classify(recs, insert=True)
    ranges = chunk_ranges(recs, segs, known)
    new = recs[known == 0]
    assert ranges.shape[0] == new.size == st["nunique"] > 0
    assert np.array_equal(ranges[:, 1], new["size"].astype(np.uint64))
    dst, offs, crcs = eng.blob_encode(src, ranges, nbytes=size)
    host = src.download()
    out = dst.download()
    magic = _magic(0)
    for i, (o, n) in enumerate(ranges):
        o, n = int(o), int(n)
        b = out[int(offs[i]):int(offs[i + 1])]
        assert b[:8].tobytes() == magic
        data = b[12:].tobytes()
        assert len(data) == n == int(new["size"][i])
        assert data == host[o:o + n].tobytes()
        c = zlib.crc32(data)
        assert int.from_bytes(b[8:12].tobytes(), "little") == c == int(crcs[i])
        assert hashlib.sha256(data).digest() == new["digest"][i].tobytes()
    blobs = np.stack([offs[:-1], offs[1:] - offs[:-1]], axis=1)
    status, vst = eng.blob_verify(dst, blobs, digests=new["digest"], sizes=new["size"])
    assert np.all(status == 0) and vst["ok"] == new.size
    assert vst["blob_bytes"] == int(offs[-1]) and vst["sha_bytes"] == vst["crc_bytes"] == int(ranges[:, 1].sum())
    dst.free()
    src.free()
    k.close()
    eng.close()


def _corpus(rng):
    """blobs of every kind in one host buffer: (buffer, [(offset, length)], digests, sizes)"""
    parts, blobs, digs, sizes, pos = [], [], [], [], 3
    parts.append(rng.integers(0, 256, 3, dtype=np.uint8).tobytes())
    for i in range(300):
        n = int(rng.integers(0, 20000)) if i % 7 else int(rng.integers(PIECE, 3 * PIECE))
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        kind = 0 if i % 5 else int(rng.integers(1, 4))
        if kind >= 2:  # IV + tag, then the ciphertext stand-in; the CRC covers what follows the 44-byte header
            b = _magic(kind) + zlib.crc32(data).to_bytes(4, "little") + bytes(32) + data
        else:
            b = _model_blob(data, kind)
        parts.append(b)
        blobs.append((pos, len(b)))
        digs.append(np.frombuffer(hashlib.sha256(data).digest(), np.uint8))
        sizes.append(n)
        pos += len(b)
        gap = int(rng.integers(0, 5))
        parts.append(bytes(gap))
        pos += gap
    buf = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    return buf, blobs, np.array(digs), np.array(sizes, dtype=np.uint32)


def _kinds(buf, blobs):
    mags = [_magic(k) for k in range(4)]
    return [mags.index(buf[o:o + 8].tobytes()) for o, _ in blobs]


def test_verify_statuses_device_and_host():
    eng = _engine()
    rng = np.random.default_rng(5)
    buf, blobs, digs, sizes = _corpus(rng)
    kinds = _kinds(buf, blobs)
    d = _dev(eng, buf)
    want = np.array([0 if k == 0 else 5 for k in kinds], dtype=np.uint8)
    for data in (d, buf):
        status, st = eng.blob_verify(data, blobs, digs, sizes, nbytes=buf.size)
        assert np.array_equal(status, want)
        assert st["ok"] == int((want == 0).sum()) and st["crc_only"] == int((want == 5).sum())
        assert st["blob_bytes"] == sum(n for _, n in blobs)
        assert st["crc_bytes"] == sum(n - (44 if k >= 2 else 12) for (_, n), k in zip(blobs, kinds))
        assert st["sha_bytes"] == sum(int(s) for s, k in zip(sizes, kinds) if k == 0)
    # no expectations: the CRC alone
    status, _ = eng.blob_verify(d, blobs, nbytes=buf.size)
    assert np.array_equal(status, want)
    # one fault per blob, chosen per blob
    bad = buf.copy()
    want_bad = want.copy()
    digs2, sizes2 = digs.copy(), sizes.copy()
    blobs2 = list(blobs)
    for i, ((o, n), k) in enumerate(zip(blobs, kinds)):
        hdr = 44 if k >= 2 else 12
        which = i % 7  # (6: left intact)
        if which == 0:  # a data byte flipped
            if n > hdr:
                bad[o + hdr + int(rng.integers(0, n - hdr))] ^= 0x40
                want_bad[i] = 2
        elif which == 1:  # a magic byte
            bad[o + int(rng.integers(0, 8))] ^= 1
            want_bad[i] = 1
        elif which == 2:  # the stored CRC
            bad[o + 8] ^= 0x80
            want_bad[i] = 2
        elif which == 3 and k == 0:  # a wrong size expectation
            sizes2[i] += 1
            want_bad[i] = 3
        elif which == 4 and k == 0:  # a wrong digest expectation
            digs2[i, 5] ^= 1
            want_bad[i] = 4
        elif which == 5:  # truncated below its header
            blobs2[i] = (o, min(n, hdr - 1 - int(rng.integers(0, hdr - 1))))
            want_bad[i] = 1
    db = _dev(eng, bad)
    for data in (db, bad):
        status, st = eng.blob_verify(data, blobs2, digs2, sizes2, nbytes=bad.size)
        mism = np.nonzero(status != want_bad)[0]
        assert mism.size == 0, [(int(i), kinds[i], int(status[i]), int(want_bad[i])) for i in mism[:10]]
        names = ("ok", "bad_magic", "bad_crc", "bad_size", "bad_digest", "crc_only")
        for code, name in enumerate(names):
            assert st[name] == int((want_bad == code).sum()), name
        assert sum(st[n] for n in names) == len(blobs2)
    assert set(range(6)) <= set(int(x) for x in want_bad)  # every status was provoked
    db.free()
    d.free()
    eng.close()


def test_encode_and_verify_beside_a_running_ring(O):
    """A page ring ingests two synthetic streams; between its pumps, encode and verify run on their own buffers on the
    same engine: both exact, and the ring's records still equal the oracle's."""
    import time

    from pbs_plus_amd import PageRing

    eng = _engine(64 << 10)
    page = 262144
    ring = PageRing(eng, arena_bytes=48 * (page + 256), page_bytes=page, max_streams=2, sha_cus=16, round_pages=8)
    jobs = [(11, 0, (96 << 20) + 5), (12, 3, (64 << 20) + 77)]
    rng = np.random.default_rng(6)
    host = rng.integers(0, 256, 24 << 20, dtype=np.uint8)
    src = _dev(eng, host)
    chunks = [(int(rng.integers(0, 1 << 20)), int(rng.integers(1, 3 << 20))) for _ in range(64)]
    want_blobs = b"".join(_model_blob(host[o:o + n].tobytes()) for o, n in chunks)
    digs = np.array([np.frombuffer(hashlib.sha256(host[o:o + n].tobytes()).digest(), np.uint8) for o, n in chunks])
    sizes = np.array([n for _, n in chunks], dtype=np.uint32)
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
            dst, offs, crcs = eng.blob_encode(src, chunks, nbytes=host.size)
            assert dst.download().tobytes() == want_blobs
            blobs = np.stack([offs[:-1], offs[1:] - offs[:-1]], axis=1)
            status, _ = eng.blob_verify(dst, blobs, digs, sizes)
            assert np.all(status == 0)
            dst.free()
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
    src.free()
    eng.close()
