"""Restore with the keyed digest check (pbsgpu_blob_decode4_device): pbsgpu_blob_decode3_device plus the id key. One index
over blobs of all four kinds, the encrypted entries carrying SHA-256(content || id_key) and the others SHA-256(content); a blob
named by three entries, entries clipped by both ends of the range. Built like tests/test_gpu_blob_decode3.py (the same helper
modules, the same layout of dst: pre-filled with a pattern and larger than the range). And one round trip of an encrypted
session: keyed batch digests, the known-chunk set, encrypted blobs written on the device, restored and checked."""
import hashlib
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aes_inputs as ai  # noqa: E402
import zstd_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0xA5
TAIL = 256  # bytes of dst behind the range
OK, BAD_MAGIC, BAD_CRC, BAD_SIZE, BAD_DIGEST, CRC_ONLY, BAD_DATA, BAD_TAG = range(8)
PLAIN, ZSTD, ENC, ENC_ZSTD = range(4)
ID_RIGHT = bytes((13 * i + 1) & 0xFF for i in range(32))
ID_WRONG = bytes((13 * i + 2) & 0xFF for i in range(32))


@pytest.fixture(scope="module")
def eng():
    from pbs_plus_amd import Engine, buzhash

    e = Engine(buzhash.NewConfig(4096), device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def keys(eng):
    from pbs_plus_amd import AesKey, IdKey

    k = {"right": AesKey(eng, ai.key_of(5)), "wrong": AesKey(eng, ai.key_of(6)), "id": IdKey(eng, ID_RIGHT),
         "id_wrong": IdKey(eng, ID_WRONG)}
    yield k
    for v in k.values():
        v.close()


def encrypt_many(eng, key, plains, ivs):
    """[(ciphertext, tag)] by the device's batch call"""
    buf = np.frombuffer(b"".join(plains) + bytes(16), np.uint8)
    lens = np.array([len(p) for p in plains], dtype=np.uint64)
    segs = np.stack([np.cumsum(lens) - lens, lens], axis=1)
    src = eng.alloc(buf.size)
    try:
        src.upload(buf)
        dst, status, tags, out = eng.aes_gcm_many(key, src, segs, ivs, encrypt=True)
        got = dst.download(0, max(int(lens.sum()), 1))
        dst.free()
    finally:
        src.free()
    assert not status.any()
    return [(got[int(o):int(o) + int(n)].tobytes(), tags[i].tobytes()) for i, (o, n) in enumerate(segs)]


def frame_blob(kind, body, iv=b"", tag=b""):
    from pbs_plus_amd import blob_magic

    return blob_magic(kind) + zlib.crc32(body).to_bytes(4, "little") + iv + tag + body


@pytest.fixture(scope="module")
def world(eng, keys):
    """the blobs by name, each blob's content and kind, the entries in order (e1 is named by three), and the index digests:
    keyed for the encrypted kinds, plain for the others"""
    z = {c["name"]: c for c in zstd_inputs.cases() if c["status"] == 0}
    contents = {
        "p0": (PLAIN, ai.pattern(3000, 1)), "p1": (PLAIN, ai.pattern(40001, 2)),
        "z0": (ZSTD, z["lowsym-3000"]), "e0": (ENC, ai.pattern(3001, 3)), "e1": (ENC, ai.pattern(5000, 4)),
        "e2": (ENC, ai.pattern(70001, 5)), "e3": (ENC, ai.pattern(23, 6)),
        "ez0": (ENC_ZSTD, z["text-60000-level1"]), "ez1": (ENC_ZSTD, z["many-90000"]), "ez2": (ENC_ZSTD, z["hand-rle-block"]),
    }
    enc = [n for n, (k, _) in contents.items() if k in (ENC, ENC_ZSTD)]
    ivs = [ai.pattern(16, 700 + i) for i in range(len(enc))]
    plains = [contents[n][1] if contents[n][0] == ENC else contents[n][1]["frame"] for n in enc]
    sealed = dict(zip(enc, zip(ivs, encrypt_many(eng, keys["right"], plains, ivs))))
    blobs, content, digest = {}, {}, {}
    for n, (kind, c) in contents.items():
        if kind == PLAIN:
            blobs[n], content[n] = frame_blob(kind, c), c
        elif kind == ZSTD:
            blobs[n], content[n] = frame_blob(kind, c["frame"]), c["content"]
        else:
            iv, (ct, tag) = sealed[n]
            blobs[n] = frame_blob(kind, ct, iv, tag)
            content[n] = c if kind == ENC else c["content"]
        digest[n] = hashlib.sha256(bytes(content[n]) + (ID_RIGHT if kind in (ENC, ENC_ZSTD) else b"")).digest()
    order = ["e0", "p0", "e1", "z0", "ez0", "e1", "e2", "p1", "ez1", "e3", "e1", "ez2", "ez0"]
    return dict(blobs=blobs, content=content, kinds={n: k for n, (k, _) in contents.items()}, order=order, digest=digest)


def restore(eng, w, key, id_key, blobs=None, digests=None, clip=(1000, 777), digest=True, call="decode4", aes=None):
    """-> status, the range's bytes as restored, stats, the stream, (start, end), the index"""
    from pbs_plus_amd import RECORD_DTYPE

    order = w["order"]
    blobs = dict(w["blobs"], **(blobs or {}))
    names = sorted(set(order))
    buf, ranges = bytearray(), []
    for n in names:
        buf += bytes(3)  # blobs at odd offsets
        ranges.append((len(buf), len(blobs[n])))
        buf += blobs[n]
    host = np.frombuffer(bytes(buf) + bytes(16), np.uint8)
    idx = np.zeros(len(order), dtype=RECORD_DTYPE)
    idx["size"] = [len(w["content"][n]) for n in order]
    idx["end"] = np.cumsum(idx["size"].astype(np.uint64))
    for i, n in enumerate(order):
        idx["digest"][i] = np.frombuffer((digests or {}).get(n, w["digest"][n]), np.uint8)
    stream = b"".join(bytes(w["content"][n]) for n in order)
    start, end = clip[0], int(idx["end"][-1]) - clip[1]
    blob_of = np.array([names.index(n) for n in order], dtype=np.uint32)
    src, dst = eng.alloc(host.size), eng.alloc(end - start + TAIL)
    try:
        src.upload(host)
        dst.upload(np.full(end - start + TAIL, FILL, np.uint8))
        args = (src, np.array(ranges, dtype=np.uint64), idx, blob_of, start, end, digest)
        try:
            if call == "decode4":
                _, status, stats = eng.blob_decode4(*args, dst=dst, key=key, id_key=id_key, aes=aes)
            else:
                _, status, stats = eng.blob_decode3(*args, dst=dst, key=key, aes=aes)
        except Exception:
            assert np.all(dst.download(0, end - start + TAIL) == FILL), "a refused call wrote to dst"
            raise
        got = dst.download(0, end - start + TAIL)
    finally:
        src.free()
        dst.free()
    assert np.all(got[end - start:] == FILL), "a byte behind the range was written"
    return dict(status=status, got=got[:end - start].tobytes(), stats=stats, stream=stream, span=(start, end), idx=idx)


def part(r, i):
    """entry i's part of the range, as (restored bytes, the stream's bytes)"""
    start, end = r["span"]
    lo = max(int(r["idx"]["end"][i]) - int(r["idx"]["size"][i]), start)
    hi = min(int(r["idx"]["end"][i]), end)
    return r["got"][lo - start:hi - start], r["stream"][lo:hi]


def encrypted(world, n):
    return world["kinds"][n] in (ENC, ENC_ZSTD)


def test_the_right_id_key_every_entry_ok_and_the_bytes_equal(eng, keys, world):
    r = restore(eng, world, keys["right"], keys["id"])
    assert not r["status"].any(), r["status"]
    start, end = r["span"]
    assert r["got"] == r["stream"][start:end]
    assert r["stats"]["ok"] == len(world["order"]) and r["stats"]["out_bytes"] == end - start
    # sha_bytes: each distinct blob's content once: the plain kinds as in blob_decode3, the encrypted ones keyed
    distinct = set(world["order"])
    assert r["stats"]["sha_bytes"] == sum(len(world["content"][n]) for n in distinct)
    d3 = restore(eng, world, keys["right"], None, call="decode3")
    assert d3["stats"]["sha_bytes"] == sum(len(world["content"][n]) for n in distinct if not encrypted(world, n))


def test_the_wrong_id_key_is_a_bad_digest_on_exactly_the_encrypted_entries(eng, keys, world):
    r = restore(eng, world, keys["right"], keys["id_wrong"])
    for i, n in enumerate(world["order"]):
        assert r["status"][i] == (BAD_DIGEST if encrypted(world, n) else OK), n
        got, stream = part(r, i)
        assert got == stream, n  # the bytes already stored stay: the caller reads the status
    nenc = sum(encrypted(world, n) for n in world["order"])
    assert r["stats"]["bad_digest"] == nenc and r["stats"]["ok"] == len(world["order"]) - nenc
    # one wrong digest in the index: that entry alone, of the three that name e1
    r = restore(eng, world, keys["right"], keys["id"], digests={"e2": hashlib.sha256(world["content"]["e2"]).digest()})
    for i, n in enumerate(world["order"]):
        assert r["status"][i] == (BAD_DIGEST if n == "e2" else OK), n


def test_without_an_id_key_it_is_decode3(eng, keys, world):
    for digest in (True, False):
        a = restore(eng, world, keys["right"], None, digest=digest)
        b = restore(eng, world, keys["right"], None, digest=digest, call="decode3")
        assert np.array_equal(a["status"], b["status"]) and a["got"] == b["got"] and a["stats"] == b["stats"]
    # an id key without F_DIGEST, or without F_AES, is ignored
    a = restore(eng, world, keys["right"], keys["id_wrong"], digest=False)
    b = restore(eng, world, keys["right"], None, digest=False, call="decode3")
    assert np.array_equal(a["status"], b["status"]) and a["got"] == b["got"] and a["stats"] == b["stats"]
    a = restore(eng, world, None, keys["id_wrong"], aes=False)
    b = restore(eng, world, None, None, aes=False, call="decode3")
    assert np.array_equal(a["status"], b["status"]) and a["got"] == b["got"] and a["stats"] == b["stats"]


def test_a_bad_tag_wins_over_the_digest(eng, keys, world):
    b = world["blobs"]
    flip = lambda x, at: x[:at] + bytes([x[at] ^ 1]) + x[at + 1:]  # noqa: E731
    resealed = lambda x: x[:8] + zlib.crc32(x[44:]).to_bytes(4, "little") + x[12:]  # noqa: E731
    bad = {"e1": resealed(flip(b["e1"], 30)), "ez1": resealed(flip(b["ez1"], 13))}
    r = restore(eng, world, keys["right"], keys["id_wrong"], blobs=bad)
    for i, n in enumerate(world["order"]):
        want = BAD_TAG if n in bad else BAD_DIGEST if encrypted(world, n) else OK
        assert r["status"][i] == want, (n, r["status"][i])
    # the wrong AES key: a bad tag on every encrypted entry, whatever the id key
    r = restore(eng, world, keys["wrong"], keys["id"])
    for i, n in enumerate(world["order"]):
        assert r["status"][i] == (BAD_TAG if encrypted(world, n) else OK), n
    assert r["stats"]["sha_bytes"] == sum(len(world["content"][n]) for n in set(world["order"]) if not encrypted(world, n))


def test_an_id_key_of_another_engine_is_refused_with_dst_untouched(eng, keys, world):
    from pbs_plus_amd import Engine, IdKey, PbsGpuError, _lib, buzhash

    with Engine(buzhash.NewConfig(4096), device=0) as other, IdKey(other, ID_RIGHT) as foreign:
        with pytest.raises(PbsGpuError) as ei:
            restore(eng, world, keys["right"], foreign)
        assert ei.value.status == _lib.E_INVALID


def test_round_trip_of_an_encrypted_session(eng, keys):
    """chunk_and_digest(id_key=) -> KnownChunks.classify -> blob_encode3 of the new chunks -> blob_decode4 with F_AES | F_DIGEST"""
    from oracle import oracle as O
    from pbs_plus_amd import KnownChunks, blob_index, chunk_ranges

    half = O.fill(1_500_000, 31, 3)
    data = np.concatenate([half, half[:700_000], O.fill(300_001, 32, 0)])  # repeated content: some chunks are duplicates
    src = eng.alloc(data.size + 16)
    try:
        src.upload(data)
        recs = eng.chunk_and_digest(src, nbytes=data.size, id_key=keys["id"])
        with KnownChunks(eng) as known:
            flags, _ = known.classify(recs)
            assert 0 < int((flags == 0).sum()) < len(recs)  # the duplicates of the repeated content are known by then
            new = chunk_ranges(recs, known=flags)
            buf, offsets, lens, kinds, crcs, stats, ivs = eng.blob_encode3(src, new, key=keys["right"], nbytes=data.size)
            try:
                assert set(int(k) for k in kinds) <= {ENC, ENC_ZSTD}
                blobs = np.stack([offsets[:-1], lens.astype(np.uint64)], axis=1)
                blob_of = blob_index(recs["digest"][flags == 0], recs)
                dst, status, dstats = eng.blob_decode4(buf, blobs, recs, blob_of, key=keys["right"], id_key=keys["id"])
                try:
                    assert not status.any(), status
                    assert np.array_equal(dst.download(0, data.size), data)
                    assert dstats["sha_bytes"] == int(new[:, 1].sum())
                finally:
                    dst.free()
                # the same blobs under another id key: every entry's digest is wrong
                dst, status, _ = eng.blob_decode4(buf, blobs, recs, blob_of, key=keys["right"], id_key=keys["id_wrong"])
                dst.free()
                assert np.all(status == BAD_DIGEST)
            finally:
                buf.free()
            # a second keyed pass over the same data: every chunk is known; a pass without the key: none is
            again, _ = known.classify(eng.chunk_and_digest(src, nbytes=data.size, id_key=keys["id"]), insert=False)
            assert np.all(again == 1)
            plain = eng.chunk_and_digest(src, nbytes=data.size)
            assert np.array_equal(plain["end"], recs["end"])
            first = np.unique(plain["digest"], axis=0, return_index=True)[1]
            none, _ = known.classify(plain[np.sort(first)], insert=False)
            assert not none.any()
    finally:
        src.free()
