"""Restore with encrypted blobs decrypted on the device (pbsgpu_blob_decode3_device): one index over blobs of all four
kinds, a blob named by three entries, entries clipped by both ends of the range, and the frames of the encrypted-compressed
kind taken from tests/golden/zstd_*. The ciphertexts are made by Engine.aes_gcm_many(encrypt=True), which
tests/test_gpu_aes.py holds against libcrypto's recorded answers. dst is pre-filled with a pattern and larger than the range,
so a byte stored outside an entry's part is seen."""
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aes_inputs as ai  # noqa: E402
import zstd_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0xA5
TAIL = 256  # bytes of dst behind the range
OK, BAD_MAGIC, BAD_CRC, BAD_SIZE, BAD_DIGEST, CRC_ONLY, BAD_DATA, BAD_TAG = range(8)
PLAIN, ZSTD, ENC, ENC_ZSTD = range(4)


@pytest.fixture(scope="module")
def eng():
    from pbs_plus_amd import Engine, buzhash

    e = Engine(buzhash.NewConfig(4096), device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def keys(eng):
    from pbs_plus_amd import AesKey

    k = {"right": AesKey(eng, ai.key_of(5)), "wrong": AesKey(eng, ai.key_of(6))}
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

    return blob_magic(kind) + zlib.crc32(body).to_bytes(4, "little") + iv + tag + body  # (the CRC covers what follows the header)


@pytest.fixture(scope="module")
def world(eng, keys):
    """the blobs (bytes per blob, by name), the entries [(blob name, content)] and what each blob is"""
    z = {c["name"]: c for c in zstd_inputs.cases() if c["status"] == 0}
    contents = {
        "p0": (PLAIN, ai.pattern(3000, 1)), "p1": (PLAIN, ai.pattern(40001, 2)),
        "z0": (ZSTD, z["lowsym-3000"]), "e0": (ENC, ai.pattern(3001, 3)), "e1": (ENC, ai.pattern(5000, 4)),
        "e2": (ENC, ai.pattern(70001, 5)), "e3": (ENC, ai.pattern(17, 6)),
        "ez0": (ENC_ZSTD, z["text-60000-level1"]), "ez1": (ENC_ZSTD, z["many-90000"]), "ez2": (ENC_ZSTD, z["hand-rle-block"]),
        "eg": (ENC_ZSTD, dict(frame=ai.pattern(500, 7), content=ai.pattern(500, 8))),  # a good tag over garbage
    }
    enc = [n for n, (k, _) in contents.items() if k in (ENC, ENC_ZSTD)]
    ivs = [ai.pattern(16, 700 + i) for i in range(len(enc))]
    plains = [contents[n][1] if contents[n][0] == ENC else contents[n][1]["frame"] for n in enc]
    sealed = dict(zip(enc, zip(ivs, encrypt_many(eng, keys["right"], plains, ivs))))
    blobs, content = {}, {}
    for n, (kind, c) in contents.items():
        if kind == PLAIN:
            blobs[n], content[n] = frame_blob(kind, c), c
        elif kind == ZSTD:
            blobs[n], content[n] = frame_blob(kind, c["frame"]), c["content"]
        else:
            iv, (ct, tag) = sealed[n]
            blobs[n] = frame_blob(kind, ct, iv, tag)
            content[n] = c if kind == ENC else c["content"]
    # e1 is named by three entries; the first and the last entry are encrypted and clipped by the range
    order = ["e0", "p0", "e1", "z0", "ez0", "e1", "e2", "p1", "ez1", "e3", "e1", "ez2", "ez0"]
    return dict(blobs=blobs, content=content, kinds={n: k for n, (k, _) in contents.items()}, order=order)


def restore(eng, w, key, order=None, blobs=None, sizes=None, zstd=True, aes=None, clip=(1000, 777), digest=False, call="decode3"):
    """-> (status, the range's bytes as restored, dst's tail, stats, the stream, (start, end))"""
    from pbs_plus_amd import RECORD_DTYPE

    order = order or w["order"]
    blobs = dict(w["blobs"], **(blobs or {}))
    names = sorted(set(order))
    buf, ranges = bytearray(), []
    for n in names:
        buf += bytes(3)  # blobs at odd offsets
        ranges.append((len(buf), len(blobs[n])))
        buf += blobs[n]
    host = np.frombuffer(bytes(buf) + bytes(16), np.uint8)
    size = [len(w["content"][n]) for n in order]
    if sizes:
        for i, v in sizes.items():
            size[i] = v
    idx = np.zeros(len(order), dtype=RECORD_DTYPE)
    idx["size"] = size
    idx["end"] = np.cumsum(np.array(size, dtype=np.uint64))
    stream = b"".join(w["content"][n] for n in order)
    start, end = clip[0], int(idx["end"][-1]) - clip[1]
    blob_of = np.array([names.index(n) for n in order], dtype=np.uint32)
    src, dst = eng.alloc(host.size), eng.alloc(end - start + TAIL)
    try:
        src.upload(host)
        dst.upload(np.full(end - start + TAIL, FILL, np.uint8))
        args = (src, np.array(ranges, dtype=np.uint64), idx, blob_of, start, end, digest)
        try:
            if call == "decode3":
                _, status, stats = eng.blob_decode3(*args, dst=dst, zstd=zstd, key=key, aes=aes)
            else:
                _, status, stats = eng.blob_decode2(*args, dst=dst, zstd=zstd)
        except Exception:
            assert np.all(dst.download(0, end - start + TAIL) == FILL), "a refused call wrote to dst"
            raise
        got = dst.download(0, end - start + TAIL)
        verify = eng.blob_verify(src, np.array(ranges, dtype=np.uint64))[0]
    finally:
        src.free()
        dst.free()
    assert np.all(got[end - start:] == FILL), "a byte behind the range was written"
    return dict(status=status, got=got[:end - start].tobytes(), stats=stats, stream=stream, span=(start, end), idx=idx, names=names,
                verify=verify)


def part(r, i):
    """entry i's part of the range, as (restored bytes, the stream's bytes)"""
    start, end = r["span"]
    lo = max(int(r["idx"]["end"][i]) - int(r["idx"]["size"][i]), start)
    hi = min(int(r["idx"]["end"][i]), end)
    return r["got"][lo - start:hi - start], r["stream"][lo:hi]


def test_the_plaintext_stream_byte_for_byte(eng, keys, world):
    r = restore(eng, world, keys["right"])
    assert not r["status"].any(), r["status"]
    start, end = r["span"]
    assert r["got"] == r["stream"][start:end]
    distinct = {n for n in world["order"] if world["kinds"][n] in (ENC, ENC_ZSTD)}
    assert r["stats"]["aes_bytes"] == sum(len(world["blobs"][n]) - 44 for n in distinct)  # each distinct blob once
    assert r["stats"]["ok"] == len(world["order"]) and r["stats"]["out_bytes"] == end - start
    frames = {n for n in distinct if world["kinds"][n] == ENC_ZSTD}
    assert r["stats"]["zstd_in_bytes"] == sum(len(world["blobs"][n]) - 44 for n in frames) + len(world["blobs"]["z0"]) - 12
    # the digest check is not applied to encrypted entries: with it, only the others are compared (their digests are zero here)
    d = restore(eng, world, keys["right"], digest=True)
    for i, n in enumerate(world["order"]):
        assert d["status"][i] == (OK if world["kinds"][n] in (ENC, ENC_ZSTD) else BAD_DIGEST), n


def test_without_the_flag_it_is_decode2(eng, keys, world):
    for zstd in (True, False):
        a = restore(eng, world, keys["right"], zstd=zstd, aes=False)
        b = restore(eng, world, None, zstd=zstd, call="decode2")
        assert np.array_equal(a["status"], b["status"]) and a["got"] == b["got"]
        assert {k: v for k, v in a["stats"].items() if k not in ("aes_bytes", "bad_tag")} == b["stats"]
        assert a["stats"]["aes_bytes"] == 0 and a["stats"]["bad_tag"] == 0
        for i, n in enumerate(world["order"]):
            if world["kinds"][n] in (ENC, ENC_ZSTD):
                assert a["status"][i] == CRC_ONLY and set(part(a, i)[0]) <= {FILL}, n
    # blob_verify on the same buffer still says CRC_ONLY for both encrypted kinds
    for n, v in zip(a["names"], a["verify"]):
        assert v == (CRC_ONLY if world["kinds"][n] != PLAIN else OK), n


def test_an_encrypted_compressed_blob_without_zstd_stays_crc_only(eng, keys, world):
    r = restore(eng, world, keys["right"], zstd=False)
    for i, n in enumerate(world["order"]):
        k = world["kinds"][n]
        assert r["status"][i] == (OK if k in (PLAIN, ENC) else CRC_ONLY), n
        got, want = part(r, i)
        assert got == want if k in (PLAIN, ENC) else set(got) <= {FILL}, n


def test_a_bad_crc_is_not_decrypted_and_a_bad_tag_hands_out_nothing(eng, keys, world):
    b = world["blobs"]
    flip = lambda x, at: x[:at] + bytes([x[at] ^ 1]) + x[at + 1:]  # noqa: E731
    resealed = lambda x: x[:8] + zlib.crc32(x[44:]).to_bytes(4, "little") + x[12:]  # noqa: E731
    bad = {"e2": flip(b["e2"], 50000),                # ciphertext damaged, CRC not updated
           "e1": resealed(flip(b["e1"], 30)),         # a tag byte flipped, CRC good: three entries, copies out of scratch or in place
           "e3": resealed(flip(b["e3"], 50)),         # a ciphertext byte flipped, CRC good
           "ez1": resealed(flip(b["ez1"], 13))}       # an IV byte flipped, CRC good
    r = restore(eng, world, keys["right"], blobs=bad)
    good = restore(eng, world, keys["right"])
    want = {"e2": BAD_CRC, "e1": BAD_TAG, "e3": BAD_TAG, "ez1": BAD_TAG}
    for i, n in enumerate(world["order"]):
        assert r["status"][i] == want.get(n, OK), n
        got, stream = part(r, i)
        if n == "e2":
            assert set(got) <= {FILL}, n                    # untouched
        elif n in want:
            assert set(got) <= {FILL} or set(got) == {0}, n  # untouched, or zero where it was decrypted in place
            assert got != stream
        else:
            assert got == stream, n
    assert r["stats"]["aes_bytes"] == good["stats"]["aes_bytes"] - (len(b["e2"]) - 44)  # the bad CRC is not decrypted
    assert r["stats"]["bad_tag"] == 5 and r["stats"]["bad_crc"] == 1
    # e3 lies wholly inside the range and no other entry names it: decrypted in place, so its part is zero
    i3 = world["order"].index("e3")
    assert set(part(r, i3)[0]) == {0}


def test_the_wrong_key_is_a_bad_tag_on_every_encrypted_entry(eng, keys, world):
    r = restore(eng, world, keys["wrong"])
    for i, n in enumerate(world["order"]):
        k = world["kinds"][n]
        assert r["status"][i] == (BAD_TAG if k in (ENC, ENC_ZSTD) else OK), n
        got, stream = part(r, i)
        if k in (PLAIN, ZSTD):
            assert got == stream, n
        else:
            assert (set(got) <= {FILL} or set(got) == {0}) and (got != stream or not got), n


def test_garbage_behind_a_good_tag_and_a_wrong_size(eng, keys, world):
    order = world["order"] + ["eg", "p0"]
    i_e2, i_ez2 = world["order"].index("e2"), world["order"].index("ez2")
    r = restore(eng, world, keys["right"], order=order, sizes={i_e2: 70000, i_ez2: 1001}, clip=(0, 0))
    for i, n in enumerate(order):
        want = BAD_DATA if n == "eg" else BAD_SIZE if i in (i_e2, i_ez2) else OK
        assert r["status"][i] == want, (n, r["status"][i])
    assert r["stats"]["bad_data"] == 1 and r["stats"]["bad_size"] == 2


def test_the_flag_without_a_key_is_refused_with_dst_untouched(eng, keys, world):
    from pbs_plus_amd import PbsGpuError, _lib

    with pytest.raises(PbsGpuError) as ei:
        restore(eng, world, None, aes=True)
    assert ei.value.status == _lib.E_INVALID
    from pbs_plus_amd import AesKey, Engine, buzhash

    other = Engine(buzhash.NewConfig(4096), device=0)
    try:
        with AesKey(other, ai.key_of(5)) as foreign, pytest.raises(PbsGpuError) as ei:
            restore(eng, world, foreign)  # a key of another engine
        assert ei.value.status == _lib.E_INVALID
    finally:
        other.close()
