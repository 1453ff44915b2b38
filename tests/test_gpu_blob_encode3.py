"""Encrypted blobs written on the device (pbsgpu_blob_encode3_device, Engine.blob_encode3). With F_AES alone every blob is
compared byte for byte with magic | CRC-32 of the ciphertext | IV | tag | ciphertext made on the CPU (the pure-Python GCM of
tests/aes_inputs.py up to 70 KiB, libcrypto where it loads; for longer messages without libcrypto the device's batch cipher,
a different piece kernel that tests/test_gpu_aes.py holds against recorded answers). With F_AES | F_ZSTD the expectation
comes from Engine.zstd_encode of the same chunk on the same engine: kind 3 over the frame when it is shorter, kind 2 over
the chunk otherwise. Then the round trip through blob_decode3, a call with more pieces than workgroups, and the older call's
outputs without the flag. The chunks lie at offsets of differing residues mod 16; dst is pre-filled and 256 bytes longer than
the slots, so a byte stored outside them is seen."""
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aes_inputs as ai  # noqa: E402
import zstd_enc_inputs as zi  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0xA5
TAIL = 256
OK, CRC_ONLY, BAD_TAG = 0, 5, 7
ENC, ENC_ZSTD = 2, 3
HDR = 44
LENGTHS = (1, 15, 16, 17, 4095, 65535, 65536, 65537, 3 * 65536 + 5, 0)  # (pbsgpu_blob_encode_device takes an empty chunk)
PY_LIMIT = 70 << 10  # the pure-Python GCM runs at about 14 us per byte


@pytest.fixture(scope="module")
def eng():
    from pbs_plus_amd import Engine, buzhash

    e = Engine(buzhash.NewConfig(4096), device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def keys(eng):
    from pbs_plus_amd import AesKey

    raw = {"right": ai.key_of(5), "wrong": ai.key_of(6)}
    k = {n: AesKey(eng, v) for n, v in raw.items()}
    k["raw"] = raw
    yield k
    for n in raw:
        k[n].close()


def frame_blob(kind, body, iv, tag):
    from pbs_plus_amd import blob_magic

    return blob_magic(kind) + zlib.crc32(body).to_bytes(4, "little") + iv + tag + body  # (the CRC covers the ciphertext only)


def seal(eng, key, raw_key, plains, ivs):
    """[(ciphertext, tag)] from outside the call under test: libcrypto for every message where it loads (the pure-Python
    GCM must agree on the short ones); where it does not, pure Python up to PY_LIMIT and the device's batch cipher for the
    longer ones"""
    out = [None] * len(plains)
    for i, (p, iv) in enumerate(zip(plains, ivs)):
        if ai.libcrypto() is not None:
            out[i] = ai.libcrypto_encrypt(raw_key, iv, p)
            if len(p) <= 4096:
                c = ai.gcm_encrypt(raw_key, iv, p)
                assert (bytes(out[i][0]), bytes(out[i][1])) == (bytes(c[0]), bytes(c[1]))
        elif len(p) <= PY_LIMIT:
            out[i] = ai.gcm_encrypt(raw_key, iv, p)
    rest = [i for i, v in enumerate(out) if v is None]
    if rest:
        buf = np.frombuffer(b"".join(plains[i] for i in rest) + bytes(16), np.uint8)
        lens = np.array([len(plains[i]) for i in rest], dtype=np.uint64)
        segs = np.stack([np.cumsum(lens) - lens, lens], axis=1)
        src = eng.alloc(buf.size)
        try:
            src.upload(buf)
            dst, status, tags, _ = eng.aes_gcm_many(key, src, segs, [ivs[i] for i in rest], encrypt=True)
            got = dst.download(0, max(int(lens.sum()), 1))
            dst.free()
        finally:
            src.free()
        assert not status.any()
        for j, i in enumerate(rest):
            out[i] = (got[int(segs[j, 0]):int(segs[j, 0] + segs[j, 1])].tobytes(), tags[j].tobytes())
    return [(bytes(c), bytes(t)) for c, t in out]


def lay_out(chunks):
    """the chunks in one source buffer at offsets of differing residues mod 16: (host bytes, ranges)"""
    buf, ranges = bytearray(), []
    for i, c in enumerate(chunks):
        want = (5 * i + 1) % 16
        buf += bytes((want - len(buf)) % 16)
        ranges.append((len(buf), len(c)))
        buf += c
    assert len({o % 16 for o, _ in ranges}) == min(len(chunks), 16)
    return np.frombuffer(bytes(buf) + bytes(16), np.uint8), np.array(ranges, dtype=np.uint64).reshape(-1, 2)


class Run:
    """one call of blob_encode3 into a pre-filled dst with a tail; the buffers stay for a restore until free()"""

    def __init__(self, eng, chunks, key, ivs, zstd, aes=None, header=HDR, call="encode3", cap=None):
        self.eng, self.chunks = eng, chunks
        host, self.ranges = lay_out(chunks)
        self.total = sum(header + len(c) for c in chunks)
        self.src, self.dst = eng.alloc(host.size), eng.alloc(self.total + TAIL)
        try:
            self.src.upload(host)
            self.dst.upload(np.full(self.total + TAIL, FILL, np.uint8))
            view = self.dst if cap is None else _View(self.dst.ptr, cap)
            try:
                if call == "encode3":
                    _, self.offs, self.lens, self.kinds, self.crcs, self.stats, self.ivs = eng.blob_encode3(
                        self.src, self.ranges, key=key, ivs=ivs, dst=view, zstd=zstd, aes=aes)
                else:
                    _, self.offs, self.lens, self.kinds, self.crcs, self.stats = eng.blob_encode2(self.src, self.ranges, dst=view, zstd=zstd)
            except Exception:
                assert np.all(self.dst.download(0, self.total + TAIL) == FILL), "a refused call wrote to dst"
                raise
            self.got = self.dst.download(0, self.total + TAIL)
        except Exception:
            self.free()
            raise
        assert np.all(self.got[self.total:] == FILL), "a byte behind the slots was written"
        assert int(self.offs[0]) == 0 and int(self.offs[-1]) == self.total
        assert np.array_equal(np.diff(self.offs), header + self.ranges[:, 1])  # the slots, back to back

    def blob(self, i):
        return self.got[int(self.offs[i]):int(self.offs[i]) + int(self.lens[i])].tobytes()

    def restore(self, key, only=None):
        """the blobs (all, or those of `only`) through blob_decode3: (status, restored bytes, blob_verify's statuses)"""
        from pbs_plus_amd import RECORD_DTYPE

        which = [i for i in (range(len(self.chunks)) if only is None else only)]
        blobs = np.stack([self.offs[which], self.lens[which].astype(np.uint64)], axis=1)
        idx = np.zeros(len(which), dtype=RECORD_DTYPE)
        idx["size"] = [len(self.chunks[i]) for i in which]
        idx["end"] = np.cumsum(idx["size"].astype(np.uint64))
        end = int(idx["end"][-1])
        out = self.eng.alloc(end + TAIL)
        try:
            out.upload(np.full(end + TAIL, FILL, np.uint8))
            _, status, _ = self.eng.blob_decode3(self.dst, blobs, idx, None, 0, end, False, dst=out, key=key)
            got = out.download(0, end + TAIL)
            verify = self.eng.blob_verify(self.dst, blobs)[0]
        finally:
            out.free()
        assert np.all(got[end:] == FILL)
        return status, got[:end].tobytes(), verify, b"".join(self.chunks[i] for i in which)

    def free(self):
        self.src.free()
        self.dst.free()


class _View:
    def __init__(self, ptr, nbytes):
        self.ptr, self.nbytes = ptr, nbytes


def make_ivs(n, salt):
    return [ai.pattern(16, salt + i) for i in range(n)]


@pytest.fixture(scope="module")
def plain_set(eng, keys):
    """F_AES alone over LENGTHS: the run and the CPU's (ciphertext, tag) per chunk"""
    chunks = [ai.pattern(n, 40 + i) for i, n in enumerate(LENGTHS)]
    assert sum(len(c) for c in chunks if len(c) <= PY_LIMIT) < 400 << 10
    ivs = make_ivs(len(chunks), 800)
    r = Run(eng, chunks, keys["right"], ivs, zstd=False)
    sealed = seal(eng, keys["right"], keys["raw"]["right"], chunks, ivs)
    yield r, ivs, sealed
    r.free()


def zstd_chunks():
    repeat = ai.pattern(512, 77)
    half = ai.pattern(200_000, 9) + repeat * (200_000 // 512 + 1)
    noise = np.random.default_rng(12)  # (ai.pattern repeats itself over tens of KiB: the encoder finds that)
    return [bytes(300_000), zi.content_of("text-131072"), half[:400_000]] + [noise.bytes(n) for n in (17, 4096, 70_001)]


@pytest.fixture(scope="module")
def zstd_set(eng, keys):
    """F_AES | F_ZSTD over chunks with verdicts both ways: the run, and per chunk (kind, message) from Engine.zstd_encode"""
    chunks = zstd_chunks()
    ivs = make_ivs(len(chunks), 900)
    r = Run(eng, chunks, keys["right"], ivs, zstd=True)
    fdst, status, flen, out = eng.zstd_encode(r.src, r.ranges)
    try:
        fbytes = fdst.download()
    finally:
        fdst.free()
    assert not status.any()
    want = []
    for i, c in enumerate(chunks):
        frame = fbytes[int(out[i, 0]):int(out[i, 0]) + int(flen[i])].tobytes()
        want.append((ENC_ZSTD, frame) if len(frame) < len(c) else (ENC, c))
    sealed = seal(eng, keys["right"], keys["raw"]["right"], [m for _, m in want], ivs)
    yield r, ivs, want, sealed
    r.free()


def test_aes_alone_every_blob_byte_for_byte(plain_set):
    r, ivs, sealed = plain_set
    n = len(LENGTHS)
    for i, (ct, tag) in enumerate(sealed):
        assert len(ct) == LENGTHS[i]
        assert r.blob(i) == frame_blob(ENC, ct, ivs[i], tag), LENGTHS[i]
        assert r.crcs[i] == zlib.crc32(ct), LENGTHS[i]
    assert np.array_equal(r.lens, HDR + np.array(LENGTHS)) and np.all(r.kinds == ENC)
    assert np.array_equal(r.ivs, np.frombuffer(b"".join(ivs), np.uint8).reshape(n, 16))
    total = sum(LENGTHS)
    assert r.stats == dict(blobs=[0, 0, n, 0], blob_bytes=[0, 0, total + HDR * n, 0], chunk_bytes=[0, 0, total, 0], frame_bytes=0,
                           crc_bytes=total, aes_bytes=total)


def test_aes_and_zstd_the_frame_is_encrypted_when_it_is_shorter(zstd_set):
    r, ivs, want, sealed = zstd_set
    stats = dict(blobs=[0] * 4, blob_bytes=[0] * 4, chunk_bytes=[0] * 4, frame_bytes=0, crc_bytes=0, aes_bytes=0)
    for i, ((kind, msg), (ct, tag)) in enumerate(zip(want, sealed)):
        assert r.kinds[i] == kind and r.lens[i] == HDR + len(msg), i
        assert r.blob(i) == frame_blob(kind, ct, ivs[i], tag), i
        assert r.crcs[i] == zlib.crc32(ct), i
        stats["blobs"][kind] += 1
        stats["blob_bytes"][kind] += HDR + len(msg)
        stats["chunk_bytes"][kind] += len(r.chunks[i])
        stats["frame_bytes"] += len(msg) if kind == ENC_ZSTD else 0
        stats["crc_bytes"] += len(msg)
        stats["aes_bytes"] += len(msg)
    assert r.stats == stats
    kinds = [k for k, _ in want]
    assert kinds[:3] == [ENC_ZSTD] * 3 and kinds[3:] == [ENC] * 3  # the set holds both kinds
    assert len(want[0][1]) < 65536 < len(r.chunks[0])  # planned pieces past the frame's end are skipped
    assert len(want[2][1]) > 65536                     # a frame that crosses a piece boundary, encrypted where it lies


def test_round_trip_through_the_restore(plain_set, zstd_set, keys):
    for r in (plain_set[0], zstd_set[0]):
        only = [i for i, c in enumerate(r.chunks) if len(c)]
        status, got, verify, content = r.restore(keys["right"], only)
        assert not status.any() and got == content
        assert np.all(verify == CRC_ONLY)  # a good CRC and a magic the older calls know
        status, got, _, content = r.restore(keys["wrong"], only)
        assert np.all(status == BAD_TAG)
        assert set(got) <= {FILL, 0}


def test_more_pieces_than_workgroups(eng, keys):
    rng = np.random.default_rng(3)
    lens = rng.integers(1, 301, size=2100)
    lens[:4] = (1, 300, 16, 17)
    chunks = [ai.pattern(int(n), 3000 + i) for i, n in enumerate(lens)]
    ivs = np.frombuffer(ai.pattern(16 * 2100, 31), np.uint8).reshape(2100, 16)
    r = Run(eng, chunks, keys["right"], ivs, zstd=False)
    try:
        assert np.all(r.kinds == ENC) and np.array_equal(r.lens, HDR + lens)
        for i in list(range(4)) + [int(v) for v in rng.choice(np.arange(4, 2100), size=28, replace=False)]:
            ct, tag = ai.gcm_encrypt(keys["raw"]["right"], ivs[i].tobytes(), chunks[i])
            assert r.blob(i) == frame_blob(ENC, bytes(ct), ivs[i].tobytes(), bytes(tag)), i
        status, got, verify, content = r.restore(keys["right"])
        assert not status.any() and got == content and np.all(verify == CRC_ONLY)
    finally:
        r.free()


def test_without_the_flag_it_is_blob_encode2(eng, keys):
    chunks = zstd_chunks() + [ai.pattern(n, 60 + n) for n in (1, 17, 4095)] + [b""]
    for zstd in (False, True):
        old = Run(eng, chunks, None, None, zstd=zstd, header=12, call="encode2")
        try:
            for key, aes in ((None, None), (keys["right"], False)):
                new = Run(eng, chunks, key, None, zstd=zstd, aes=aes, header=12)
                try:
                    assert np.array_equal(new.offs, old.offs) and np.array_equal(new.lens, old.lens)
                    assert np.array_equal(new.kinds, old.kinds) and np.array_equal(new.crcs, old.crcs)
                    for i in range(len(chunks)):
                        assert new.blob(i) == old.blob(i), i
                    assert new.stats["aes_bytes"] == 0 and new.ivs.shape == (0, 16)
                    for k in ("blobs", "blob_bytes", "chunk_bytes"):
                        assert new.stats[k] == old.stats[k] + [0, 0], k
                    assert new.stats["frame_bytes"] == old.stats["frame_bytes"] and new.stats["crc_bytes"] == old.stats["crc_bytes"]
                finally:
                    new.free()
            assert (len(set(old.kinds)) == 2) == zstd
        finally:
            old.free()


def test_two_keys_give_different_blobs_and_each_decodes_under_its_own(eng, keys):
    chunks = [ai.pattern(n, 70 + n) for n in (100, 5000, 65537)] + [zi.content_of("text-4096")]
    ivs = make_ivs(len(chunks), 1000)
    a, b = Run(eng, chunks, keys["right"], ivs, zstd=True), Run(eng, chunks, keys["wrong"], ivs, zstd=True)
    try:
        assert np.array_equal(a.lens, b.lens) and np.array_equal(a.kinds, b.kinds) and set(a.kinds) == {ENC, ENC_ZSTD}
        for i in range(len(chunks)):
            x, y = a.blob(i), b.blob(i)
            assert x[:8] == y[:8] and x[12:28] == y[12:28] == ivs[i]  # magic and IV
            assert x[8:12] != y[8:12] and x[28:44] != y[28:44] and x[44:] != y[44:]
        for r, own, other in ((a, "right", "wrong"), (b, "wrong", "right")):
            status, got, _, content = r.restore(keys[own])
            assert not status.any() and got == content
            assert np.all(r.restore(keys[other])[0] == BAD_TAG)
    finally:
        a.free()
        b.free()


def test_default_ivs_are_drawn_and_returned(eng, keys):
    chunks = [ai.pattern(n, 90 + n) for n in (10, 1000, 70000)]
    r = Run(eng, chunks, keys["right"], None, zstd=False)
    try:
        assert r.ivs.shape == (3, 16) and len({v.tobytes() for v in r.ivs}) == 3
        for i in range(3):
            assert r.blob(i)[12:28] == r.ivs[i].tobytes()
        status, got, _, content = r.restore(keys["right"])
        assert not status.any() and got == content
    finally:
        r.free()


def test_refusals_leave_dst_untouched(eng, keys):
    from pbs_plus_amd import AesKey, Engine, PbsGpuError, _lib, buzhash

    chunks = [ai.pattern(n, 95 + n) for n in (100, 200, 300)]
    ivs = make_ivs(3, 1100)
    for zstd in (False, True):
        with pytest.raises(PbsGpuError) as ei:
            Run(eng, chunks, keys["right"], [ivs[0], ivs[1], ivs[0]], zstd=zstd)  # two equal IVs
        assert ei.value.status == _lib.E_INVALID
        with pytest.raises(PbsGpuError) as ei:
            Run(eng, chunks, None, ivs, zstd=zstd, aes=True)  # the flag without a key
        assert ei.value.status == _lib.E_INVALID
        with pytest.raises(PbsGpuError) as ei:
            Run(eng, chunks, keys["right"], ivs, zstd=zstd, cap=3 * HDR + 600 - 1)
        assert ei.value.status == _lib.E_CAPACITY
    other = Engine(buzhash.NewConfig(4096), device=0)
    try:
        with AesKey(other, ai.key_of(5)) as foreign, pytest.raises(PbsGpuError) as ei:
            Run(eng, chunks, foreign, ivs, zstd=True)  # a key of another engine
        assert ei.value.status == _lib.E_INVALID
    finally:
        other.close()
