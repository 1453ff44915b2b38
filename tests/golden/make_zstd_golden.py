"""Writes tests/golden/zstd_v1*.npz: the zstd frames the decoder tests read (tests/test_zstd_*.py, tests/test_gpu_zstd.py).

Run on a machine where libzstd.so.1 loads (ctypes; there is no Python zstd module): `python tests/golden/make_zstd_golden.py`.
The tests never need libzstd: every case's content is regenerated from its name by content_of(), and the files hold per
case the frame, the SHA-256 and the length of the content, the status a decoder must report and what the frame header
declares. Frames that libzstd does not emit on request are assembled by hand below.
"""
import ctypes as C
import ctypes.util
import glob
import hashlib
import os
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OK, BAD_FRAME, BAD_SIZE, UNSUPPORTED = range(4)
MAGIC = struct.pack("<I", 0xFD2FB528)


# ---- content, from the name alone -------------------------------------------------------------------------------------
def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def _text_few(n, seed):
    """words over fewer than 128 distinct byte values"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789", dtype=np.uint8)
    vocab = [letters[rng.integers(0, letters.size, size=int(k))].tobytes() for k in rng.integers(2, 11, size=400)]
    out, size = [], 0
    pick = rng.zipf(1.3, size=n // 3 + 16) % len(vocab)
    seps = rng.integers(0, 12, size=pick.size)
    for w, s in zip(pick, seps):
        piece = vocab[w] + (b" " if s else b".\n")
        out.append(piece)
        size += len(piece)
        if size >= n:
            break
    return b"".join(out)[:n]


def _text_many(n, seed):
    """skewed bytes over more than 128 distinct values, with phrases that repeat"""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, 221) ** 0.9
    sym = rng.permutation(256)[:220].astype(np.uint8)
    body = sym[rng.choice(220, size=n, p=p / p.sum())]
    for at in rng.integers(0, max(1, n - 64), size=n // 400):
        ln = int(rng.integers(4, 40))
        src = int(rng.integers(0, max(1, at)))
        body[at:at + ln] = body[src:src + ln][:len(body[at:at + ln])]
    return body.tobytes()


def _mixed(n, seed):
    rng = np.random.default_rng(seed)
    parts = [_text_few(180_000, seed + 1), _rand(12_000, seed + 2), bytes(140_000), _text_many(50_000, seed + 3),
             np.tile(np.frombuffer(_rand(977, seed + 4), dtype=np.uint8), 220).tobytes(),
             (rng.integers(0, 16, size=30_000, dtype=np.uint8) * 7 + 33).astype(np.uint8).tobytes()]
    parts.append(parts[0][5_000:65_000])      # far back-references
    parts.append(_text_few(150_000, seed + 5))
    parts.append(parts[3][:40_000])
    parts.append(b"xyz" * 9_000)
    data = b"".join(parts)
    while len(data) < n:
        data += data[len(data) // 3:len(data) // 3 + 50_000]
    return data[:n]


HAND = {}  # name -> content of the hand-assembled frames (filled below)


def content_of(name, length):
    """the content of case `name` (length bytes); b"" for the cases no decoder may accept"""
    kind = name.split("-")[0]
    if kind == "hand":
        return HAND[name]
    if kind == "text":
        data = _text_few(length, 11)
    elif kind == "many":
        data = _text_many(length, 12)
    elif kind == "rand":
        data = _rand(length, 13)
    elif kind == "byte":
        data = b"\x5a" * length
    elif kind == "period3":
        data = (b"abc" * (length // 3 + 1))[:length]
    elif kind == "period70000":
        data = (_rand(70_000, 14) * (length // 70_000 + 1))[:length]
    elif kind == "mixed":
        data = _mixed(length, 15)
    elif kind == "lowsym":
        data = np.random.default_rng(16).integers(0, 10, size=length, dtype=np.uint8).tobytes()
    elif kind == "bad":
        data = b""
    else:
        raise KeyError(name)
    assert len(data) == length, (name, len(data), length)
    return data


# ---- frames assembled by hand ------------------------------------------------------------------------------------------
def _block(kind, payload, size=None, last=False):
    size = len(payload) if size is None else size
    return struct.pack("<I", int(last) | kind << 1 | size << 3)[:3] + payload


def _lit_block(lit_type, fmt_bytes, data, last=False):
    """a compressed block of raw (0) or RLE (1) literals with a 1-, 2- or 3-byte size and no sequences"""
    n = len(data)
    if fmt_bytes == 1:
        head = bytes([lit_type | n << 3])
    elif fmt_bytes == 2:
        head = struct.pack("<H", lit_type | 1 << 2 | n << 4)
    else:
        head = struct.pack("<I", lit_type | 3 << 2 | n << 4)[:3]
    body = data if lit_type == 0 else data[:1]
    return _block(2, head + body + b"\x00", last=last)


def _hand_frames():
    out = []
    raw = bytes(range(97, 97 + 26)) * 3
    out.append(("hand-raw-block", MAGIC + b"\x20" + bytes([len(raw)]) + _block(0, raw, last=True), raw, OK))
    rle = b"\x07" * 1000
    out.append(("hand-rle-block", MAGIC + b"\x60" + struct.pack("<H", 1000 - 256) + _block(1, b"\x07", 1000, last=True), rle, OK))
    full = bytes((i * 7 + 3) & 255 for i in range(100))
    out.append(("hand-empty-last-block", MAGIC + b"\x00\x00" + _block(0, full) + _block(0, b"", last=True), full, OK))
    out.append(("hand-fcs8", MAGIC + b"\xe0" + struct.pack("<Q", len(raw)) + _block(0, raw, last=True), raw, OK))
    pieces = [(0, 1, bytes(range(20))), (0, 2, bytes(i & 255 for i in range(300))), (0, 3, bytes((i * 3) & 255 for i in range(5000))),
              (1, 1, b"\x11" * 20), (1, 2, b"\x22" * 300), (1, 3, b"\x33" * 5000)]
    body = b"".join(_lit_block(t, f, d, last=(i == len(pieces) - 1)) for i, (t, f, d) in enumerate(pieces))
    lits = b"".join(d for _, _, d in pieces)
    out.append(("hand-literal-forms", MAGIC + b"\xa0" + struct.pack("<I", len(lits)) + body, lits, OK))
    # 32 512 sequences in one block, the smallest count that takes the 3-byte form: all three tables in RLE mode
    # (literal length 0, match length 3, offset code 2 + two zero bits = offset 1), so a sequence costs two bits
    nseq = 0x7F00
    seqs = b"\x00" + b"\xff" + struct.pack("<H", nseq - 0x7F00) + bytes([1 << 6 | 1 << 4 | 1 << 2]) + b"\x00\x02\x00" + \
        bytes(nseq * 2 // 8) + b"\x01"
    many = b"x" * (1 + 3 * nseq)
    out.append(("hand-nseq-3-bytes", MAGIC + b"\xa0" + struct.pack("<I", len(many)) + _block(0, b"x") + _block(2, seqs, last=True),
                many, OK))
    one = MAGIC + b"\x20" + bytes([len(raw)]) + _block(0, raw, last=True)
    out.append(("bad-skippable-frame", struct.pack("<II", 0x184D2A53, 8) + b"skipped!", b"", UNSUPPORTED))
    out.append(("bad-two-frames", one + one, b"", UNSUPPORTED))
    out.append(("bad-dictionary-id", MAGIC + b"\x21" + b"\x09" + bytes([len(raw)]) + _block(0, raw, last=True), b"", UNSUPPORTED))
    out.append(("bad-trailing-garbage", one + b"\x00\x01\x02", b"", UNSUPPORTED))
    out.append(("bad-reserved-block-type", MAGIC + b"\x20" + bytes([len(raw)]) + _block(3, raw, last=True), b"", BAD_FRAME))
    out.append(("bad-content-size", MAGIC + b"\x20" + bytes([len(raw) - 1]) + _block(0, raw, last=True), b"", BAD_SIZE))
    out.append(("bad-magic", b"\x29" + one[1:], b"", BAD_FRAME))
    for cut in (3, 7, len(one) - 1):
        out.append(("bad-truncated-%d" % cut, one[:cut], b"", BAD_FRAME))
    return out


for _name, _frame, _content, _status in _hand_frames():
    HAND[_name] = _content


# ---- what a frame header declares (an independent reading, for pbsgpu_zstd_frame_info) ---------------------------------
def frame_info(frame):
    """(status, content_size or -1, window_size, header_bytes, has_checksum)"""
    if len(frame) < 4:
        return BAD_FRAME, -1, 0, 0, 0
    magic = struct.unpack_from("<I", frame)[0]
    if magic & 0xFFFFFFF0 == 0x184D2A50:
        return UNSUPPORTED, -1, 0, 0, 0
    if magic != 0xFD2FB528 or len(frame) < 5:
        return BAD_FRAME, -1, 0, 0, 0
    fhd = frame[4]
    single, did = fhd >> 5 & 1, (0, 1, 2, 4)[fhd & 3]
    fcs = (single, 2, 4, 8)[fhd >> 6]
    hb = 5 + (1 - single) + did + fcs
    if fhd & 8 or len(frame) < hb:
        return BAD_FRAME, -1, 0, 0, 0
    p, window = 5, 0
    if not single:
        base = 1 << (10 + (frame[p] >> 3))
        window = base + base // 8 * (frame[p] & 7)
        p += 1
    if did and int.from_bytes(frame[p:p + did], "little"):
        return UNSUPPORTED, -1, 0, 0, 0
    p += did
    size = -1
    if fcs:
        size = int.from_bytes(frame[p:p + fcs], "little") + (256 if fcs == 2 else 0)
    if single:
        window = size
    return OK, size, window, hb, fhd >> 2 & 1


# ---- libzstd through ctypes --------------------------------------------------------------------------------------------
class _Buf(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("size", C.c_size_t), ("pos", C.c_size_t)]


def load_libzstd():
    """the library, with the prototypes the generator and the comparison in tests/test_zstd_core_native.py use; None when absent"""
    for name in ("libzstd.so.1", ctypes.util.find_library("zstd")):
        if not name:
            continue
        try:
            z = C.CDLL(name)
        except OSError:
            continue
        z.ZSTD_compressBound.restype = C.c_size_t
        z.ZSTD_compressBound.argtypes = [C.c_size_t]
        z.ZSTD_isError.restype = C.c_uint
        z.ZSTD_isError.argtypes = [C.c_size_t]
        z.ZSTD_createCCtx.restype = C.c_void_p
        z.ZSTD_freeCCtx.argtypes = [C.c_void_p]
        z.ZSTD_CCtx_setParameter.restype = C.c_size_t
        z.ZSTD_CCtx_setParameter.argtypes = [C.c_void_p, C.c_int, C.c_int]
        z.ZSTD_compress2.restype = C.c_size_t
        z.ZSTD_compress2.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        z.ZSTD_compressStream2.restype = C.c_size_t
        z.ZSTD_compressStream2.argtypes = [C.c_void_p, C.POINTER(_Buf), C.POINTER(_Buf), C.c_int]
        z.ZSTD_decompress.restype = C.c_size_t
        z.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        return z
    return None


LEVEL, WINDOW_LOG, CONTENT_SIZE_FLAG, CHECKSUM_FLAG = 100, 101, 200, 201  # ZSTD_cParameter


def compress(z, data, level=3, checksum=False, content_size=True, stream_piece=0, window_log=0):
    cctx = z.ZSTD_createCCtx()
    try:
        for k, v in ((LEVEL, level), (CHECKSUM_FLAG, int(checksum)), (CONTENT_SIZE_FLAG, int(content_size)), (WINDOW_LOG, window_log)):
            assert not z.ZSTD_isError(z.ZSTD_CCtx_setParameter(cctx, k, v))
        cap = z.ZSTD_compressBound(len(data)) + 64
        dst = C.create_string_buffer(cap)
        if not stream_piece:
            n = z.ZSTD_compress2(cctx, dst, cap, data, len(data))
            assert not z.ZSTD_isError(n)
            return dst.raw[:n]
        src = C.create_string_buffer(data, len(data) or 1)  # fed in pieces: the encoder never learns the size
        ob = _Buf(C.addressof(dst), cap, 0)
        at = 0
        while True:
            take = min(stream_piece, len(data) - at)
            ib = _Buf(C.addressof(src) + at, take, 0)
            end = at + take == len(data)
            while True:
                left = z.ZSTD_compressStream2(cctx, C.byref(ob), C.byref(ib), 2 if end else 0)
                assert not z.ZSTD_isError(left)
                if (end and left == 0) or (not end and ib.pos == ib.size):
                    break
            at += take
            if end:
                return dst.raw[:ob.pos]
    finally:
        z.ZSTD_freeCCtx(cctx)


def decompress(z, frame, cap):
    """(bytes, None) or (None, error code) from ZSTD_decompress"""
    dst = C.create_string_buffer(max(cap, 1))
    n = z.ZSTD_decompress(dst, cap, frame, len(frame))
    if z.ZSTD_isError(n):
        return None, n
    return dst.raw[:n], None


def _library_cases(z):
    cases = []

    def add(name, length, **kw):
        data = content_of(name, length)
        frame = compress(z, data, **kw)
        got, err = decompress(z, frame, len(data))
        assert err is None and got == data, name
        cases.append((name, frame, data, OK))

    for n in (0, 1, 2, 3, 131_071, 131_072, 131_073):
        add("text-%d" % n, n)
    add("rand-140000", 140_000)
    add("byte-300000", 300_000)
    add("text-60000-level1", 60_000, level=1)
    add("many-90000", 90_000)
    add("many-90000-level19", 90_000, level=19)
    add("period3-50000", 50_000)
    add("period70000-300000", 300_000)
    for level in (1, 3, 19):
        add("mixed-1048576-level%d" % level, 1 << 20, level=level)
    add("lowsym-3000", 3_000)
    add("text-40000-checksum", 40_000, checksum=True)
    add("many-30000-checksum-level19", 30_000, checksum=True, level=19)
    add("text-50000-nosize", 50_000, content_size=False)
    add("byte-200-nosize", 200, content_size=False)
    add("text-400000-streamed-level7", 400_000, stream_piece=30_011, window_log=17, level=7)  # repeat table modes
    add("mixed-300000-streamed-checksum", 300_000, stream_piece=4_099, checksum=True, level=19, window_log=16)
    return cases


def load():
    """every case of the golden files, in file and case order: dicts with name, frame, sha256, length, status, info"""
    cases = []
    for path in sorted(glob.glob(os.path.join(HERE, "zstd_v1*.npz"))):
        with np.load(path) as f:
            off = f["frame_off"]
            for i, name in enumerate(f["names"]):
                cases.append({"name": str(name), "frame": f["frames"][off[i]:off[i + 1]].tobytes(), "sha256": f["sha256"][i].tobytes(),
                              "length": int(f["length"][i]), "status": int(f["status"][i]), "info": [int(v) for v in f["info"][i]]})
    return cases


def _save(path, cases):
    frames = b"".join(c[1] for c in cases)
    off = np.cumsum([0] + [len(c[1]) for c in cases]).astype(np.int64)
    np.savez(path, names=np.array([c[0] for c in cases]), frames=np.frombuffer(frames, dtype=np.uint8), frame_off=off,
             sha256=np.array([np.frombuffer(hashlib.sha256(c[2]).digest(), dtype=np.uint8) for c in cases]),
             length=np.array([len(c[2]) for c in cases], dtype=np.uint64), status=np.array([c[3] for c in cases], dtype=np.uint8),
             info=np.array([frame_info(c[1]) for c in cases], dtype=np.int64))
    print("%s: %d cases, %d bytes" % (os.path.basename(path), len(cases), os.path.getsize(path)))


def main():
    z = load_libzstd()
    assert z is not None, "libzstd.so.1 does not load here"
    lib = _library_cases(z)
    for name, frame, data, status in _hand_frames():  # libzstd reads the hand-assembled frames the same way
        if status == OK:
            got, err = decompress(z, frame, 1 << 17)
            assert err is None and got == data, name
    big = [c for c in lib if len(c[1]) > 30_000]
    _save(os.path.join(HERE, "zstd_v1.npz"), [c for c in lib if len(c[1]) <= 30_000] + _hand_frames())
    for c in big:  # one file each: every committed file stays well under 256 KiB
        _save(os.path.join(HERE, "zstd_v1_%s.npz" % c[0].replace("-", "_")), [c])


if __name__ == "__main__":
    main()
