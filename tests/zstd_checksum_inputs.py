"""What the checksum and stream tests share (tests/test_zstd_checksum_native.py, tests/test_gpu_zstd_checksum.py): the
cases of tests/golden/zstd_checksum_v1.json with their regenerated content, and what is derived from them by construction:
frames with a flipped checksum byte or a flipped byte of a raw block, whole streams with the status and the content a
decoder must report for them (tests/golden/make_zstd_checksum_golden.py asks libzstd the same when it writes the file),
and the contents the encoder tests compress. Computed once, shared, not to be changed."""
import base64
import json
import os
import struct

import numpy as np

import zstd_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_FRAME, BAD_SIZE, UNSUPPORTED, BAD_CHECKSUM = range(5)
F_CHECKSUM, F_STREAM = 1, 2

XXH_LENGTHS = (0, 1, 3, 4, 7, 8, 31, 32, 33, 63, 64, 65, 95, 96, 97, 4095, 4096, 4097)
XXH_SEEDS = (0, 0x9E3779B97F4A7C15)
# contents of make_zstd_golden.content_of(): empty, tiny (raw blocks), text, incompressible (a raw block), many symbols, one
# byte (three RLE blocks), low entropy. Small, so that the golden file stays small: frames of several compressed blocks
# with a checksum are the encoder's own (ENC_CONTENTS)
FRAME_CONTENTS = (("text-0", 0), ("text-1", 1), ("text-3", 3), ("text-8000", 8_000), ("rand-2000", 2_000),
                  ("many-3000", 3_000), ("byte-300000", 300_000), ("lowsym-3000", 3_000))
ENC_SIZES = (0, 1, 255, 256, 65_791, 65_792, 131_072, 131_073, 300_000)
ENC_CONTENTS = tuple(("mixed", n) for n in ENC_SIZES) + (("rand", 1), ("rand", 300_000))

_cache = {}


def pattern(n):
    i = np.arange(n, dtype=np.uint64)
    return ((i * i * 31 + i * 7 + 13) & 255).astype(np.uint8).tobytes()


def enc_content(name, n):
    key = ("enc", name, n)
    if key not in _cache:
        _cache[key] = zstd_inputs.golden().content_of("%s-%d" % (name, n), n)
    return _cache[key]


def golden():
    if "json" not in _cache:
        _cache["json"] = json.load(open(os.path.join(ROOT, "tests", "golden", "zstd_checksum_v1.json")))
    return _cache["json"]


def frames():
    """the libzstd frames with a checksum: name, frame, content, length, xxh64 (of the content, seed 0)"""
    if "frames" not in _cache:
        g = zstd_inputs.golden()
        _cache["frames"] = [dict(name=f["name"], frame=base64.b64decode(f["frame"]), content=g.content_of(f["content"], f["length"]),
                                 length=f["length"], xxh64=int(f["xxh64"], 16)) for f in golden()["frames"]]
    return _cache["frames"]


def frame(name):
    return next(f for f in frames() if f["name"] == name)


def raw_block_byte(fr):
    """the position of the middle byte of the first non-empty raw block of a frame; None if it has none"""
    fhd = fr[4]
    single, fcs_flag, did = fhd >> 5 & 1, fhd >> 6, (0, 1, 2, 4)[fhd & 3]
    pos = 5 + (0 if single else 1) + did + (single if fcs_flag == 0 else 1 << fcs_flag)
    while True:
        bh = int.from_bytes(fr[pos:pos + 3], "little")
        last, kind, size = bh & 1, bh >> 1 & 3, bh >> 3
        if kind == 0 and size:
            return pos + 3 + size // 2
        pos += 3 + (1 if kind == 1 else size)
        if last:
            return None


def flip(fr, at, xor):
    return fr[:at] + bytes([fr[at] ^ xor]) + fr[at + 1:]


def flipped():
    """every frame with a checksum byte flipped, and with a byte of a raw block flipped where it has one: still a frame
    that decodes, to what its checksum does not say. name, frame, length (of what it decodes to), kind"""
    if "flipped" not in _cache:
        out = []
        for k, f in enumerate(frames()):
            fr = f["frame"]
            out.append(dict(name=f["name"] + "-sumflip", frame=flip(fr, len(fr) - 1 - k % 4, 0x40), length=f["length"], kind="sum"))
            at = raw_block_byte(fr)
            if at is not None:
                out.append(dict(name=f["name"] + "-rawflip", frame=flip(fr, at, 0x01), length=f["length"], kind="raw"))
        assert sum(c["kind"] == "raw" for c in out) >= 4
        _cache["flipped"] = out
    return _cache["flipped"]


def skippable(n, nibble=0):
    return struct.pack("<II", 0x184D2A50 + nibble, n) + pattern(n)


MAGIC = struct.pack("<I", 0xFD2FB528)
RESERVED_BIT_FRAME = MAGIC + bytes([0x28, 0x00, 0x01, 0x00, 0x00])    # single segment, reserved bit 3 set
DICTIONARY_FRAME = MAGIC + bytes([0x21, 0x05, 0x00, 0x01, 0x00, 0x00])  # single segment, dictionary id 5, empty content


def streams():
    """whole streams: name, stream, status and content with both flags (content b"" unless OK), and the room to decode it
    into: exactly the content, and for a stream that fails enough for every frame in it"""
    if "streams" not in _cache:
        a, b, c = frame("text-8000-level1"), frame("rand-2000-level3"), frame("lowsym-3000-level1")
        n = next(x for x in zstd_inputs.cases() if x["name"] == "lowsym-3000")  # a frame without a checksum
        A, B, C, N = a["frame"], b["frame"], c["frame"], n["frame"]
        ca, cb, cc, cn = a["content"], b["content"], c["content"], n["content"]
        out = []

        def add(name, stream, status, content=b""):
            out.append(dict(name=name, stream=stream, status=status, content=content,
                            room=len(content) if status == OK else len(ca) + len(cb) + len(cc)))

        add("two", A + B, OK, ca + cb)
        add("three", A + N + C, OK, ca + cn + cc)
        add("skip-front", skippable(12) + A, OK, ca)
        add("skip-between", A + skippable(0, 5) + B, OK, ca + cb)
        add("skip-behind", A + skippable(100, 15), OK, ca)
        add("skip-everywhere", skippable(1) + C + skippable(9, 3) + skippable(0) + N + skippable(5, 1), OK, cc + cn)
        add("skip-alone", skippable(33), OK)
        add("skips-alone", skippable(0) + skippable(7, 9), OK)
        add("empty", b"", OK)
        add("one", C, OK, cc)
        add("skip-cut-header", A + skippable(10)[:6], BAD_FRAME)
        add("skip-cut-body", A + skippable(50)[:-1], BAD_FRAME)
        add("garbage-behind", A + b"\x01\x02\x03\x04", BAD_FRAME)
        add("three-bytes-behind", C + MAGIC[:3], BAD_FRAME)
        add("second-cut", A + B[:len(B) // 2], BAD_FRAME)
        add("second-bad-checksum", A + flip(B, len(B) - 2, 0x11), BAD_CHECKSUM)
        add("second-bad-raw-byte", C + flip(B, raw_block_byte(B), 0x80), BAD_CHECKSUM)
        add("first-bad-checksum", flip(C, len(C) - 4, 0x01) + A, BAD_CHECKSUM)
        add("middle-bad", A + RESERVED_BIT_FRAME + C, BAD_FRAME)
        add("middle-dictionary", C + DICTIONARY_FRAME + A, UNSUPPORTED)
        _cache["streams"] = out
    return _cache["streams"]
