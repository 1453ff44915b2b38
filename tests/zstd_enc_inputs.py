"""What the zstd encoder tests share: the case list, the contents (the generators of tests/golden/make_zstd_golden.py plus a
few of their own), one build and run of tests/native/test_zstd_encode.cpp per process, and the golden file."""
import json
import os
import struct
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_inputs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "zstd_enc_v1.json")
BLOCK = 128 << 10
SEQ_CAP = 24576

# one bit per branch, in the order of the enum in zstd_encode.h
BRANCHES = ("fcs_1 fcs_2 fcs_4 block_raw block_rle block_compressed empty_last_block lit_raw lit_rle huf_1stream huf_4stream "
            "weights_direct weights_fse nseq_0 nseq_below_128 nseq_2_bytes match_overlap match_offset_1 ll_extra ml_extra "
            "seq_cap huf_refused").split()
# lit_rle: a byte value's first occurrence in a block is a literal, so literals of one value mean a block of one value,
#   and that is an RLE block before the literals are looked at. The branch is kept: it costs one comparison.
UNREACHED = ("lit_rle",)

LENGTHS = (0, 1, 3, 4, 5, 255, 256, 65_791, 65_792, 131_071, 131_072, 131_073, 300_000)


def bound(n):
    return 5 + (1 if n <= 255 else 2 if n <= 65_791 else 4) + 3 * max(1, -(-n // BLOCK)) + n


def _unique(n, start=0):
    """n bytes over the values 0..119 in which no four consecutive bytes occur twice: groups of three digits of a counter,
    each digit in a range of its own"""
    out = bytearray()
    i = start
    while len(out) < n:
        out += bytes((i % 40, 40 + i // 40 % 40, 80 + i // 1600 % 40))
        i += 1
    return bytes(out[:n])


def _seqs(n):
    """a block of exactly n sequences: 12 n + 64 bytes without a repeat, then n times twelve of those bytes again behind a
    separator of three bytes that occurs once"""
    head = _unique(12 * n + 64)
    out = [head]
    for k in range(n):
        out.append(bytes((120 + k % 8, 120 + k // 8 % 8, 120 + (k + k // 64) % 8)) + head[12 * k:12 * k + 12])
    return b"".join(out)


def _cap():
    """more matches in one block than the encoder keeps sequences: two words of four bytes in turn, each behind one of
    thirty bytes drawn so that it seldom continues the match before it. There are few distinct runs of four bytes, so the
    hash table loses none, and a sequence spans five bytes"""
    import numpy as np
    out = bytearray()
    for k, sep in enumerate(np.random.default_rng(22).integers(64, 94, size=BLOCK // 5 + 1)):
        out += bytes((int(sep), 4 * (k % 2), 4 * (k % 2) + 1, 4 * (k % 2) + 2, 4 * (k % 2) + 3))
    return bytes(out[:BLOCK])


def content_of(name):
    kind, _, arg = name.partition("-")
    n = int(arg) if arg else 0
    if kind == "zeros":
        return bytes(n)
    if kind == "text10":
        import numpy as np
        rng = np.random.default_rng(21)
        words = [bytes(rng.integers(97, 107, size=int(k), dtype=np.uint8)) for k in rng.integers(2, 9, size=60)]
        out, size = [], 0
        for w in rng.zipf(1.4, size=n // 2 + 8) % len(words):
            out.append(words[w] + b"a")
            size += len(out[-1])
            if size >= n:
                break
        return b"".join(out)[:n]
    if kind == "four":  # four byte values: the direct weight description (three bytes) is the shorter one
        import numpy as np
        return np.random.default_rng(23).integers(0, 4, size=n, dtype=np.uint8).tobytes()
    if kind == "lits":
        return _unique(n)
    if kind == "seqs":
        return _seqs(n)
    if kind == "cap":
        return _cap()
    return zstd_inputs.golden().content_of(name, n)


def case_names():
    names = []
    for kind in ("text", "many", "rand", "byte", "period3", "zeros", "text10"):
        names += ["%s-%d" % (kind, n) for n in LENGTHS]
    names += ["period70000-300000", "mixed-4096", "mixed-300000", "mixed-1048576", "text-4096"]
    names += ["lits-%d" % n for n in (31, 32, 1023, 1024, 4095, 4096, 16383, 16384)]
    names += ["seqs-127", "seqs-128", "cap", "four-2000"]
    return names


_cache = {}


def cases():
    """[(name, content)], computed once, shared, not to be changed"""
    if "cases" not in _cache:
        _cache["cases"] = [(name, content_of(name)) for name in case_names()]
    return _cache["cases"]


def run_native():
    """builds tests/native/test_zstd_encode.cpp with g++ under ASan + UBSan and runs it over every case, once per process:
    (return code, stdout, stderr, [frame], [[index, frame length, coverage, literals, sequences]])"""
    if "run" in _cache:
        return _cache["run"]
    tmp = tempfile.mkdtemp(prefix="zstd_encode")
    path, fpath, rpath, exe = (os.path.join(tmp, n) for n in ("cases.bin", "frames.bin", "results.txt", "test_zstd_encode"))
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases())))
        for name, data in cases():
            f.write(struct.pack("<I", len(name)) + name.encode() + struct.pack("<Q", len(data)) + data)
    flags = ["-std=c++17", "-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
             "-Wall", "-Wextra"]
    subprocess.run(["g++", *flags, os.path.join(ROOT, "tests", "native", "test_zstd_encode.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    p = subprocess.run([exe, path, fpath, rpath], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=900)
    frames, rows = [], []
    if os.path.exists(fpath):
        blob = open(fpath, "rb").read()
        at = 0
        while at < len(blob):
            (n,) = struct.unpack_from("<Q", blob, at)
            frames.append(blob[at + 8:at + 8 + n])
            at += 8 + n
        rows = [[int(v, 0) for v in ln.split()] for ln in open(rpath)]
    _cache["run"] = (p.returncode, p.stdout, p.stderr, frames, rows)
    return _cache["run"]


def golden():
    """{name: [frame length, SHA-256 of the frame in hex]}"""
    if "golden" not in _cache:
        _cache["golden"] = json.load(open(GOLDEN))
    return _cache["golden"]
