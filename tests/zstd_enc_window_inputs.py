"""What the tests of the zstd encoder's long-range match finder share (pbsgpu_engine_options.zstd_window_log = 17, 18 or
19: a block's matches may start in the chunk's bytes in front of it): every case of zstd_enc_tables_inputs, two contents
with far repeats, contents crafted for the window's edges, one build and run of tests/native/test_zstd_encode_window.cpp
per process, and the golden file."""
import json
import os
import struct
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_enc_tables_inputs as ti  # noqa: E402

zi = ti.zi
ROOT = zi.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "zstd_enc_window_v1.json")
BLOCK = zi.BLOCK

# the frames the program writes per case, in this order: (window log, sequence tables); window 0 is the match finder
# that never leaves its block
MODES = ((0, 0), (0, 1), (17, 0), (17, 1), (19, 0), (19, 1))
WINDOW_MODES = MODES[2:]
KEY = {m: "w%d-t%d" % m for m in MODES}

# the bits the long-range match finder adds, behind ti.BRANCHES, in the order of the enum in zstd_encode.h
BRANCHES = ti.BRANCHES + "w_cand_history w_cross w_beyond w_of_18 w_chunk_start".split()
NEW = BRANCHES[len(ti.BRANCHES):]
UNREACHED = ti.UNREACHED  # every new bit is reached


PATTERN = bytes(range(200, 224))  # 24 bytes, each value once


def _edge(n, source, copy):
    """n zero bytes, but for PATTERN at `source` and again at `copy`, with a byte of its own behind either, so that the
    match is the pattern's 24 bytes and no more. The zeros take one entry of the match finder's table, so that nothing
    between the two displaces the source's; a block of zeros alone is an RLE block, and in a block that holds the
    pattern the zeros in front of it are one match at offset 1 that ends where the pattern begins."""
    out = bytearray(n)
    for at, stop in ((source, 250), (copy, 251)):
        out[at:at + len(PATTERN) + 1] = PATTERN + bytes((stop,))
    return bytes(out)


# name: (length, where the pattern lies, where it lies again). Block k begins at k * BLOCK, and with window log 17 its
# history begins at (k - 1) * BLOCK.
EDGES = {
    "edge-far": (3 * BLOCK, BLOCK, 2 * BLOCK + 1000),             # the source begins the history of the last block at 17
    "edge-beyond": (3 * BLOCK, BLOCK - 1, 2 * BLOCK + 1000),      # ... and one byte in front of it: 23 bytes match at 17
    "edge-cross": (2 * BLOCK, BLOCK - 3, BLOCK + 30),             # from the last three history bytes into the block
    "edge-off131072": (2 * BLOCK, 5000, BLOCK + 5000),            # offset 131 072 exactly
    "edge-code19": (4 * BLOCK + 4096, 100, 4 * BLOCK + 150),      # offset (1 << 19) + 50: offset code 19, window 19 only
}
FAR = ("dup200000x3", "text-1048576")
TAIL = ("text-131074",)  # a last block of two bytes behind its history: its last history positions hash past its end


def content_of(name):
    if name in EDGES:
        return _edge(*EDGES[name])
    if name == "dup200000x3":
        import numpy as np
        return np.random.default_rng(5).integers(0, 256, size=200_000, dtype=np.uint8).tobytes() * 3
    return ti.content_of(name)


def case_names():
    return list(ti.case_names()) + list(FAR) + list(EDGES) + list(TAIL)


# what tests/test_gpu_zstd_encode_window.py encodes on the device
GPU_SUBSET = ("text-131073", "text-300000", "period70000-300000", "mixed-1048576", "dup200000x3") + tuple(EDGES) + TAIL

_cache = {}


def cases():
    """[(name, content)], computed once, shared, not to be changed; zstd_enc_tables_inputs.cases() first, as they are"""
    if "cases" not in _cache:
        base = ti.cases()
        _cache["cases"] = list(base) + [(name, content_of(name)) for name in case_names()[len(base):]]
    return _cache["cases"]


def run_native():
    """builds tests/native/test_zstd_encode_window.cpp with g++ under ASan + UBSan and runs it over every case in every
    mode, once per process: (return code, stdout, stderr, {mode: [frame]}, {mode: [[frame length, coverage, literals and
    sequences of the last block]]}) with the modes of MODES as keys"""
    if "run" in _cache:
        return _cache["run"]
    tmp = tempfile.mkdtemp(prefix="zstd_encode_window")
    path, fpath, rpath, exe = (os.path.join(tmp, n) for n in ("cases.bin", "frames.bin", "results.txt", "test_zstd_encode_window"))
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases())))
        for name, data in cases():
            f.write(struct.pack("<I", len(name)) + name.encode() + struct.pack("<Q", len(data)) + data)
    flags = ["-std=c++17", "-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
             "-Wall", "-Wextra"]
    subprocess.run(["g++", *flags, os.path.join(ROOT, "tests", "native", "test_zstd_encode_window.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    p = subprocess.run([exe, path, fpath, rpath], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=1800)
    frames, rows = {m: [] for m in MODES}, {m: [] for m in MODES}
    if os.path.exists(fpath):
        blob = open(fpath, "rb").read()
        at = k = 0
        while at < len(blob):
            (n,) = struct.unpack_from("<Q", blob, at)
            frames[MODES[k % len(MODES)]].append(blob[at + 8:at + 8 + n])
            at += 8 + n
            k += 1
        for ln in open(rpath):
            v = [int(x, 0) for x in ln.split()]
            rows[(v[1], v[2])].append(v[3:])
    _cache["run"] = (p.returncode, p.stdout, p.stderr, frames, rows)
    return _cache["run"]


def golden():
    """{name: {"w17-t0": [frame length, SHA-256 of the frame in hex], ...}} of the four window modes"""
    if "golden" not in _cache:
        _cache["golden"] = json.load(open(GOLDEN))
    return _cache["golden"]
