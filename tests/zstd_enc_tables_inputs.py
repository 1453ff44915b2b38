"""What the tests of the zstd encoder's second mode share (per-block sequence tables and repeat codes,
pbsgpu_engine_options.zstd_seq_tables = 1): every case of zstd_enc_inputs plus contents crafted for the repeat codes and
the table modes, one build and run of tests/native/test_zstd_encode_tables.cpp per process, and the golden file."""
import json
import os
import struct
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_enc_inputs as zi  # noqa: E402

ROOT = zi.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "zstd_enc_tables_v1.json")

# the bits the second mode adds, behind zi.BRANCHES, in the order of the enum in zstd_encode.h
BRANCHES = zi.BRANCHES + ("ll_predef ll_rle ll_fse of_predef of_rle of_fse ml_predef ml_rle ml_fse rep_1 rep_2 rep_3 rep0_1 rep0_2 "
                          "rep0_3 rep_unknown ll_log_max of_log_max ml_log_max").split()
NEW = BRANCHES[len(zi.BRANCHES):]
UNREACHED = zi.UNREACHED  # every new bit is reached
REPEAT_CASES = ("records-20000", "reps-20000", "touch-20000", "touch-131072", "touch-131073", "touch-300000")
SHORTER = ("text-131072", "text-300000", "text10-300000", "mixed-300000", "four-2000") + REPEAT_CASES


def _fresh(i):
    """three bytes above 127 that occur once: the separators between matches"""
    return bytes((128 + i % 40, 168 + i // 40 % 40, 208 + i // 1600 % 40))


def _records(n):
    """fixed-stride records of five fields of eight bytes behind a separator each: three fields are the same in every
    record, one alternates between two values and one goes round three, so that a record's matches lie at one, one, two,
    one and three strides and every one of them is a repeat of one of the three offsets before it"""
    import numpy as np
    rng = np.random.default_rng(31)
    val = lambda: bytes(rng.integers(0, 120, size=8, dtype=np.uint8))  # noqa: E731
    a, b, c = val(), val(), val()
    two, three = [val(), val()], [val(), val(), val()]
    out, k = bytearray(), 0
    while len(out) < n:
        for j, f in enumerate((a, b, two[k % 2], c, three[k % 3])):
            out += _fresh(5 * k + j) + f
        k += 1
    return bytes(out[:n])


def _unit(pattern, start, nrec, zones):
    """One unit of matches at chosen offsets: a head of bytes without a repeat, then `nrec` records. A record is a list of
    (zone, shift, touching): eight bytes copied from `offset(zone) - shift` back, behind a separator unless `touching`.
    Zone z's sources lie in their own part of the head and move along with the output, so every copy of a zone has the
    same offset, no source is copied twice, and the copy is the only earlier occurrence of its bytes."""
    reclen = sum(8 + (0 if t else 3) for _, _, t in pattern) + 3
    lz = nrec * reclen
    lz += (1 - lz) % 3  # not a multiple of 3: the byte behind a source differs from the first byte of the next zone's
    p0 = zones * lz + 9
    out = bytearray(zi._unique(p0, start))
    sep = start
    for _ in range(nrec):
        for z, shift, touching in pattern:
            if not touching:
                out += _fresh(sep)
                sep += 1
            q = len(out) - (p0 - z * lz) + shift
            out += out[q:q + 8]
        out += _fresh(sep)  # (the source behind a shifted copy is left out by the next one)
        sep += 1
    return bytes(out), p0, lz


def _units(n, pattern, nrec, zones):
    out, start = bytearray(), 0
    while len(out) < n:
        u, _, _ = _unit(pattern, start, nrec, zones)
        out += u
        start += len(u)  # a head of its own for every unit
    return bytes(out[:n])


# matches behind literals at offsets 1 1 2 1 3 (zones): the repeat codes 2 1 3 2 3 once the three are known
REPS = ((0, 0, False), (0, 0, False), (1, 0, False), (0, 0, False), (2, 0, False))
# matches that touch: offsets 1 | 2 1 3 2 and the second zone's offset less one: behind no literals the codes 1 1 2 2 3
TOUCH = ((0, 0, False), (1, 0, True), (0, 0, True), (2, 0, True), (1, 0, True), (1, 1, True))


def _ofrle():
    """sixteen matches at four offsets in turn, all of them between 1024 and 2047 - 3: no offset repeats one of the three
    before it, and every offset code is 10"""
    head = 1900
    out = bytearray(zi._unique(head))
    for k in range(16):
        out += _fresh(k)
        q = len(out) - (head - (k % 4) * 178)
        out += out[q:q + 8]
    return bytes(out)


def _llrle():
    """every sequence with 16 or 17 literals, the first one too: literal length code 16 only"""
    out = bytearray(zi._unique(17))
    for k in range(40):
        out += out[len(out) - 12:len(out) - 4]  # eight bytes of the run before, which nothing has copied yet
        out += zi._unique(16, 100 + 10 * k)
    return bytes(out)


def content_of(name):
    kind, _, arg = name.partition("-")
    n = int(arg) if arg else 0
    if kind == "records":
        return _records(n)
    if kind == "reps":
        return _units(n, REPS, 12, 3)
    if kind == "touch":
        return _units(n, TOUCH, 12, 3)
    if kind == "ofrle":
        return _ofrle()
    if kind == "llrle":
        return _llrle()
    return zi.content_of(name)


def case_names():
    return list(zi.case_names()) + ["records-20000", "reps-20000", "touch-20000", "touch-131072", "touch-131073", "touch-300000",
                                    "ofrle", "llrle", "seqs-1", "seqs-2"]


_cache = {}


def cases():
    """[(name, content)], computed once, shared, not to be changed; zstd_enc_inputs.cases() first, as they are"""
    if "cases" not in _cache:
        base = zi.cases()
        _cache["cases"] = list(base) + [(name, content_of(name)) for name in case_names()[len(base):]]
    return _cache["cases"]


def run_native():
    """builds tests/native/test_zstd_encode_tables.cpp with g++ under ASan + UBSan and runs it over every case in both modes,
    once per process: (return code, stdout, stderr, {mode: [frame]}, {mode: [[frame length, coverage, literals, sequences]]})"""
    if "run" in _cache:
        return _cache["run"]
    tmp = tempfile.mkdtemp(prefix="zstd_encode_tables")
    path, fpath, rpath, exe = (os.path.join(tmp, n) for n in ("cases.bin", "frames.bin", "results.txt", "test_zstd_encode_tables"))
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases())))
        for name, data in cases():
            f.write(struct.pack("<I", len(name)) + name.encode() + struct.pack("<Q", len(data)) + data)
    flags = ["-std=c++17", "-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
             "-Wall", "-Wextra"]
    subprocess.run(["g++", *flags, os.path.join(ROOT, "tests", "native", "test_zstd_encode_tables.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    p = subprocess.run([exe, path, fpath, rpath], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=900)
    frames, rows = {0: [], 1: []}, {0: [], 1: []}
    if os.path.exists(fpath):
        blob = open(fpath, "rb").read()
        at = k = 0
        while at < len(blob):
            (n,) = struct.unpack_from("<Q", blob, at)
            frames[k & 1].append(blob[at + 8:at + 8 + n])
            at += 8 + n
            k += 1
        for ln in open(rpath):
            v = [int(x, 0) for x in ln.split()]
            rows[v[1]].append(v[2:])
    _cache["run"] = (p.returncode, p.stdout, p.stderr, frames, rows)
    return _cache["run"]


def golden():
    """{name: [frame length, SHA-256 of the frame in hex]} of mode 1"""
    if "golden" not in _cache:
        _cache["golden"] = json.load(open(GOLDEN))
    return _cache["golden"]
