"""What the zstd tests share: the golden cases of tests/golden/zstd_v1*.npz with their regenerated content, the seeded
mutations of tests/native/test_zstd_core.cpp, and the three mutated and three truncated frames that the GPU test takes from that program's run
(tests/test_zstd_core_native.py checks that the run reports for them exactly what is recorded here)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = (1 << 64) - 1
OK, BAD_FRAME, BAD_SIZE, UNSUPPORTED = range(4)

# (case, byte position, xor value, status, bytes decoded, CRC-32 of them): single-byte mutations of the sanitizer run
MUTATIONS = (("text-60000-level1", 8475, 195, BAD_FRAME, 0, 0),
             ("text-60000-level1", 4312, 200, BAD_SIZE, 0, 0),
             ("text-60000-level1", 1851, 114, OK, 60000, 1109016140))

# (case, length, status): truncations of a compressed fixture from the same run, ending inside a Huffman stream or the
# sequences of a block
CUTS = (("text-60000-level1", 118, BAD_FRAME), ("text-60000-level1", 8033, BAD_FRAME), ("text-60000-level1", 15548, BAD_FRAME))

_cache = {}


def golden():
    """tests/golden/make_zstd_golden.py as a module (it needs libzstd only to write the files)"""
    if "golden" not in _cache:
        spec = importlib.util.spec_from_file_location("make_zstd_golden", os.path.join(ROOT, "tests", "golden", "make_zstd_golden.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _cache["golden"] = mod
    return _cache["golden"]


def cases():
    """every golden case, with its content under "content": computed once, shared, not to be changed"""
    if "cases" not in _cache:
        g = golden()
        out = g.load()
        for c in out:
            c["content"] = g.content_of(c["name"], c["length"])
        _cache["cases"] = out
    return _cache["cases"]


def splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def mutation(ci, j, n):
    """(position, xor value) of mutation j of case ci, whose frame has n bytes: the program's formula"""
    r = splitmix(((ci << 32) + j + 77) & MASK)
    return r % n, 1 + (r >> 32) % 255


def mutated(frame, at, xor):
    return frame[:at] + bytes([frame[at] ^ xor]) + frame[at + 1:]
