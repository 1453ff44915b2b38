"""The tail of the keyed chunk digest SHA-256(content || id_key) on the CPU, under AddressSanitizer + UBSan: a stand-alone
program with its own main (tests/native/test_sha256_suffix.cpp), nothing loaded into Python, nothing preloaded. It includes
pbs_plus_amd/csrc/sha256_suffix.h, the one function the kernels build their keyed tail blocks with, assembles the data words the
way the kernels do, compares every tail block byte for byte with the padding of content || key built by the definition, and
prints the digests, which are compared here with hashlib for the same pattern and key."""
import hashlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = tuple(range(201)) + (4096, 65535, 65536, 65537)
KEY_SEED = 0x4B45


def pattern(n, seed):
    """tests/native/test_sha256_suffix.cpp: pattern_byte"""
    out = bytearray(n)
    for i in range(n):
        x = ((i + seed * 7919) * 2654435761) & 0xFFFFFFFF
        out[i] = ((x >> 24) ^ (x >> 9)) & 0xFF
    return bytes(out)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """builds and runs the program once: (exit code, stdout, stderr)"""
    exe = str(tmp_path_factory.mktemp("sha256_suffix") / "test_sha256_suffix")
    flags = ["-std=c++17", "-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
             "-Wall", "-Wextra"]
    subprocess.run(["g++", *flags, os.path.join(ROOT, "tests", "native", "test_sha256_suffix.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    return p.returncode, p.stdout, p.stderr


def test_the_program_ends_clean_under_the_sanitizers(run):
    code, so, se = run
    assert code == 0 and "sha256-suffix-ok" in so, so[-4000:] + se[-4000:]
    assert "runtime error" not in se and "AddressSanitizer" not in se


def test_every_tail_block_equals_the_definition(run):
    lines = [ln.split() for ln in run[1].splitlines() if ln.startswith("blocks ")]
    assert len(lines) == 1 and lines[0][1] == "ok", lines
    # every (length, alignment) has one or two tail blocks: two when (len % 64) + 32 + 9 > 64
    want = sum(4 * (2 if (n % 64) + 41 > 64 else 1) for n in LENGTHS)
    assert int(lines[0][2]) == want, (lines, want)


def test_the_digests_equal_hashlib(run):
    key = pattern(32, KEY_SEED)
    got = {}
    for ln in run[1].splitlines():
        w = ln.split()
        if len(w) == 4 and w[0] == "digest":
            got[(int(w[1]), int(w[2]))] = w[3]
    assert set(got) == {(n, a) for n in LENGTHS for a in range(4)}
    for n in LENGTHS:
        want = hashlib.sha256(pattern(n, n) + key).hexdigest()
        for a in range(4):
            assert got[(n, a)] == want, (n, a)
    # the keyed digest is not the plain one, and the empty chunk's is the digest of the key alone
    assert got[(0, 0)] == hashlib.sha256(key).hexdigest() != hashlib.sha256(b"").hexdigest()
