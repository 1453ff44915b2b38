"""aes_gcm.h (pbs_plus_amd/csrc) as a CPU program under AddressSanitizer + UBSan: a stand-alone program with its own main
(tests/native/test_aes_gcm.cpp), nothing loaded into Python, nothing preloaded. The golden cases of
tests/golden/aes_gcm_v1.json (libcrypto's answers, the zero-key known answer among them); IV lengths 8, 12, 16 and 60 at
every length of 0-49 bytes; pieces + fold against the serial GHASH chain for 1, 2, 3 and 5 pieces with odd tails and for
every split of a short chain; H^n against repeated multiplication; the inc32 wrap; every single-bit flip of a 33-byte
message's ciphertext, tag and IV; guard bytes around every output; and a branch-coverage word."""
import os
import subprocess
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aes_inputs as ai  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one bit per branch, in the order of the enum in aes_gcm.h
BRANCHES = ("iv_12 iv_blocks iv_part block_full block_part lane_idle lane_one lane_many lane_at_end lane_moved ctr_wrap "
            "pow_bit_set pow_bit_clear empty tag_good tag_bad encrypt decrypt").split()


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """builds and runs the program once: (exit code, stdout, stderr, {section: (verdict, count)})"""
    tmp = tmp_path_factory.mktemp("aes_gcm")
    path = str(tmp / "cases.txt")
    with open(path, "w") as f:
        for c in ai.golden():
            f.write("%s %s %d %d %s %d\n" % (c["key"].hex(), c["iv"].hex() or "-", c["length"], c["seed"], c["tag"].hex(), c["crc"]))
    exe = str(tmp / "test_aes_gcm")
    flags = ["-std=c++17", "-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
             "-Wall", "-Wextra"]
    subprocess.run(["g++", *flags, os.path.join(ROOT, "tests", "native", "test_aes_gcm.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    p = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=600)
    sections = {}
    for ln in p.stdout.splitlines():
        w = ln.split()
        if len(w) == 3 and w[1] in ("ok", "FAIL"):
            sections[w[0]] = (w[1], int(w[2]))
    return p.returncode, p.stdout, p.stderr, sections


def test_the_program_ends_clean_under_the_sanitizers(run):
    code, so, se, sections = run
    assert code == 0 and "aes-gcm-ok" in so, so[-4000:] + se[-4000:]
    assert "runtime error" not in se and "AddressSanitizer" not in se
    assert all(v == "ok" for v, _ in sections.values()), sections


def test_the_golden_cases_and_the_counter_wraps(run):
    sections = run[3]
    assert sections["golden"] == ("ok", len(ai.golden()))
    assert sections["golden-wraps"] == ("ok", 4)  # first piece, piece boundary, third piece, and J0 = ...FFFFFFFE
    names = [c["name"] for c in ai.golden()]
    assert names == [c[0] for c in ai.cases()]  # the file is what the generator would write today
    zero = ai.golden()[0]
    assert zero["key"] == bytes(32) and zero["iv"] == bytes(12) and zero["tag"].hex() == "d0d1c8a799996bf0265b98b5d48ab919"
    assert zero["crc"] == zlib.crc32(bytes.fromhex("cea7403d4d606b6e074ec5d3baf39d18"))
    assert os.path.getsize(ai.GOLDEN) < 16 << 10


def test_lengths_pieces_splits_powers_and_flips(run):
    sections = run[3]
    assert sections["lengths"] == ("ok", 4 * 50)
    assert sections["pieces"] == ("ok", 6)
    assert sections["splits"] == ("ok", 24 * 25 // 2)  # every 0 <= a <= b <= 23
    assert sections["powers"][0] == "ok" and sections["powers"][1] >= 601 + 12 + 300
    assert sections["flips"] == ("ok", (33 + 16 + 16) * 8)


def test_every_branch_is_reached(run):
    so = run[1]
    word = [ln for ln in so.splitlines() if ln.startswith("coverage ")][0].split()
    assert int(word[3]) == len(BRANCHES)
    missing = [b for i, b in enumerate(BRANCHES) if not int(word[1], 16) >> i & 1]
    assert not missing, missing


def test_the_python_gcm_agrees_with_the_recorded_cases_and_with_libcrypto():
    """the pure-Python GCM (short cases), the file, and libcrypto where it loads (every case) tell one story"""
    for c in ai.golden():
        plain = ai.pattern(c["length"], c["seed"])
        if c["length"] <= 64:
            ct, tag = ai.gcm_encrypt(c["key"], c["iv"], plain)
            assert tag == c["tag"] and zlib.crc32(ct) == c["crc"], c["name"]
        if ai.libcrypto() is not None:
            ct, tag = ai.libcrypto_encrypt(c["key"], c["iv"], plain)
            assert tag == c["tag"] and zlib.crc32(ct) == c["crc"], c["name"]
    k = ai.key_of(3)
    assert ai.j0_of(k, ai.wrap_iv(k, 1, 4)) & 0xFFFFFFFF == 0xFFFFFFFE
