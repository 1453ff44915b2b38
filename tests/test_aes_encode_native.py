"""What pbsgpu_blob_encode3_device rests on, as a CPU program under AddressSanitizer + UBSan: a stand-alone program with its
own main (tests/native/test_aes_encode.cpp), nothing loaded into Python, nothing preloaded. aes_gcm.h's piece walk run in
place (in == out: how the device encrypts a frame where it lies) against the run with two buffers and against the serial
definition, at the lengths the GPU test runs; and blob_plan.h's additions: the slot offsets for both header sizes, the piece
table for the slots' capacities against a loop by the definition, the duplicate-IV check, the statistics."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1, 15, 16, 17, 4095, 65535, 65536, 65537, 3 * 65536 + 5)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """builds and runs the program once: (exit code, stdout, stderr, {section: (verdict, count)})"""
    exe = str(tmp_path_factory.mktemp("aes_encode") / "test_aes_encode")
    flags = ["-std=c++17", "-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
             "-Wall", "-Wextra"]
    subprocess.run(["g++", *flags, os.path.join(ROOT, "tests", "native", "test_aes_encode.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    sections = {}
    for ln in p.stdout.splitlines():
        w = ln.split()
        if len(w) == 3 and w[1] in ("ok", "FAIL"):
            sections[w[0]] = (w[1], int(w[2]))
    return p.returncode, p.stdout, p.stderr, sections


def test_the_program_ends_clean_under_the_sanitizers(run):
    code, so, se, sections = run
    assert code == 0 and "aes-encode-ok" in so, so[-4000:] + se[-4000:]
    assert "runtime error" not in se and "AddressSanitizer" not in se
    assert set(sections) == {"in-place", "offsets", "pieces", "ivs", "stats"}
    assert all(v == "ok" for v, _ in sections.values()), sections


def test_ctr_in_place_equals_two_buffers_and_the_serial_definition(run):
    assert run[3]["in-place"] == ("ok", len(LENGTHS))
    src = open(os.path.join(ROOT, "tests", "native", "test_aes_encode.cpp")).read()
    assert "{1, 15, 16, 17, 4095, 65535, 65536, 65537, 3 * 65536 + 5}" in src  # the lengths above are the program's
    assert "same.p(), same.p()" in src


def test_the_plan_additions(run):
    sections = run[3]
    assert sections["offsets"] == ("ok", 2 * 13 + 4)  # thirteen chunks under both header sizes, and the sums that wrap
    assert sections["pieces"][0] == "ok" and sections["pieces"][1] >= 10 * 5
    assert sections["ivs"] == ("ok", 2 + 5 * 5 + 2)
    assert sections["stats"] == ("ok", 5)
