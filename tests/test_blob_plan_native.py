"""The host plans of the aux calls (pbs_plus_amd/csrc/blob_plan.h) as a CPU program under AddressSanitizer + UBSan: a
stand-alone program with its own main (tests/native/test_blob_plan.cpp), nothing loaded into Python, nothing preloaded.
The program checks the piece table (lengths at the piece's edges, no ranges, 2^32 - 1 and 2^32 pieces), the restore plan
(one blob behind many entries, ranges that cut entries, blobs with no byte in the range, an empty range, blobs by
position, lengths of 12 bytes and fewer, and for zstd direct placement exactly when the first entry in range is whole and
the largest) and the packed blocks, whose offsets must equal the expressions they replaced, written out literally."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_host_plans_hold_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_blob_plan")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra"]
    subprocess.run(["g++", *flags, os.path.join(ROOT, "tests", "native", "test_blob_plan.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "blob-plan-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
