"""The page ring's host-side decisions (pbs_plus_amd/csrc/ring_plan.h: the shape of a ring, the pair / express split, the
round's gate, size, deferral and cut-side partition, the queue policy) as a CPU program under AddressSanitizer + UBSan: a
stand-alone program with its own main (tests/native/test_ring_plan.cpp), nothing loaded into Python, nothing preloaded.
The program checks the values the project's documents state, invariants over a seeded sweep of options, and the shapes
that the parent commit's build reported on the device (tests/golden/ring_shape_v1.txt)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ring_plan_stated_values_invariants_and_parent_shapes_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_ring_plan")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra"]
    subprocess.run(["g++", *flags, os.path.join(ROOT, "tests", "native", "test_ring_plan.cpp"), "-o", exe], check=True,
                   timeout=300)
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "ring_shape_v1.txt")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "ring-plan-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
