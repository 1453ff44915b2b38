"""The held-page bookkeeping (pbs_plus_amd/csrc/hold.h) as the engine's ring uses it for payload streams that hold their
pages beside streams that do not (pbsgpu_stream_hold), as a CPU program under AddressSanitizer + UBSan: a
stand-alone program with its own main (tests/native/test_hold_streams.cpp), nothing loaded into Python, nothing preloaded.
The program drives holding and non-holding streams interleaved against a model: a non-holder's page is freed by its
hand-back, alone and so in hand-back order; the predicate "a page can become free without a release" is true exactly
when the model finds such a page; a stream closed late returns every page once."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_holders_beside_non_holders_equal_the_model_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_hold_streams")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra"]
    subprocess.run(["g++", *flags, os.path.join(ROOT, "tests", "native", "test_hold_streams.cpp"), "-o", exe], check=True,
                   timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "hold-streams-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
