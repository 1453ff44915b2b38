"""The shape of a page ring as the library reports it — page size and count, the pair / express / lanes CU split, the long
and short thresholds, the backlog gate — for the rings of tests/golden/ring_shape_v1.txt: the same options must give what
the build named in the fixture's first line gave (tests/golden/make_ring_shape_golden.py wrote it and creates the rings
here). The rules themselves are pbs_plus_amd/csrc/ring_plan.h; tests/test_ring_plan_native.py checks them against the same
fixture without a device. Every ring has a small explicit arena and carries no stream: the file runs in a few seconds."""
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_ring_shape_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu


def test_rings_report_the_recorded_shapes(gpu_lib, monkeypatch):
    for k in list(os.environ):
        if k.startswith("PBSGPU_RING_") and k != "PBSGPU_RING_IDLE_TIMEOUT_S":
            monkeypatch.delenv(k)  # (debug overrides of the options under test)
    want = G.read_fixture(os.path.join(GOLDEN, "ring_shape_v1.txt"))
    assert len(want) == len(G.CASES) >= 12
    cus = G.num_cus()
    if cus != want[0]["num_cus"]:
        pytest.skip(f"the fixture was recorded on a device with {want[0]['num_cus']} CUs, this one has {cus}")
    engines = {}
    try:
        for case, row in zip(G.CASES, want):
            got = G.report(engines, case, cus)
            assert got == row, (case, {k: (got[k], row[k]) for k in G.COLUMNS if got[k] != row[k]})
    finally:
        for e in engines.values():
            e.close()
