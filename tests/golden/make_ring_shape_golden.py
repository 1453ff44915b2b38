"""What the library reports for a dozen page rings, as a flat text fixture (tests/golden/ring_shape_v1.txt).

Only the public API: the script runs unchanged on any build of the library, and the fixture in the tree was written by the
build of the commit named in its first line. tests/native/test_ring_plan.cpp requires pbs_plus_amd/csrc/ring_plan.h to give
the recorded values for the recorded inputs, tests/test_gpu_ring_shape.py requires them of the rings themselves.

One case per line, integers only, the inputs first (COLUMNS). Every ring has an explicit small arena, so that a creation
takes a few milliseconds.

    python tests/golden/make_ring_shape_golden.py --commit <short hash> [--out tests/golden/ring_shape_v1.txt]
"""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OFF = 0xFFFFFFFF
INPUTS = ("num_cus", "avg", "min", "max", "mask", "arena_bytes", "page_bytes", "max_streams", "sha_cus", "round_pages",
          "express_cus", "min_round_pages", "max_inflight", "long_bytes", "flags", "lanes_cus", "backlog_mib", "short_bytes")
OUTPUTS = ("got_page_bytes", "got_pages_total", "got_sha_cus", "got_express_cus", "got_long_bytes", "got_backlog_limit",
           "got_lanes_cus", "got_short_bytes")
COLUMNS = INPUTS + OUTPUTS
OPTION_FIELDS = INPUTS[5:]

SMALL, LARGE, TINY = 64 << 10, 4 << 20, 256   # average chunk sizes: pages of 256 KiB, 16.2 MiB and 64 KiB
MIB = 1 << 20
CASES = [
    dict(avg=SMALL, arena_bytes=32 * MIB),                                             # the defaults
    dict(avg=SMALL, arena_bytes=32 * MIB, sha_cus=100),                                # pair CUs given: no express service
    dict(avg=SMALL, arena_bytes=32 * MIB, sha_cus=250),                                # ... beyond what the cut side leaves
    dict(avg=SMALL, arena_bytes=32 * MIB, sha_cus=64, express_cus=24),                 # express on top of a given share
    dict(avg=SMALL, arena_bytes=32 * MIB, express_cus=OFF),
    dict(avg=SMALL, arena_bytes=32 * MIB, express_cus=1000),                           # at most half the chip
    dict(avg=SMALL, arena_bytes=32 * MIB, lanes_cus=32),                               # short_bytes = 3/2 of the average
    dict(avg=SMALL, arena_bytes=32 * MIB, lanes_cus=32, short_bytes=50000),
    dict(avg=SMALL, arena_bytes=32 * MIB, lanes_cus=1000, short_bytes=1 << 30),        # both clamped
    dict(avg=SMALL, arena_bytes=32 * MIB, long_bytes=OFF),                             # no long queue: no express service
    dict(avg=SMALL, arena_bytes=32 * MIB, long_bytes=100000),
    dict(avg=SMALL, arena_bytes=32 * MIB, round_pages=100000, min_round_pages=100000, max_inflight=100),
    dict(avg=SMALL, arena_bytes=32 * MIB, round_pages=2, min_round_pages=1, max_inflight=1),
    dict(avg=SMALL, arena_bytes=32 * MIB, backlog_mib=-1),
    dict(avg=SMALL, arena_bytes=32 * MIB, backlog_mib=37),
    dict(avg=SMALL, arena_bytes=24 * MIB, page_bytes=512 << 10, max_streams=4, flags=8),  # pages of two chunks, split fixed
    dict(avg=LARGE, arena_bytes=5 * (16990208 + 256)),                                 # five pages of 61 large tiles
    dict(avg=TINY, arena_bytes=4 * MIB),                                               # min 64 < effmin 65
]


def num_cus() -> int:
    """the CU count of device 0, asked of the HIP runtime the library itself has loaded (no second runtime in the process)"""
    import ctypes as C

    from pbs_plus_amd import _lib

    _lib.lib()
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    if len(paths) > 1:  # (a Python package imported after the library has brought a runtime of its own: not that one)
        paths = {p for p in paths if "-packages/" not in p}
    assert len(paths) == 1, paths
    hip = C.CDLL(paths.pop())
    n = C.c_int(0)
    multiprocessor_count = 63  # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h)
    assert hip.hipDeviceGetAttribute(C.byref(n), multiprocessor_count, 0) == 0
    assert 0 < n.value <= 4096, n.value
    return n.value


def report(engines: dict, case: dict, cus: int) -> dict:
    """the full row of one case: its inputs (missing options are 0) and what a ring created from them reports"""
    from pbs_plus_amd import Engine, PageRing, buzhash

    avg = case["avg"]
    if avg not in engines:
        engines[avg] = Engine(buzhash.NewConfig(avg), device=0, inflight=1)
    cfg = buzhash.NewConfig(avg)
    row = dict(num_cus=cus, avg=avg, min=cfg.MinSize, max=cfg.MaxSize, mask=cfg.BreakTestMask)
    for k in OPTION_FIELDS:
        row[k] = int(case.get(k, 0))
    opts = {k: row[k] for k in OPTION_FIELDS}
    opts["backlog_mib"] = float(opts["backlog_mib"])
    ring = PageRing(engines[avg], **opts)
    try:
        st, (xcus, xfrom), text = ring.stats(), ring.express(), ring.debug()
    finally:
        ring.close()
    lanes = re.search(r"lanes service: cus=(\d+) short_bytes=(\d+)", text)
    row.update(got_page_bytes=st["page_bytes"], got_pages_total=st["pages_total"], got_sha_cus=st["sha_cus"],
               got_express_cus=xcus, got_long_bytes=xfrom,
               got_backlog_limit=int(re.search(r"backlog_limit=(\d+)", text).group(1)),
               got_lanes_cus=int(lanes.group(1)), got_short_bytes=int(lanes.group(2)))
    return row


def read_fixture(path: str) -> list:
    rows = []
    with open(path) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            rows.append(dict(zip(COLUMNS, (int(v) for v in line.split()))))
    return rows


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose build is loaded (first line of the fixture)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ring_shape_v1.txt"))
    a = ap.parse_args()
    for k in os.environ:
        assert not k.startswith("PBSGPU_RING_"), f"{k} would override the options"
    cus, engines = num_cus(), {}
    lines = [f"# ring shapes reported by the build of commit {a.commit} on a device with {cus} CUs", "# " + " ".join(COLUMNS)]
    for case in CASES:
        row = report(engines, case, cus)
        lines.append(" ".join(str(row[k]) for k in COLUMNS))
    for e in engines.values():
        e.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{len(CASES)} cases -> {a.out}")


if __name__ == "__main__":
    main()
