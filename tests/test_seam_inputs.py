"""The planted-cut builder of the page-ring seam tests (tests/seam_inputs.py) checked on the CPU: the serial chunker confirms
every planned cut list (build_stream asserts it; checked again here), and every cell of the seam grids is present for each
chunker the GPU test runs (tests/test_gpu_ring_seams.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seam_inputs as S  # noqa: E402

_PLANS = {}


@pytest.fixture(params=sorted(S.PAGES), ids=lambda a: f"avg{a}")
def planned(request, O):
    avg = request.param
    if avg not in _PLANS:
        _PLANS[avg] = S.plan(O, avg)
    return (avg,) + _PLANS[avg]


def test_plant_and_clear_are_exact(O):
    for avg in (256, 65536):
        cfg = O.new_config(avg)
        P = S.Planter(O, cfg, seed=3)
        data = np.random.default_rng(4).integers(0, 256, 200_000, dtype=np.uint8)
        P.clear(data)
        assert O.candidates(cfg, data).size == 0
        at = [68, 500, 777, 5000, 65536, 65600, 199_900, 200_000]          # (plants at least 68 bytes apart)
        for e in at:
            P.plant(data, e)
        assert list(O.candidates(cfg, data)) == at, avg


def test_the_oracle_confirms_every_planned_cut_list(O, planned):
    avg, cfg, page, streams = planned
    em = S.effmin(cfg)
    for data, ends in streams:
        assert np.array_equal(O.chunk_stream(cfg, data), ends)
        if data.size:
            assert int(ends[-1]) == data.size
            sizes = np.diff(np.concatenate([[0], ends.astype(np.int64)]))
            assert (sizes[:-1] >= em).all() and (sizes <= cfg.max).all()


def test_every_seam_grid_cell_is_present(O, planned):
    avg, cfg, page, streams = planned
    cross, near, onseam_then_more, tiny = set(), set(), 0, set()
    for data, ends in streams:
        c, _, n = S.census(ends, page)
        cross |= c
        near |= n
        onseam_then_more += sum(1 for e in ends[:-1] if int(e) % page == 0)
        if data.size < page:
            tiny.add(data.size)
    # SHA seam grid: len1 = 1..68 with a short and with a long second piece, all len1 residues mod 64
    for lo, hi in ((1, 8), (52, 72)):
        assert {l for l, p2, _, _ in cross if lo <= p2 <= hi} >= set(range(1, 69)), (avg, lo, hi)
    assert {l % 64 for l, _, _, _ in cross} == set(range(64))
    # every second piece at every chunk-start alignment; every chunk length mod 64
    for p2 in S.SHA_P2[1:]:
        assert {a for _, p, a, _ in cross if p == p2} == {0, 1, 2, 3}, (avg, p2)
    assert {m for _, _, _, m in cross} == set(range(64))
    # a block that starts in the last 15 bytes before the seam and reads 49+ bytes past it (the last third of the tail pad)
    assert {l for l, p2, _, _ in cross if p2 >= 52 and 1 <= l % 64 <= 15} >= set(range(1, 16))
    # a chunk ends exactly on a seam and the next one starts at the page start
    assert onseam_then_more >= 2
    # scan seam grid: ends at seam + 1..64 in a chunk that started in the previous page, at seam - 0..64
    assert near >= set(range(-64, 65)), sorted(set(range(-64, 65)) - near)
    # tiny final chunks
    assert tiny >= set(range(0, 131)) | {int(cfg.min) - 1, int(cfg.min), int(cfg.min) + 1}


def test_a_candidate_64_bytes_behind_a_cut_on_the_seam(O, planned):
    """the ring's head-pad argument (k_ring_prep_pages): no candidate of the first 64 bytes behind a cut can be accepted —
    at avg 256 (min 64) the candidate 64 bytes behind a seam cut is exactly at the minimum, and is present, and ignored"""
    avg, cfg, page, streams = planned
    hits = 0
    for data, ends in streams:
        cands = set(int(x) for x in O.candidates(cfg, data))
        es = set(int(x) for x in ends)
        for e in es:
            if e % page == 0 and e + 64 in cands:
                assert e + 64 not in es
                hits += 1
    assert hits >= 2
