"""The oracle at every chunker configuration NewConfig accepts (avg = 2^8 .. 2^28), on the CPU.

tests/test_oracle_buzhash.py pins the oracle's fields at 4 MiB and its break test by a vector at 64 KiB; the GPU suite compares
against the oracle at every average (tests/test_gpu_config_range.py), so the oracle itself is pinned here at each of them:
  * the binding's and the oracle's NewConfig fields against the formula (min = avg/4, max = 4 avg, mask = 2 avg - 1,
    break_min = mask - 2);
  * the oracle's candidate list against a vectorised numpy restatement of the 64-byte window hash
    (config_inputs.candidates_model), and its cut list against helpers.resolve_model and against the PLANNED cut list of
    tests/config_inputs.py (a content cut at exactly effmin behind an ignored candidate at effmin - 1, content cuts at random
    distances, a final chunk below the minimum; forced cuts at max and a candidate at max up to avg 1 MiB, where max-size
    chunks stay small), plus the 0-byte and the 1-byte stream.
"""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import config_inputs as CI  # noqa: E402
from dense_inputs import window_hash  # noqa: E402
from helpers import resolve_model  # noqa: E402


@pytest.mark.parametrize("avg", CI.AVGS, ids=lambda a: f"avg{a}")
def test_newconfig_fields_follow_the_formula(O, avg):
    from pbs_plus_amd import buzhash

    want = CI.expected_config(avg)
    o = O.new_config(avg)
    assert dict(avg=o.avg, min=o.min, max=o.max, window=o.window, mask=o.mask, break_min=o.break_min) == want
    c = buzhash.NewConfig(avg)
    assert dict(avg=c.AvgSize, min=c.MinSize, max=c.MaxSize, window=c.WindowSize, mask=c.BreakTestMask,
                break_min=c.BreakTestMinimum) == want
    assert np.array_equal(c.Table, O.default_table())
    bits = want["mask"].bit_length()
    assert want["mask"] == (1 << bits) - 1 and 9 <= bits <= 29


def test_window_hash_restatement_matches_the_scalar_one(O):
    """the six-pass window hash equals dense_inputs.window_hash (the oracle's recurrence written out) at sampled ends,
    across block borders"""
    T = O.default_table()
    data = np.random.default_rng(9).integers(0, 256, 3000, dtype=np.uint8)
    h = CI.window_hashes(T, data, block=1000)
    assert h.size == data.size - 63
    for e in list(range(64, 200)) + list(range(990, 1130)) + [2063, 2064, 2065, 3000]:
        assert int(h[e - 64]) == window_hash(T, data[e - 64:e]), e


@pytest.mark.parametrize("avg", CI.AVGS, ids=lambda a: f"avg{a}")
def test_oracle_candidates_and_cuts_on_planned_streams(O, avg):
    cfg, data, ends = CI.plan_stream(O, avg, seed=avg % 997 + 11, full=avg <= (1 << 20), target=2 << 20)
    em, mn, mx = max(int(cfg.min), 65), int(cfg.min), int(cfg.max)
    cand = O.candidates(cfg, data)
    assert np.array_equal(cand, CI.candidates_model(cfg, data)), avg
    cuts = O.chunk_stream(cfg, data)
    assert np.array_equal(cuts, ends)
    assert np.array_equal(resolve_model(cand, data.size, mn, mx), ends)
    # the plan holds what it claims: a cut at exactly effmin behind a candidate at effmin - 1, a final chunk below the minimum
    sizes = np.diff(np.concatenate([[0], ends.astype(np.int64)]))
    starts = ends.astype(np.int64) - sizes
    cset = set(int(x) for x in cand)
    assert any(sz == em and int(s) + em - 1 in cset for s, sz in zip(starts, sizes))
    assert 0 < sizes[-1] < mn
    if avg <= (1 << 20):
        assert any(sz == mx and not any(int(s) < c <= int(s) + mx for c in cset) for s, sz in zip(starts[:-1], sizes[:-1]))
        assert any(sz == mx and int(s) + mx in cset for s, sz in zip(starts, sizes))
    rec = O.chunk_and_digest(cfg, data, [(0, data.size)])
    assert np.array_equal(rec["end"], ends) and np.array_equal(rec["size"].astype(np.int64), sizes)
    for s, e, dg in list(zip(starts, ends.astype(np.int64), rec["digest"]))[-4:]:
        assert bytes(dg) == hashlib.sha256(data[s:e].tobytes()).digest()
    for tiny in CI.tiny_streams(O, avg, seed=avg % 997):
        assert O.candidates(cfg, tiny).size == 0
        assert list(O.chunk_stream(cfg, tiny)) == ([tiny.size] if tiny.size else [])
