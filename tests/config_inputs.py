"""Planned inputs for every chunker configuration NewConfig accepts (test infrastructure).

buzhash.NewConfig takes every power-of-two average from 2^8 to 2^28 bytes: min = avg / 4, max = 4 * avg (up to 1 GiB),
mask = 2 * avg - 1 (9 to 29 bits). The builder here lays out a stream whose serial cut list is PLANNED for any of them (the
candidates are planted and cleared with seam_inputs.Planter, the CPU oracle confirms the plan), so that every cut rule is
present at every average by construction:
  * "rand":  a content cut at a random distance in [effmin, max);
  * "pair":  a content cut at exactly effmin, with a candidate at effmin - 1 in front of it that the chunker must ignore;
  * "max":   a forced cut at exactly max, with no candidate anywhere in the chunk;
  * "atmax": a candidate exactly at max (the cut is the forced one, at the same offset);
and, at the stream's end, a final chunk shorter than the minimum. `full=False` leaves out the two max-size chunks (the CPU
restatement and the second stream of a ring run keep their size down that way).
"""
import numpy as np

from dense_inputs import _rotl
from seam_inputs import Planter, effmin

AVGS = [1 << k for k in range(8, 29)]


def expected_config(avg: int) -> dict:
    """NewConfig's fields restated from the formula"""
    return dict(avg=avg, min=avg // 4, max=avg * 4, window=64, mask=2 * avg - 1, break_min=2 * avg - 3)


def _span(cfg) -> int:
    """random content-cut distances lie in [effmin, effmin + span]: the whole range up to max at small averages, a few MiB
    at large ones (the stream's size is the time the GPU spends on it)"""
    return min(int(cfg.max) - 1 - effmin(cfg), 2 << 20)


def plan_stream(O, avg: int, seed: int, full: bool = True, target: int = 0, planter=None):
    """(cfg, bytes, planned chunk END offsets) of one stream: the pattern rand, pair, [max, atmax,] rand repeated until the
    stream holds at least `target` bytes (at least once), then a final chunk of 1 .. min - 1 bytes."""
    cfg = O.new_config(avg)
    em, mn, mx = effmin(cfg), int(cfg.min), int(cfg.max)
    rng = np.random.default_rng(seed)
    P = planter or Planter(O, cfg, seed)
    pattern = ["rand", "pair"] + (["max", "atmax"] if full else []) + ["rand"]
    ends, plants, pairs = [], [], []
    pos = 0
    while True:
        for kind in pattern:
            if kind == "rand":
                pos += int(rng.integers(em, em + _span(cfg) + 1))
                plants.append(pos)
            elif kind == "pair":
                pos += em
                pairs.append(pos)
            elif kind == "max":
                pos += mx
            else:
                pos += mx
                plants.append(pos)
            ends.append(pos)
        if pos >= target:
            break
    pos += int(rng.integers(1, mn))
    ends.append(pos)
    data = rng.integers(0, 256, pos, dtype=np.uint8)
    P.clear(data)
    for e in sorted(plants + pairs):
        P.plant(data, e, pair=e in pairs)
    want_c = sorted(plants + pairs + [e - 1 for e in pairs])
    assert list(O.candidates(cfg, data)) == want_c, "the planted candidates are not the stream's candidates"
    got = O.chunk_stream(cfg, data)
    assert list(got) == ends, "the serial chunker does not confirm the plan"
    return cfg, data, np.asarray(ends, dtype=np.uint64)


def tiny_streams(O, avg: int, seed: int):
    """the 0-byte and the 1-byte stream: no chunk, one chunk"""
    rng = np.random.default_rng(seed)
    return [np.zeros(0, dtype=np.uint8), rng.integers(0, 256, 1, dtype=np.uint8)]


def window_hashes(table, data: np.ndarray, block: int = 8 << 20) -> np.ndarray:
    """h(e) for every window END e = 64 .. n (index e - 64), vectorised: H_1(i) = T[b_i] and
    H_2L(i) = H_L(i) ^ rotl(H_L(i - L), L), so H_64(i) = XOR_k rotl(T[b[i - k]], k mod 32) — dense_inputs.window_hash at
    every position, in six passes over the bytes instead of 64. Blocks of `block` bytes with a 63-byte overlap."""
    T = np.asarray(table, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    n = data.size
    out = np.empty(max(0, n - 63), dtype=np.uint64)
    for b0 in range(63, n, block):
        lo = b0 - 63
        h = T[data[lo:min(n, b0 + block)]]
        L = 1
        while L < 64:
            h = h[L:] ^ _rotl(h[:-L], L)
            L *= 2
        out[lo:lo + h.size] = h
    return out


def candidates_model(cfg, data: np.ndarray) -> np.ndarray:
    """candidate END offsets restated: (h & mask) >= break_min at every window end >= 64"""
    h = window_hashes(np.ctypeslib.as_array(cfg.table), data)
    hit = (h & np.uint64(cfg.mask)) >= np.uint64(cfg.break_min)
    return (np.nonzero(hit)[0] + 64).astype(np.uint64)
