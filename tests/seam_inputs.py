"""Planted-cut inputs for the page ring's seam tests (test infrastructure).

The page ring splits a stream into pages of `page` bytes; a chunk may cross one page seam, and then its SHA-256 blocks come
from two physical pages (ring_order_one: `p1`, `p2v`, `len1`) and a block that starts before the seam reads on into the
previous page's 128-byte tail pad. The scan warms its window for a page's first 64 positions from the page's head pad. Which
of these cases random bytes produce is left to chance; the builder here produces bytes whose serial cut list is a PLANNED one,
so every case is present by construction and the CPU oracle confirms the plan.

Two tools on the Buzhash window hash (dense_inputs.window_hash; the break test of oracle/buzhash_oracle.c is
`(h & mask) >= break_min`, break_min = mask - 2):
  * clear: random bytes made candidate-free (the last byte of every candidate's window re-drawn until none is left);
  * plant: a candidate that ends at exactly `e` and no other one — a meet in the middle over the four bytes in front of `e`
    (as dense_inputs.all_candidate_pattern, aimed at the low bits the break test looks at).
A chunk end planted at distance [max(min, 65), max] from the previous cut is then a cut of the serial chunker, a gap of exactly
`max` needs no candidate at all, and the stream's last chunk ends where its bytes do.
"""
import numpy as np

from dense_inputs import _rotl, window_hash

# the second piece of a seam-crossing chunk: its tail or padding block before, on or after the seam
SHA_P2 = tuple(range(0, 9)) + tuple(range(52, 73))
# chunker average -> page size the seam tests run it at
PAGES = {256: 65536, 4096: 65536, 65536: 262144}
# chunk lengths around the edge rows of blob.hip's piece walk (rows of 1024 bytes, pieces of 64 KiB): under one 16-byte unit,
# the row and piece edges, and n = 1..3 mod 1024 above a row, where the four inverted bytes reach into row 1
BLOB_PIECE = 1 << 16
BLOB_EDGE_LENS = (list(range(1, 21)) + list(range(1023, 1029)) + list(range(2047, 2053)) +
                  list(range(BLOB_PIECE - 1, BLOB_PIECE + 4)) + list(range(2 * BLOB_PIECE + 1, 2 * BLOB_PIECE + 4)))


def effmin(cfg) -> int:
    """Smallest chunk the serial chunker cuts by a candidate: the first break test comes after the 64-byte warm-up."""
    return max(int(cfg.min), 65)


def sha_grid_cases():
    """(len1, p2) of the SHA seam grid: len1 = 1..68 bytes before the seam, each with a short (0..8) and a long (52..72)
    second piece; every second piece (0: the chunk ends on the seam) with all four chunk-start alignments; chunk lengths over
    all 64 residues."""
    cases = set()
    for len1 in range(1, 69):
        cases.add((len1, 1 + len1 % 7))
        cases.add((len1, 52 + len1 % 21))
    for p2 in SHA_P2:
        for a in range(4):
            if not any(p == p2 and (-l) % 4 == a for l, p in cases):
                cases.add((next(l for l in range(68, 0, -1) if (-l) % 4 == a and (l, p2) not in cases), p2))
    for m in range(64):
        if not any((l + p) % 64 == m for l, p in cases):
            cases.add(next((l, p) for l in range(1, 69) for p in SHA_P2[:9] if (l + p) % 64 == m))
    return sorted(cases)


class Planter:
    """clear / plant for one chunker config."""

    def __init__(self, O, cfg, seed: int = 0):
        self.O, self.cfg = O, cfg
        self.mask = int(cfg.mask)
        self.T = np.asarray(np.ctypeslib.as_array(cfg.table), dtype=np.uint64).copy()
        self.rng = np.random.default_rng(seed)
        v = np.arange(256)
        # contribution of the window's bytes 60, 61 (left) and 62, 63 (right) to the hash of a window that ends on byte 63
        left = (_rotl(self.T[v], 3)[:, None] ^ _rotl(self.T[v], 2)[None, :]).reshape(-1)
        self.right = (_rotl(self.T[v], 1)[:, None] ^ _rotl(self.T[v], 0)[None, :]).reshape(-1)
        lm = left & np.uint64(self.mask)
        self.order = np.argsort(lm, kind="stable")
        self.lsorted = lm[self.order]

    def clear(self, data: np.ndarray) -> None:
        """Re-draw the last byte of every candidate's window until the bytes hold no candidate."""
        for _ in range(200):
            c = self.O.candidates(self.cfg, data)
            if c.size == 0:
                return
            idx = c.astype(np.int64) - 1
            data[idx] = self.rng.integers(0, 256, idx.size, dtype=np.uint8)
        raise AssertionError("clear did not converge")

    def _local(self, data, e):
        lo = max(0, e - 128)
        return self.O.candidates(self.cfg, data[lo:e + 64]).astype(np.int64) + lo

    def plant(self, data: np.ndarray, e: int, pair: bool = False) -> None:
        """Make a candidate end at exactly `e` (window data[e-64:e]) without creating any other one; `data` is candidate-free
        around `e` but for candidates planted at least 64 bytes in front of it, which stay.

        pair: candidates at e - 1 AND e. h(e) = rotl(h(e - 1), 1) ^ T[b[e - 1]] ^ T[b[e - 65]] (rotl by 64 is the identity),
        so with b[e - 1] = b[e - 65] and the low bits of h(e - 1) all ones, the low bits of h(e) are all ones but bit 0 (which
        is bit 31 of h(e - 1)): both pass the break test. The plant then aims at e - 1 with the value `mask` alone."""
        keep = set()
        if pair:
            assert 69 <= e <= data.size, e
            keep.add(e)
            e -= 1
        keep |= set(int(x) for x in self._local(data, e))
        if pair:
            data[e] = data[e - 64]
        assert 68 <= e <= data.size, e
        mask = np.uint64(self.mask)
        keep = sorted(keep | {e})
        for attempt in range(16):
            if attempt:
                # h(e + 32) takes the four bytes in front of e at the same rotations as h(e) (rotl by k and k + 32 agree):
                # for some bytes around e every hit here is a hit there too. A byte that only h(e) sees breaks the tie.
                q = e - 36 - int(self.rng.integers(0, 24))
                data[q] = self.rng.integers(0, 256)
                if pair:
                    # h(e + 64) sees b[e] but none of the bytes the search sets: the pair's shared byte is re-drawn too; and
                    # h(e + 2) = rotl(h(e), 2) passes as well when b[e + 1] = b[e - 63]: that byte is re-drawn as well
                    data[e - 64] = data[e] = self.rng.integers(0, 256)
                    data[e - 63] = self.rng.integers(0, 256)
            w = data[e - 64:e].copy()
            rest = window_hash(self.T, w)
            for j in range(60, 64):
                rest ^= int(_rotl(self.T[int(w[j])], 63 - j))
            for _ in range(4):
                # 256 right halves meet one of 65 536 left halves with probability 2^(24 - bits) each: enough up to 20 bits;
                # wider masks (up to 29 bits at avg 2^28) search every right half (~2^(32 - bits) hits)
                r = self.rng.integers(0, 65536, 256) if self.mask < (1 << 20) else self.rng.permutation(65536)
                v = np.uint64(self.mask - int(self.rng.integers(0, 3)))      # mask, mask - 1 or mask - 2: the break test passes
                if pair:
                    v = np.uint64(self.mask)
                want = (np.uint64(rest) ^ self.right[r] ^ v) & mask
                pos = np.searchsorted(self.lsorted, want)
                pos[pos >= self.lsorted.size] = 0
                for i in np.nonzero(self.lsorted[pos] == want)[0][:32]:
                    lv, rv = int(self.order[pos[i]]), int(r[i])
                    old = data[e - 4:e].copy()
                    data[e - 4:e] = (lv >> 8, lv & 255, rv >> 8, rv & 255)
                    if list(self._local(data, e)) == keep:
                        return
                    data[e - 4:e] = old
        raise AssertionError(f"could not plant a candidate at {e}")


def build_stream(O, cfg, page: int, cases, seed: int, fill_max: int = 0, planter=None):
    """Host bytes of one ring stream and their planned cut list (chunk END offsets), confirmed by the serial chunker.

    `cases`, one per page seam in order (seam k * page for k = 1, 2, ...):
      ("cross", len1, p2)  a chunk [seam - len1, seam + p2) (of at least max(min, 65) bytes);
      ("final", len1, p2)  the same as the stream's last chunk (any length): the stream ends at seam + p2 — last case only;
      ("end", d)           a chunk that started in the previous page ends at seam + d (d <= 0: before or on the seam);
      ("onseam",)          a chunk ends exactly on the seam, a candidate that must NOT cut sits 64 bytes behind it (the
                           chunk there is 64 bytes long: below the first break test), the next chunk starts at the page start;
      ("tiny", n)          the whole stream is n bytes (one chunk, or none) — only case.
    Between cases: filler chunks of at most `fill_max` bytes (default the maximum: cut by size, no candidate needed)."""
    em, mx = effmin(cfg), int(cfg.max)
    fill_max = min(fill_max or mx, mx)
    P = planter or Planter(O, cfg, seed)
    rng = np.random.default_rng(seed + 7)
    ends, extras = [], []
    pos = 0

    def filler(target, first_min=em):
        nonlocal pos
        gap = target - pos
        if gap == 0:
            return
        assert gap >= first_min, (pos, target)
        n = -(-gap // fill_max)
        sizes = [fill_max] * (n - 1) + [gap - (n - 1) * fill_max]
        if sizes[-1] < em:
            sizes[-2] -= em - sizes[-1]
            sizes[-1] = em
        if n > 1 and first_min > em:
            sizes.sort(reverse=True)
        elif n > 1:
            rng.shuffle(sizes)
        assert sum(sizes) == gap and all(em <= s <= mx for s in sizes), sizes
        for s in sizes:
            pos += s
            ends.append(pos)

    if cases and cases[0][0] == "tiny":
        assert len(cases) == 1
        n = cases[0][1]
        data = rng.integers(0, 256, n, dtype=np.uint8)
        P.clear(data)
        want = [n] if n else []
    else:
        after_extra = False
        for k, case in enumerate(cases, start=1):
            seam = k * page
            kind = case[0]
            fm = max(em, 140) if after_extra else em            # keep the next plant's bytes clear of the extra candidate
            after_extra = False
            if kind in ("cross", "final"):
                len1, p2 = case[1], case[2]
                assert kind == "final" or em <= len1 + p2 <= mx, case
                assert kind == "cross" or k == len(cases), "a final chunk ends the stream"
                filler(seam - len1, fm)
                pos = seam + p2
                ends.append(pos)
            elif kind == "end":
                d = case[1]
                L = int(rng.integers(max(em, d + 1), min(mx, em + 300) + 1))
                filler(seam + d - L, fm)
                pos = seam + d
                ends.append(pos)
            elif kind == "onseam":
                filler(seam, fm)
                extras.append(seam + 64)
                after_extra = True
            else:
                raise ValueError(case)
        want = list(ends)
        n = pos
        data = rng.integers(0, 256, n, dtype=np.uint8)
        P.clear(data)
        prev = 0
        plants = []
        for e in ends:
            if e != n and e - prev != mx:
                plants.append(e)
            prev = e
        for e in sorted(plants + extras):
            P.plant(data, e)
        assert list(O.candidates(cfg, data)) == sorted(plants + extras)
    got = O.chunk_stream(cfg, data)
    assert list(got) == want, "the serial chunker does not confirm the plan"
    return data, np.asarray(want, dtype=np.uint64)


def census(ends, page: int):
    """What the cut list covers: crossing chunks (len1, p2, start mod 4, L mod 64), chunks ending on a seam, candidate-window
    cases (end - seam for ends within 64 bytes of a seam, in a chunk that started in the previous page)."""
    cross, onseam, near = set(), 0, set()
    s = 0
    for e in (int(x) for x in ends):
        L = e - s
        if s // page != (e - 1) // page:
            seam = (e - 1) // page * page
            len1 = seam - s
            cross.add((len1, e - seam, s % 4, L % 64))
        if e % page == 0 and e > 0:
            onseam += 1
        K = (e - 1) // page * page                         # the seam the chunk's last byte lies behind
        if K > 0 and 0 < e - K <= 64 and K - page <= s < K:
            near.add(e - K)
        K = -(-e // page) * page                           # the seam at or after the chunk's end
        if K > 0 and 0 <= K - e <= 64 and s >= K - page:
            near.add(e - K)
        s = e
    return cross, onseam, near


def plan(O, avg: int, seed: int = 1):
    """The seam grids for one chunker: [(bytes, planned ends)] — mid-stream seam cases in streams of many pages, every
    too-short crossing chunk as the last chunk of a stream of its own, and the tiny streams."""
    cfg = O.new_config(avg)
    page = PAGES[avg]
    em, mx = effmin(cfg), int(cfg.max)
    literal = sha_grid_cases()
    mid = [("cross", l, p) for l, p in literal if em <= l + p <= mx]
    finals = [("final", l, p) for l, p in literal if l + p < em]
    seen = set(literal)
    for r in range(64):                                   # the same residues on chunks long enough to sit mid-stream
        for p2 in (r % 9, 52 + r % 21):
            l = r or 64
            while l + p2 < em:
                l += 64
            if (l, p2) not in seen:
                seen.add((l, p2))
                mid.append(("cross", l, p2))
    scan = [("end", d) for d in range(1, 65)] + [("end", -d) for d in range(0, 65)] + [("onseam",)] * 2
    rng = np.random.default_rng(seed)
    allmid = mid + scan
    rng.shuffle(allmid)
    fill_max = mx if avg <= 4096 else 2 * avg           # avg 64 KiB: 128 KiB chunks keep a page's hash chains short
    P = Planter(O, cfg, seed)
    out = []
    per = 48
    for i in range(0, len(allmid), per):
        out.append(build_stream(O, cfg, page, allmid[i:i + per], seed + i, fill_max, P))
    for i, c in enumerate(finals):
        out.append(build_stream(O, cfg, page, [c], seed + 1000 + i, fill_max, P))
    for n in list(range(0, 131)) + [int(cfg.min) - 1, int(cfg.min), int(cfg.min) + 1]:
        out.append(build_stream(O, cfg, page, [("tiny", n)], seed + 5000 + n, fill_max, P))
    return cfg, page, out
