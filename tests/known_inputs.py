"""Crafted digests for the known-chunk set (pbs_plus_amd/csrc/known.hip) — test infrastructure.

The set places a digest by a mix of its bytes 8..31 (the home slot) and sorts a batch by a mix of all 32 bytes (the
32-bit sort key). The mix is splitmix64's finaliser, which is a bijection of 64-bit words: two multiplications by odd
constants (inverted by their modular inverses) and three xor-shifts (inverted by repeating them). So digests with a
CHOSEN home slot, sort key and tag can be written down:

    home(d) = mix(w1 ^ mix(w2 ^ mix(w3)))      =>  w1 = unmix(H) ^ mix(w2 ^ mix(w3))           for any w2, w3
    key(d)  = low 32 bits of mix(home ^ w0)    =>  w0 = H ^ unmix(K | r << 32)                 for any 32-bit r

(w0..w3: the digest's four little-endian 64-bit words, as known_load of known_hash.h reads them.)
tests/test_known_inputs.py binds this port to the C++ of known_hash.h: if the device's hash changes, it fails there.

Also here: the record builder and the sequential reference (`records`, `set_model`) that the GPU tests of the set share, a
sequential model of the table itself (`TableModel`: which slot, how long a probe, when it grows — it proves that a
scenario reaches the path it claims, it is NOT the reference for the flags), and the scenarios of
tests/test_gpu_known_collisions.py, which tests/test_known_inputs.py replays on the model without a GPU.
"""
import numpy as np

M64 = (1 << 64) - 1
_C1, _C2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
_C1_INV, _C2_INV = pow(_C1, -1, 1 << 64), pow(_C2, -1, 1 << 64)

# the low 24 bits decide the slot in every table of up to 2^24 slots, before and after a growth
HOME_LAST = 0x5A17C3D2E1FFFFFF      # the last slot: a chain from here wraps to slot 0 at once
HOME_FIRST = 0xC96E4B07A2000000     # slot 0
HOME_MID = 0x3B9F12E457000200       # slot 512: a chain of up to 512 stays inside a 1 024-slot table

MIN_SLOTS = 1024


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def _mul(x, c):
    with np.errstate(over="ignore"):
        return np.multiply(x, np.uint64(c), dtype=np.uint64)


def _unshift(x, s):
    """the inverse of y = x ^ (x >> s)"""
    y = x
    for _ in range(64 // s + 1):
        y = x ^ (y >> np.uint64(s))
    return y


def mix(x):
    """known_mix (splitmix64's finaliser) on uint64 values of any shape"""
    x = _u64(x)
    x = x ^ (x >> np.uint64(30))
    x = _mul(x, _C1)
    x = x ^ (x >> np.uint64(27))
    x = _mul(x, _C2)
    return x ^ (x >> np.uint64(31))


def unmix(x):
    """mix's inverse"""
    x = _unshift(_u64(x), 31)
    x = _unshift(_mul(x, _C2_INV), 27)
    return _unshift(_mul(x, _C1_INV), 30)


def words(digests):
    """(n, 4) uint64: the little-endian words of (n, 32) uint8 digests"""
    return np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32).view("<u8").astype(np.uint64)


def home(digests):
    w = words(digests)
    return mix(w[:, 1] ^ mix(w[:, 2] ^ mix(w[:, 3])))


def key(digests):
    return (mix(home(digests) ^ words(digests)[:, 0]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def tag(digests):
    w0 = words(digests)[:, 0]
    return np.where(w0 == 0, np.uint64(1), w0)


def _rand64(rng, n):
    return rng.integers(0, 1 << 64, n, dtype=np.uint64)


def family(rng, n, home=None, key=None, w0=None, w1=None):
    """n pairwise distinct digests, (n, 32) uint8.
    home = H: every known_home is H.  key = K: every known_key is K (with no home: each digest a random home, the run is
    spread over the table).  w0 = W (in place of key, with home): tag, home and key are all shared, the digests differ
    only in bytes 8..31.  w1 = V as well (with home): they differ only in bytes 16..31."""
    assert key is None or w0 is None
    assert w1 is None or home is not None
    out = np.zeros((0, 4), dtype=np.uint64)
    while out.shape[0] < n:
        m = n - out.shape[0]
        w = np.empty((m, 4), dtype=np.uint64)
        w[:, 3] = _rand64(rng, m)
        if w1 is not None:
            w[:, 1] = np.uint64(w1)
            w[:, 2] = unmix(np.uint64(w1) ^ unmix(np.uint64(home))) ^ mix(w[:, 3])
        else:
            w[:, 2] = _rand64(rng, m)
            inner = mix(w[:, 2] ^ mix(w[:, 3]))
            w[:, 1] = _rand64(rng, m) if home is None else unmix(np.uint64(home)) ^ inner
        h = mix(w[:, 1] ^ mix(w[:, 2] ^ mix(w[:, 3])))
        if w0 is not None:
            w[:, 0] = np.uint64(w0)
        elif key is not None:
            w[:, 0] = h ^ unmix(np.uint64(key) | (rng.integers(0, 1 << 32, m, dtype=np.uint64) << np.uint64(32)))
        else:
            w[:, 0] = _rand64(rng, m)
        out = np.unique(np.concatenate([out, w]), axis=0)
    out = out[rng.permutation(out.shape[0])[:n]]
    return np.ascontiguousarray(out.astype("<u8")).view(np.uint8).reshape(n, 32)


def random_digests(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


# ---- the records and the reference the GPU tests of the set share ----

def records(digests, sizes=None, seed=0):
    from pbs_plus_amd import RECORD_DTYPE

    d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
    r = np.zeros(d.shape[0], dtype=RECORD_DTYPE)
    r["digest"] = d
    r["size"] = sizes if sizes is not None else np.random.default_rng(seed).integers(1, 1 << 20, d.shape[0])
    r["end"] = np.cumsum(r["size"].astype(np.uint64))
    return r


def set_model(initial, recs, insert=True):
    """The reference rule, sequentially: (known flags, stats, the set afterwards)."""
    s = set(initial)
    seen = set()
    known = np.zeros(recs.size, dtype=np.uint8)
    for i, d in enumerate(recs["digest"]):
        b = d.tobytes()
        if b in s or b in seen:
            known[i] = 1
        else:
            seen.add(b)
    sizes = recs["size"].astype(np.uint64)
    stats = {"nrecords": int(recs.size), "nunique": int((known == 0).sum()), "total_bytes": int(sizes.sum()),
             "unique_bytes": int(sizes[known == 0].sum())}
    return known, stats, (s | seen) if insert else s


def digest_set(digests):
    return {bytes(d) for d in np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)}


# ---- a sequential model of the table ----

def _pow2_at_least(v):
    p = MIN_SLOTS
    while p < v:
        p <<= 1
    return p


class TableModel:
    """The open-addressing table of known.hip, one digest at a time: home slot = known_home & (slots - 1), linear probing,
    growth as grow() — to max(pow2_at_least(2 * want), 2 * slots) whenever count + nnew > slots / 2, everything stored
    rehashed in slot order. Which slot a digest gets inside a contended chain depends on the order of insertion (on the
    device: on scheduling); WHICH slots a chain occupies, how long a probe for an absent digest is and when the table
    grows do not."""

    def __init__(self, slots=MIN_SLOTS):
        assert slots >= MIN_SLOTS and slots & (slots - 1) == 0
        self.slots = slots
        self.cells = {}          # slot -> digest bytes
        self.where = {}          # digest bytes -> slot
        self.homes = {}          # digest bytes -> known_home (hashed a batch at a time)
        self.growths = 0

    @classmethod
    def for_capacity(cls, capacity):
        """the table pbsgpu_known_create(capacity) allocates"""
        return cls(_pow2_at_least(2 * (capacity if capacity else 1 << 16)))

    @property
    def count(self):
        return len(self.where)

    def _home_slot(self, b):
        if b not in self.homes:
            self.homes[b] = int(home(np.frombuffer(b, dtype=np.uint8))[0])
        return self.homes[b] & (self.slots - 1)

    def _put(self, b):
        s = self._home_slot(b)
        while s in self.cells:
            s = (s + 1) & (self.slots - 1)
        self.cells[s] = b
        self.where[b] = s

    def insert(self, digests):
        """One inserting call (add / classify(insert=True)) on these digests; returns True when the table grew in it."""
        new = {}                 # (insertion-ordered)
        d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, 32)
        self.homes.update(zip((bytes(x) for x in d), (int(h) for h in home(d))))
        for b in (bytes(x) for x in d):
            if b not in self.where:
                new[b] = None
        grew = self.count + len(new) > self.slots // 2
        if grew:
            old = [self.cells[s] for s in sorted(self.cells)]
            self.slots = max(_pow2_at_least(2 * (self.count + len(new))), 2 * self.slots)
            self.cells, self.where = {}, {}
            self.growths += 1
            for b in old:
                self._put(b)
        for b in new:
            self._put(b)
        assert 2 * self.count <= self.slots
        return grew

    def slot_of(self, digest):
        return self.where.get(bytes(digest))

    def probe(self, digest):
        """(found, slots read by a lookup: every occupied slot it passes plus the one that ends it)"""
        b = bytes(digest)
        s, n = self._home_slot(b), 1
        while s in self.cells and self.cells[s] != b:
            s = (s + 1) & (self.slots - 1)
            n += 1
        return s in self.cells, n

    def occupied(self):
        return set(self.cells)


# ---- the scenarios of tests/test_gpu_known_collisions.py ----
# Each returns a dict: its digest arrays, and "families": [(name, digests, claims)] with claims among home / key / w0 / w1 —
# what tests/test_known_inputs.py checks on the native driver's output.

def _shuffled(rng, d):
    return d[rng.permutation(d.shape[0])]


def scenario_one_home(H, seed=101):
    """a: 1 200 digests of one home in three parts of 400; q_ab = a and b, a third of them repeated, shuffled;
    q_all = all 1 200 with 150 of c repeated, shuffled"""
    rng = np.random.default_rng(seed)
    fam = family(rng, 1200, home=H)
    a, b, c = fam[:400], fam[400:800], fam[800:]
    ab = fam[:800]
    q_ab = _shuffled(rng, np.concatenate([ab, ab[rng.integers(0, 800, 267)]]))
    q_all = _shuffled(rng, np.concatenate([fam, c[rng.integers(0, 400, 150)]]))
    return dict(a=a, b=b, c=c, q_ab=q_ab, q_all=q_all, families=[("one_home", fam, dict(home=H))])


KEYS_ENDS = (0, 0xFFFFFFFF)


def scenario_one_key(seed=202, shuffle_seed=0):
    """b: three sort keys (0, 0xFFFFFFFF, one random); per key 200 digests of one home and 200 of spread homes, each 1 to 4
    times; 500 random digests; shuffled by shuffle_seed (the digests depend on `seed` alone). preload = every third
    distinct digest."""
    rng = np.random.default_rng(seed)
    keys = list(KEYS_ENDS) + [int(rng.integers(1 << 8, 1 << 31))]
    fams, parts = [], []
    for i, K in enumerate(keys):
        H = int(_rand64(rng, 1)[0])
        one = family(rng, 200, home=H, key=K)
        spread = family(rng, 200, key=K)
        fams += [("key%d_one_home" % i, one, dict(home=H, key=K)), ("key%d_spread" % i, spread, dict(key=K))]
        both = np.concatenate([one, spread])
        parts.append(np.repeat(both, rng.integers(1, 5, 400), axis=0))
    rnd = random_digests(rng, 500)
    distinct = np.concatenate([f[1] for f in fams] + [rnd])
    batch = _shuffled(np.random.default_rng(1000 + shuffle_seed), np.concatenate(parts + [rnd]))
    return dict(keys=keys, batch=batch, distinct=distinct, preload=distinct[::3], run_lengths=[p.shape[0] for p in parts],
                families=fams)


def scenario_equal_tag_home_key(seed=303):
    """c: 300 digests equal in tag, home and key (they differ in bytes 8..31 only), 100 more that also share bytes 8..15,
    and 150 + 150 of another home with w0 = 0 and w0 = 1 (both stored as tag 1). content = a random half; queries = all
    of them, a third twice, shuffled."""
    rng = np.random.default_rng(seed)
    H, H2, W, V = (int(x) for x in _rand64(rng, 4))
    f_w0 = family(rng, 300, home=H, w0=W)
    f_w1 = family(rng, 100, home=H, w0=W, w1=V)
    f_t0 = family(rng, 150, home=H2, w0=0)
    f_t1 = family(rng, 150, home=H2, w0=1)
    alld = np.concatenate([f_w0, f_w1, f_t0, f_t1])
    m = alld.shape[0]
    content = alld[rng.permutation(m)[: m // 2]]
    queries = _shuffled(rng, np.concatenate([alld, alld[rng.integers(0, m, m // 3)]]))
    return dict(all=alld, content=content, queries=queries,
                families=[("w0", f_w0, dict(home=H, w0=W)), ("w0_w1", f_w1, dict(home=H, w0=W, w1=V)),
                          ("tag_zero", f_t0, dict(home=H2, w0=0)), ("tag_one", f_t1, dict(home=H2, w0=1))])


def scenario_load_boundary(seed=404):
    """d: 514 digests of the last slot's home: 511 to add at once, the 512th, the 513th, and one that stays absent"""
    rng = np.random.default_rng(seed)
    fam = family(rng, 514, home=HOME_LAST)
    return dict(first=fam[:511], d512=fam[511:512], d513=fam[512:513], absent=fam[513:514],
                families=[("boundary", fam, dict(home=HOME_LAST))])


def scenario_fused(seed=505):
    """e: 1 500 records over 750 distinct digests (two one-home one-key families of 300 and 150 random ones, every one at
    least once, shuffled); a third of the distinct digests preloaded; chunk i = a random range of 0 to 3 000 bytes of a
    1 MiB buffer"""
    rng = np.random.default_rng(seed)
    fams = []
    for i in range(2):
        H, K = int(_rand64(rng, 1)[0]), int(rng.integers(0, 1 << 32))
        fams.append(("fused%d" % i, family(rng, 300, home=H, key=K), dict(home=H, key=K)))
    distinct = np.concatenate([f[1] for f in fams] + [random_digests(rng, 150)])
    batch = _shuffled(rng, np.concatenate([distinct, distinct[rng.integers(0, 750, 750)]]))
    nbytes = 1 << 20
    lengths = rng.integers(0, 3001, 1500).astype(np.uint64)
    lengths[:4] = (0, 1, 3, 3000)
    offsets = (rng.random(1500) * (nbytes - lengths.astype(np.float64))).astype(np.uint64)
    chunks = np.stack([offsets, lengths], axis=1)
    return dict(batch=batch, distinct=distinct, preload=distinct[::3], chunks=chunks, nbytes=nbytes, data_seed=seed + 1,
                families=fams)
