"""zstd frames built sequence by sequence, for the lane cooperation of the device decoder (tests/test_gpu_zstd_seq.py) and
the CPU run of the same format core (tests/test_zstd_seq_native.py). Pure Python: no libzstd, nothing from the package.

  frame(blocks)    the writer: a single-segment frame with a 4-byte content size. A compressed block carries its literals
                   raw (or as an RLE literals section) and its sequences under the three predefined FSE tables; the
                   states are picked from the last sequence backwards (for each symbol exactly one state's range holds
                   the next state) and the backward bit stream is written as one big integer under an end mark.
  execute(blocks)  the reference: a byte-at-a-time executor with the repeat-offset rules of RFC 8878 3.1.1.5. The only
                   source of expected contents.
  cases()          the family. tests/golden/make_zstd_seq_golden.py sets every case against libzstd where it loads and
                   records lengths and SHA-256s in tests/golden/zstd_seq_v1.json; the tests regenerate and compare.

A block is (literals, [(ll, ml, offset_value), ...]) or one of comp(), raw(), rle(), treeless() below. offset_value 1-3
are the repeat codes, offset_value - 3 is the offset otherwise.

Below, a match at output position `at` with offset `off` and length `ml` has the source [at-off, at-off+min(off,ml));
`seen` is the variable of decode_block (zstd_decode.h): the match loop waits for the stores before a match whose source
ends above it, and then sets it to `at`. Within a batch it starts at the first match's `at`. A match with off < ml has its
source end at `at`, which lies at least 3 above `seen` for every match but the first of a batch: the seen-edge cases take
off < ml at that nearest distance (seen + 3) as the second and the 40th match, and exactly at `seen` as the first match of
a second batch."""
import hashlib
import struct
import zlib

import numpy as np

OK, BAD_FRAME, BAD_SIZE, UNSUPPORTED = range(4)
MAGIC = struct.pack("<I", 0xFD2FB528)

# ---- constants of the format (RFC 8878 3.1.1.3.2.1.1 and 3.1.1.3.2.2) -----------------------------------------------------
LL_BASE = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024,
           2048, 4096, 8192, 16384, 32768, 65536)
LL_BITS = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)
ML_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33,
           34, 35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539)
ML_BITS = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3,
           4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16)
LL_DEFAULT = (4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1)
ML_DEFAULT = (1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
              1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1)
OF_DEFAULT = (1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1)
LL_LOG, OF_LOG, ML_LOG = 6, 5, 6
BLOCK_MAX = 128 << 10


def _fse_table(norm, log):
    """the decoding table of a normalised distribution: per state (symbol, bits to read, base of the next state)"""
    size = 1 << log
    sym, nxt, high = [0] * size, {}, size
    for s, p in enumerate(norm):
        if p == -1:
            high -= 1
            sym[high] = s
            nxt[s] = 1
        else:
            nxt[s] = p
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, p in enumerate(norm):
        for _ in range(max(p, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos >= high:
                pos = (pos + step) & (size - 1)
    assert pos == 0
    table = []
    for u in range(size):
        nx = nxt[sym[u]]
        nxt[sym[u]] += 1
        nb = log - (nx.bit_length() - 1)
        table.append((sym[u], nb, (nx << nb) - size))
    return table


_LL, _OF, _ML = _fse_table(LL_DEFAULT, LL_LOG), _fse_table(OF_DEFAULT, OF_LOG), _fse_table(ML_DEFAULT, ML_LOG)


def _code(base, v):
    c = max(i for i, b in enumerate(base) if b <= v)
    return c, v - base[c]


def _states(table, codes):
    """one state per code such that each state's successor is reachable from it: (states, bits read after each but the last)"""
    by_sym = {}
    for u, (s, nb, b) in enumerate(table):
        by_sym.setdefault(s, []).append((b, nb, u))
    states, bits = [by_sym[codes[-1]][0][2]], []
    for c in reversed(codes[:-1]):
        hit = [(b, nb, u) for b, nb, u in by_sym[c] if b <= states[-1] < b + (1 << nb)]
        assert len(hit) == 1
        b, nb, u = hit[0]
        bits.append((states[-1] - b, nb))
        states.append(u)
    return states[::-1], bits[::-1]


# ---- blocks ----------------------------------------------------------------------------------------------------------------
def comp(literals, seqs, rle_literals=False, modes=0, pad_bits=0):
    """a compressed block. modes: the Symbol_Compression_Modes byte as written (the sequences are coded under the predefined
    tables whatever it says: anything but 0 makes a frame for the stale-* cases). pad_bits: zero bits below the stream"""
    return {"kind": "comp", "lit": bytes(literals), "seqs": [tuple(s) for s in seqs], "rle": rle_literals, "modes": modes, "pad": pad_bits}


def raw(data):
    return {"kind": "raw", "data": bytes(data)}


def rle(value, n):
    return {"kind": "rle", "value": value, "n": n}


def treeless(regen, stream):
    """a compressed block of treeless (type 3) literals in one stream and no sequences: for the stale-* cases"""
    return {"kind": "treeless", "regen": regen, "stream": bytes(stream)}


def _norm(b):
    return b if isinstance(b, dict) else comp(*b)


def _block_header(kind, size, last):
    assert size <= BLOCK_MAX
    return struct.pack("<I", int(last) | kind << 1 | size << 3)[:3]


def _literals_section(lit, as_rle):
    n, t = len(lit), 1 if as_rle else 0
    if as_rle:
        assert n >= 1 and lit == lit[:1] * n
    if n < 32:
        head = bytes([t | n << 3])
    elif n < 4096:
        head = struct.pack("<H", t | 1 << 2 | n << 4)
    else:
        assert n < 1 << 20
        head = struct.pack("<I", t | 3 << 2 | n << 4)[:3]
    return head + (lit[:1] if as_rle else lit)


def _sequences_section(seqs, modes, pad, tables=None, desc=b""):
    """tables: the (table, accuracy log) of literal lengths, offsets and match lengths that the sequences are coded under
    (the predefined ones by default); desc: what stands between the modes byte and the bit stream (tests/zstd_huf_inputs.py)"""
    (t_ll, l_ll), (t_of, l_of), (t_ml, l_ml) = tables or ((_LL, LL_LOG), (_OF, OF_LOG), (_ML, ML_LOG))
    n = len(seqs)
    if n == 0:
        return b"\x00"
    if n < 128:
        head = bytes([n])
    elif n < 0x7F00:
        head = bytes([(n >> 8) + 128, n & 255])
    else:
        head = b"\xff" + struct.pack("<H", n - 0x7F00)
    ll = [_code(LL_BASE, s[0]) for s in seqs]
    ml = [_code(ML_BASE, s[1]) for s in seqs]
    of = [(s[2].bit_length() - 1, s[2] - (1 << (s[2].bit_length() - 1))) for s in seqs]
    s_ll, b_ll = _states(t_ll, [c for c, _ in ll])
    s_of, b_of = _states(t_of, [c for c, _ in of])
    s_ml, b_ml = _states(t_ml, [c for c, _ in ml])
    fields = [(s_ll[0], l_ll), (s_of[0], l_of), (s_ml[0], l_ml)]  # in the order a decoder reads them
    for i in range(n):
        fields += [(of[i][1], of[i][0]), (ml[i][1], ML_BITS[ml[i][0]]), (ll[i][1], LL_BITS[ll[i][0]])]
        if i + 1 < n:
            fields += [b_ll[i], b_ml[i], b_of[i]]
    v, total = 1, 0  # the end mark, then every field below it
    for val, nb in fields:
        assert 0 <= val < 1 << nb or (nb == 0 and val == 0)
        v = v << nb | val
        total += nb
    v <<= pad
    total += pad
    return head + bytes([modes]) + desc + v.to_bytes(total // 8 + 1, "little")


def frame(blocks, content_size=None):
    """the frame of `blocks`; content_size: what the header declares (default: what execute() produces)"""
    blocks = [_norm(b) for b in blocks]
    body = []
    for i, b in enumerate(blocks):
        last = i == len(blocks) - 1
        if b["kind"] == "raw":
            body.append(_block_header(0, len(b["data"]), last) + b["data"])
        elif b["kind"] == "rle":
            body.append(_block_header(1, b["n"], last) + bytes([b["value"]]))
        elif b["kind"] == "treeless":
            assert b["regen"] < 1024 and len(b["stream"]) < 1024
            payload = struct.pack("<I", 3 | b["regen"] << 4 | len(b["stream"]) << 14)[:3] + b["stream"] + b"\x00"
            body.append(_block_header(2, len(payload), last) + payload)
        else:  # ("payload": the block's bytes as tests/zstd_huf_inputs.py wrote them, for the same literals and sequences)
            payload = b.get("payload") or _literals_section(b["lit"], b["rle"]) + _sequences_section(b["seqs"], b["modes"], b["pad"])
            body.append(_block_header(2, len(payload), last) + payload)
    if content_size is None:
        content_size = len(execute(blocks))
    return MAGIC + b"\xa0" + struct.pack("<I", content_size) + b"".join(body)


def execute(blocks):
    """what the blocks decode to, one byte at a time"""
    out = bytearray()
    rep = [1, 4, 8]
    for b in (_norm(b) for b in blocks):
        if b["kind"] == "raw":
            out += b["data"]
            continue
        if b["kind"] == "rle":
            out += bytes([b["value"]]) * b["n"]
            continue
        assert b["kind"] == "comp" and b["modes"] == 0, "nothing to execute: a frame nobody may accept"
        lit, lp, start = b["lit"], 0, len(out)
        for ll, ml, ov in b["seqs"]:
            assert ll <= len(lit) - lp and ml >= 3 and ov >= 1
            out += lit[lp:lp + ll]
            lp += ll
            if ov > 3:
                off = ov - 3
                rep = [off, rep[0], rep[1]]
            else:
                idx = ov + (1 if ll == 0 else 0)
                if idx == 1:
                    off = rep[0]
                elif idx == 2:
                    off = rep[1]
                    rep = [off, rep[0], rep[2]]
                elif idx == 3:
                    off = rep[2]
                    rep = [off, rep[0], rep[1]]
                else:
                    off = rep[0] - 1
                    rep = [off, rep[0], rep[1]]
            assert 1 <= off <= len(out), (off, len(out))
            for _ in range(ml):
                out.append(out[-off])
        out += lit[lp:]
        assert len(out) - start <= BLOCK_MAX
    return bytes(out)


# ---- the cases -----------------------------------------------------------------------------------------------------------
LL_EDGES = (0, 1, 15, 16, 17, 63, 64, 65, 129)
ML_EDGES = (3, 63, 64, 65, 129)
OFF_EDGES = (1, 2, 3, 7, 31, 32, 33, 63, 64, 65, 127, 129)


class _Block:
    """collects the sequences of one compressed block by real offsets; `pos` is the frame's output position"""

    def __init__(self, rng, pos=0):
        self.rng, self.pos, self.nlit, self.seqs = rng, pos, 0, []

    def seq(self, ll, ml, off):
        """a match at offset `off`; returns its `at`"""
        at = self.pos + ll
        assert 1 <= off <= at and ml >= 3, (ll, ml, off, at)
        self.seqs.append((ll, ml, off + 3))
        self.nlit += ll
        self.pos = at + ml
        return at

    def rep(self, ll, ml, code, off):
        """a match by repeat code; `off` is what the code resolves to (the caller knows; execute() checks the bytes)"""
        self.seqs.append((ll, ml, code))
        self.nlit += ll
        self.pos += ll + ml

    def done(self, tail=0, rle_value=None):
        n = self.nlit + tail
        self.pos += tail
        if rle_value is not None:
            return comp(bytes([rle_value]) * n, self.seqs, rle_literals=True)
        return comp(self.rng.integers(0, 256, n, dtype=np.uint8).tobytes(), self.seqs)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _seen_edge(name, kth, delta, moved):
    """the match number kth (0-based) of the first batch with off >= ml and its source end at seen + delta. moved: the
    match before it waits, so that `seen` is that match's `at`, not the first match's"""
    b = _Block(_rng(name))
    seen = b.seq(400, 16, 200)
    for k in range(1, kth - (1 if moved else 0)):
        at = b.pos + 5
        b.seq(5, 6, at - 9 * k)  # sources in the first literal run: nothing waits
    if moved:
        seen = b.seq(0, 12, 8)  # reads the match before it
    at, ml = b.pos + 7, 20
    b.seq(7, ml, at + ml - seen - delta)
    b.seq(2, 9, 30)
    return [b.done(tail=3)]


def _seen_overlap(name, kth):
    """off < ml as match kth of the first batch at the nearest distance, source end = seen + 3; kth = 64: as the first match
    of the second batch, source end = seen"""
    b = _Block(_rng(name))
    b.seq(400, 3, 200)
    for k in range(1, kth if kth == 64 else max(kth - 1, 1)):
        at = b.pos + 5
        b.seq(5, 6, at - 17 * (k % 20 + 1))
    if 1 < kth < 64:
        b.seq(0, 3, 2)  # waits: seen = its at, and the next match begins 3 above
    assert len(b.seqs) == kth
    b.seq(0, 70, 5)
    b.seq(1, 4, 66)
    return [b.done(tail=2)]


def _chain(name, nseq, ml, off):
    b = _Block(_rng(name))
    b.seq(max(256, off), ml, max(256, off) - 3)
    for _ in range(nseq - 1):
        b.seq(0, ml, off)
    return [b.done()]


def _overlap(name, off, ml):
    b = _Block(_rng(name))
    b.seq(200, 70, 150)
    b.seq(0, ml, off)
    b.seq(3, 10, 5)
    return [b.done(tail=1)]


def _own_literals(name, ll):
    b = _Block(_rng(name))
    b.seq(40, 5, 33)
    for off, ml in ((ll, 3 + ll % 5), (1, 5), (ll, ll + 70), (max(1, ll - 1), 64), (max(1, ll // 2), 3)):
        b.seq(ll, ml, off)  # sources inside the sequence's own literal run, short of it and beyond it by overlap
    return [b.done(tail=4)]


def _lit_pairs(name, rle_value=None):
    """every adjacent pairing of the literal-run edges; with RLE literals a raw block of random bytes goes first and the
    matches reach into it, so that the content is not one byte value"""
    rng = _rng(name)
    blocks, pos = [], 0
    if rle_value is not None:
        blocks.append(raw(rng.integers(0, 256, 700, dtype=np.uint8).tobytes()))
        pos = 700
    b = _Block(rng, pos)
    b.seq(300, 8, 100)
    for a in LL_EDGES:
        for c in LL_EDGES:
            for ll in (a, c):
                at = b.pos + ll
                b.seq(ll, 4, at - int(rng.integers(0, 600)) if rle_value is not None else int(rng.integers(1, 200)))
    return blocks + [b.done(tail=5, rle_value=rle_value)]


def _lit_batch(name, lls, tail, rle_value=None):
    rng = _rng(name)
    blocks, pos = [], 0
    if rle_value is not None:
        blocks.append(raw(rng.integers(0, 256, 300, dtype=np.uint8).tobytes()))
        pos = 300
    b = _Block(rng, pos)
    for k, ll in enumerate(lls):
        at = b.pos + ll
        b.seq(ll, 3 + k % 7, at - int(rng.integers(0, 290)) if rle_value is not None else int(rng.integers(1, max(2, min(at, 150)))))
    return blocks + [b.done(tail=tail, rle_value=rle_value)]


def _batch(name, nseq, ll):
    """nseq sequences; the first match of every batch but the first reads the last match of the batch before"""
    b = _Block(_rng(name))
    b.seq(200, 10, 77)
    for k in range(1, nseq):
        if k % 64 == 0:
            b.seq(ll, 10, ll + 7)  # 7 bytes into the match before, then its own literals
        else:
            at = b.pos + 3
            b.seq(3, 10, at - (k * 13) % 180)
    return [b.done(tail=2)]


def _blocks(name, before, ll):
    """the first match of a block reaches into what the block before ended with"""
    rng = _rng(name)
    head = raw(rng.integers(0, 256, 300, dtype=np.uint8).tobytes())
    if before == "match":
        b0 = _Block(rng, 300)
        b0.seq(20, 9, 250)
        b0.seq(4, 40, 100)
        first, pos = [head, b0.done()], b0.pos
    elif before == "raw":
        first, pos = [head], 300
    else:
        first, pos = [head, rle(0x3C, 40)], 340
    b = _Block(rng, pos)
    b.seq(ll, 30, 50 + ll)  # 50 bytes back from the block's first byte: across an RLE block's start, inside a match
    b.seq(0, 12, ll + 30 + 3)  # the last three bytes of the block before, then on into this one
    b.seq(2, 6, 4)
    return first + [b.done(tail=1)]


def _rep_fresh(name):
    b = _Block(_rng(name))
    b.rep(20, 5, 1, 1)    # 1, 4, 8
    b.rep(3, 6, 2, 4)     # -> 4, 1, 8
    b.rep(9, 4, 3, 8)     # -> 8, 4, 1
    b.rep(0, 7, 3, 7)     # literal length 0, code 3: the first offset less one -> 7, 8, 4
    b.rep(0, 3, 1, 8)     # literal length 0, code 1: the second -> 8, 7, 4
    b.rep(0, 5, 2, 4)     # literal length 0, code 2: the third -> 4, 8, 7
    b.rep(2, 8, 1, 4)
    return [b.done(tail=3)]


def _seeded(name):
    rng = _rng(name)
    blocks, pos = [], 0
    for _ in range(int(rng.integers(1, 4))):
        kind = int(rng.integers(0, 8))
        if kind == 0:
            n = int(rng.integers(1, 400))
            blocks.append(raw(rng.integers(0, 256, n, dtype=np.uint8).tobytes()))
            pos += n
        elif kind == 1 and pos:
            n = int(rng.integers(1, 200))
            blocks.append(rle(int(rng.integers(0, 256)), n))
            pos += n
        b = _Block(rng, pos)
        for k in range(int(rng.integers(1, 301))):
            ll = int(rng.choice(LL_EDGES))
            ml = int(rng.choice(ML_EDGES + (1000,), p=(0.24, 0.19, 0.19, 0.19, 0.18, 0.01)))
            if b.pos + ll == 0:
                ll = 17
            if b.pos - pos + ll + ml > BLOCK_MAX - 200:
                break
            off = int(rng.choice(OFF_EDGES + (ml - 1, ml + 1))) if rng.integers(0, 4) else int(rng.integers(1, b.pos + ll + 1))
            b.seq(ll, ml, max(1, min(off, b.pos + ll)))
        use_rle = pos > 0 and int(rng.integers(0, 4)) == 0
        blocks.append(b.done(tail=int(rng.choice((0, 1, 65))), rle_value=int(rng.integers(0, 256)) if use_rle else None))
        pos = b.pos
    return blocks


def _stale(name):
    rng = _rng(name)
    if name == "stale-treeless":
        # one literal from one byte of ones: under any Huffman table that was left behind this is the symbol of the
        # shortest code, so a decoder that kept the table of the frame before would call the frame OK
        return [treeless(1, b"\xff")]
    mode = {"stale-ll-repeat": 3 << 6, "stale-of-repeat": 3 << 4, "stale-ml-repeat": 3 << 2}[name]
    b = _Block(rng)
    b.seq(60, 9, 31)
    b.seq(5, 4, 2)
    blk = b.done(tail=6)
    return [comp(blk["lit"], blk["seqs"], modes=mode)]


def _declared(blocks):
    """what a stale-* frame declares: the size it would have if the table it asks for were there"""
    b = blocks[0]
    return b["regen"] if b["kind"] == "treeless" else len(execute([comp(b["lit"], b["seqs"])]))


_cache = {}


def _plan():
    """(name, status, builder) of every case, in the order of the golden file"""
    out = []

    def add(name, fn, *a, status=OK):
        out.append((name, status, lambda: fn(name, *a)))

    for kth in (1, 39):
        for delta, word in ((0, "at"), (1, "past")):
            add("seen-edge-k%d-%s" % (kth, word), _seen_edge, kth, delta, False)
        add("seen-edge-k%d-overlap" % kth, _seen_overlap, kth)
    for delta, word in ((0, "at"), (1, "past")):
        add("seen-edge-k39-moved-%s" % word, _seen_edge, 39, delta, True)
    add("seen-edge-k64-overlap", _seen_overlap, 64)
    for nseq in (64, 200):
        for ml in ML_EDGES:
            for off in sorted(set(OFF_EDGES + (ml - 1, ml + 1))):
                if off < 2 * ml:  # the source lies wholly or partly in the previous match's output
                    tag = "-aligned" if (ml - off) % 64 == 0 else ""  # the byte's loading lane is its storing lane
                    add("chain-%d-ml%d-off%d%s" % (nseq, ml, off, tag), _chain, nseq, ml, off)
    for off in (1, 2, 3, 7, 8, 63, 64, 65):
        for ml in sorted({max(off + 1, 3), 64, 65, 129, 1000}):  # (a match has 3 bytes at the least)
            if off < ml:
                add("overlap-off%d-ml%d" % (off, ml), _overlap, off, ml)
    for ll in (1, 16, 17, 65):
        add("own-literals-ll%d" % ll, _own_literals, ll)
    add("lit-edge-pairs", _lit_pairs)
    add("lit-edge-pairs-rle", _lit_pairs, 0xE7)
    add("lit-edge-64x16", _lit_batch, [16] * 64, 0)
    add("lit-edge-64x16-rle", _lit_batch, [16] * 64, 0, 0x5B)
    for at in (0, 31, 63):
        lls = [int(v) for v in np.random.default_rng(at).integers(1, 17, 64)]
        lls[at] = 129
        add("lit-edge-one-long-at%d" % at, _lit_batch, lls, 1)
        add("lit-edge-one-long-at%d-rle" % at, _lit_batch, lls, 1, 0x11)
    for tail in (0, 1, 65):
        add("lit-edge-tail%d" % tail, _lit_batch, [17, 0, 1, 9], tail)
        add("lit-edge-tail%d-rle" % tail, _lit_batch, [17, 0, 1, 9], tail, 0xC4)
    for nseq in (1, 63, 64, 65, 128, 129):
        for ll in (0, 3):
            add("batch-n%d-ll%d" % (nseq, ll), _batch, nseq, ll)
    for before in ("match", "raw", "rle"):
        for ll in (0, 1):
            add("blocks-after-%s-ll%d" % (before, ll), _blocks, before, ll)
    add("rep-fresh", _rep_fresh)
    for name in ("stale-treeless", "stale-ll-repeat", "stale-of-repeat", "stale-ml-repeat"):
        out.append((name, BAD_FRAME, (lambda n: lambda: _stale(n))(name)))
    for k in range(24):
        add("seeded-%02d" % k, _seeded)
    assert len({n for n, _, _ in out}) == len(out)
    return out


def cases():
    """every case: dicts with name, status, blocks, frame, content, length, sha256: computed once, shared, not to be changed"""
    if "cases" not in _cache:
        out = []
        for name, status, build in _plan():
            blocks = build()
            content = execute(blocks) if status == OK else b""
            out.append({"name": name, "status": status, "blocks": blocks, "frame": frame(blocks, len(content) if status == OK else _declared(blocks)),
                        "content": content, "length": len(content), "sha256": hashlib.sha256(content).digest()})
        _cache["cases"] = out
    return _cache["cases"]


def family(name):
    return name.split("-")[0]


# The libzstd fixture (tests/golden/zstd_v1*.npz) that goes in front of the stale-* frames on a workgroup: one compressed
# block whose literals are four Huffman streams under a described tree and whose three sequence tables are described, by
# the coverage word of the CPU run over that case alone (tests/test_zstd_seq_native.py asserts it)
TABLE_LEAVING = "text-60000-level1"
TABLE_LEAVING_BRANCHES = ("weights_fse", "ll_fse", "of_fse", "ml_fse")
TABLE_LEAVING_NOT = ("many_blocks",)
