"""zstd frames with Huffman-compressed literals and described sequence tables, built bit by bit: for the literal half of the
device decoder (tests/test_gpu_zstd_huf.py: the four streams on four lanes, the table edges, the end of a stream, treeless
blocks) and for fse_read_norm / fse_build as compiled for the device, and for the CPU run of the same format core
(tests/test_zstd_huf_native.py). Pure Python: no libzstd, nothing from the package. The frame, the block header, the
state picking and the sequence bit stream are those of tests/zstd_seq_inputs.py, by import.

  Huf(weights)          the code of a full weight list, assigned as a decoder assigns it: weight 1 first, then by symbol
  huf_bits(...)         one backward bit stream, with a chosen number of spare zero bits below it, or cut short
  direct_tree / fse_tree / fse_describe    the tree description by direct weights and by FSE-compressed weights (two
                        interleaved states written backwards), and the description of a normalised distribution as the
                        forward bit stream of RFC 8878 4.1.1, which also serves the three sequence tables
  literals(...)         the literals section: one or four streams, every size format, with a tree (type 2) or treeless (3)
  Frame                 the blocks of one frame and the tables in force between them: each of the three sequence tables is
                        predefined, RLE, described or repeated, and the sequence bits are coded under what is in force
  cases()               the family; tests/golden/make_zstd_huf_golden.py sets it against libzstd where that loads

Expected contents are known by construction: the literals are the symbols that were encoded, the sequences go through
zstd_seq_inputs.execute. The status of a refused frame is by the rule named beside its case (RFC 8878, or a stated limit
of zstd_decode.h). Nothing here is derived from the decoder under test.

Every refused frame declares at most 4096 bytes of content, so that the room it gets decides nothing."""
import hashlib
import struct
import zlib

import numpy as np

import zstd_seq_inputs as S
from zstd_seq_inputs import BAD_FRAME, OK

HUF_LOG_MAX = 12       # kHufLogMax: the longest code taken (an encoder stops at 11)
LIT_MAX = 128 << 10    # kLitMax = Block_Maximum_Size: an 18-bit size field cannot declare more than twice that, and a
#                        block of more than LIT_MAX literals regenerates more than a block may: not forced here
PREDEF = ((S._LL, S.LL_LOG), (S._OF, S.OF_LOG), (S._ML, S.ML_LOG))
MAX_SYM = (35, 31, 52)  # the last symbol of literal lengths, offsets (what the decoder supports) and match lengths
MAX_LOG = (9, 8, 9)


# ---- Huffman ---------------------------------------------------------------------------------------------------------------
def code_lengths(nsym, maxlen, minlen=1):
    """a complete set of nsym code lengths, the shortest minlen and the longest exactly maxlen, skewed: the deepest leaf
    that may still be split is split first"""
    lens = [minlen] * ((1 << minlen) - 1) + list(range(minlen + 1, maxlen)) + [maxlen, maxlen]
    if maxlen == minlen:
        lens = [minlen] * (1 << minlen)
    assert len(lens) <= nsym <= 1 << maxlen, (nsym, maxlen, minlen)
    while len(lens) < nsym:
        i = max((k for k, v in enumerate(lens) if v < maxlen), key=lambda k: lens[k])
        lens[i] += 1
        lens.append(lens[i])
    assert sum(1 << (maxlen - v) for v in lens) == 1 << maxlen
    return lens


class Huf:
    """weights[s] of every symbol 0..last (the last one not zero) -> code[s] = (value, bits), most significant bit first"""

    def __init__(self, weights):
        self.weights = list(weights)
        total = sum(1 << (w - 1) for w in self.weights if w)
        self.log = total.bit_length() - 1
        assert total == 1 << self.log and self.weights[-1], "not a complete code"
        self.code, at = {}, 0
        for w in range(1, self.log + 1):  # the decoder's table order: weight 1 (the longest codes) first, then by symbol
            for s, ws in enumerate(self.weights):
                if ws == w:
                    self.code[s] = (at >> (w - 1), self.log + 1 - w)
                    at += 1 << (w - 1)
        assert at == 1 << self.log
        self.text = {s: format(v, "0%db" % nb) for s, (v, nb) in self.code.items()}
        self.symbols = sorted(self.code)

    def draw(self, rng, n):
        """n symbols: every symbol once where there is room, the rest by the code's own probabilities"""
        p = np.array([2.0 ** -self.code[s][1] for s in self.symbols])
        out = rng.choice(self.symbols, size=n, p=p / p.sum())
        if n >= len(self.symbols):
            out[rng.permutation(n)[:len(self.symbols)]] = self.symbols
        return np.asarray(out, dtype=np.uint8).tobytes()


def make_huf(rng, alphabet, maxlen, minlen=1):
    """a code over the given symbols with the given longest code, the lengths dealt to the symbols by rng"""
    alphabet = sorted(alphabet)
    lens = code_lengths(len(alphabet), maxlen, minlen)
    weights = [0] * (alphabet[-1] + 1)
    for s, k in zip(alphabet, rng.permutation(len(lens))):
        weights[s] = maxlen + 1 - lens[k]
    return Huf(weights)


def huf_bits(huf, syms, spare=0, short=0):
    """the backward bit stream of syms: the first symbol's code directly below the end mark. spare: zero bits below the
    last code, which no symbol needs; short: bits of the last code that are missing"""
    s = "1" + "".join(huf.text[x] for x in syms)
    assert short < len(s)
    s = s[:len(s) - short] + "0" * spare
    return int(s, 2).to_bytes((len(s) + 7) // 8, "little")


def direct_tree(weights):
    """weights of the symbols 0 .. n-1 as 4-bit fields; the weight of symbol n is implied"""
    n = len(weights)
    assert 1 <= n <= 128 and all(0 <= w < 16 for w in weights)
    w = list(weights) + [0]
    return bytes([127 + n]) + bytes(w[i] << 4 | w[i + 1] for i in range(0, n, 2))


def normalise(hist, log, cap=None, less_than_one=()):
    """{symbol: count} -> a distribution over 0 .. max symbol that sums to 1 << log: every counted symbol gets 1 at the
    least (-1, "less than one", for those named), none more than cap, the rest by the counts"""
    size = 1 << log
    cap = cap or size
    norm = {s: 1 for s in hist}
    left = size - len(norm)
    assert left >= 0 and cap * sum(1 for s in hist if s not in less_than_one) + len(less_than_one) >= size
    while left:
        s = max((s for s in hist if s not in less_than_one and norm[s] < cap), key=lambda s: ((hist[s] + 1) / norm[s], -s))
        norm[s] += 1
        left -= 1
    out = [0] * (max(hist) + 1)
    for s, v in norm.items():
        out[s] = -1 if s in less_than_one else v
    return out


def fse_describe(norm, log, stop_early=False):
    """RFC 8878 4.1.1, a forward bit stream: 4 bits of accuracy log - 5, then per symbol its probability + 1 in a field
    whose width follows what is left to give out, and behind a zero the 2-bit counts of further zeros. A field holds at
    most what is left + 1, so a description cannot overshoot; it can only fall short, when the symbols run out.
    stop_early: norm does not sum to 1 << log (a description that falls short)"""
    acc, nbit = log - 5, 4
    remaining, s = 1 << log, 0
    assert stop_early or sum(abs(v) for v in norm) == remaining
    while s < len(norm) and remaining > 0:
        bits = (remaining + 1).bit_length()
        lower, threshold = (1 << (bits - 1)) - 1, (1 << bits) - 1 - (remaining + 1)
        x = norm[s] + 1
        assert 0 <= x <= remaining + 1
        if x < threshold:
            field, w = x, bits - 1
        elif x <= lower:
            field, w = x, bits
        else:
            field, w = x + threshold, bits
        acc |= field << nbit
        nbit += w
        remaining -= abs(norm[s])
        s += 1
        if x == 1:  # probability 0: how many more zeros follow, in 2-bit counts, 3 meaning "and another count"
            run = 0
            while s + run < len(norm) and norm[s + run] == 0:
                run += 1
            assert s + run < len(norm) or stop_early
            s += run
            while run >= 3:
                acc |= 3 << nbit
                nbit += 2
                run -= 3
            acc |= run << nbit
            nbit += 2
    return acc.to_bytes((nbit + 7) // 8, "little")


def fse_tree(weights, log, norm=None, stream=True):
    """the weights of the symbols 0 .. n-1, FSE-compressed: the description of their distribution, then two interleaved
    states (even weights on the first, odd on the second) written backwards. The stream ends where the state that has just
    given the last weight but one cannot be updated; the last weight is the other state's symbol"""
    n = len(weights)
    assert n >= 2
    if norm is None:
        hist = {}
        for w in weights:
            hist[w] = hist.get(w, 0) + 1
        if len(hist) == 1:
            hist[0 if 0 not in hist else 1] = 0
        norm = normalise(hist, log, cap=1 << (log - 1))  # (no state of 0 bits; hufsyms-dominant has them)
    body = fse_describe(norm, log)
    if stream:
        table = S._fse_table(norm, log)
        sa, ba = S._states(table, list(weights[0::2]))
        sb, bb = S._states(table, list(weights[1::2]))
        assert table[sa[-1]][1] > 0 and table[sb[-1]][1] > 0
        fields = [(sa[0], log), (sb[0], log)] + [(ba, bb)[i & 1][i // 2] for i in range(n - 2)]
        v, total = 1, 0
        for val, nb in fields:
            assert 0 <= val < 1 << nb
            v = v << nb | val
            total += nb
        body += v.to_bytes(total // 8 + 1, "little")
    assert len(body) < 128, len(body)
    return bytes([len(body)]) + body


def literals(huf, lits, streams, tree, fmt=None, spare=(0, 0, 0, 0), short=(0, 0, 0, 0), empty=(), jump_add=(0, 0, 0), cut=None):
    """the literals section of lits under huf. tree: the tree description's bytes, or None for a treeless section.
    fmt: 3, 4 or 5 header bytes (the smallest that fits by default). Per stream: spare and short as in huf_bits, empty: the
    streams of no bytes at all; jump_add: added to the jump table's entries; cut: the bytes kept behind the tree"""
    regen = len(lits)
    if streams == 1:
        data = b"" if 0 in empty else huf_bits(huf, lits, spare[0], short[0])
    else:
        seg = (regen + 3) // 4
        parts = [b"" if k in empty else huf_bits(huf, lits[k * seg:(k + 1) * seg if k < 3 else regen], spare[k], short[k]) for k in range(4)]
        data = struct.pack("<3H", *(len(parts[k]) + jump_add[k] for k in range(3))) + b"".join(parts)
    if cut is not None:
        data = data[:cut]
    body = (tree or b"") + data
    if fmt is None:
        fmt = 3 if max(regen, len(body)) < 1 << 10 else 4 if max(regen, len(body)) < 1 << 14 else 5
    bits = {3: 10, 4: 14, 5: 18}[fmt]
    assert regen < 1 << bits and len(body) < 1 << bits and (streams == 4 or fmt == 3)
    sf = {3: 0 if streams == 1 else 1, 4: 2, 5: 3}[fmt]
    head = (2 if tree is not None else 3) | sf << 2 | regen << 4 | len(body) << (4 + bits)
    return head.to_bytes(fmt, "little") + body


# ---- sequence tables and frames -------------------------------------------------------------------------------------------
def rle_table(sym):
    return ("rle", sym)


def fse_table(norm, log):
    return ("fse", list(norm), log)


class Frame:
    """the blocks of one frame; keeps the Huffman code and the three sequence tables in force, as a decoder does"""

    def __init__(self):
        self.blocks, self.huf, self.tabs = [], None, [None, None, None]

    def raw(self, data):
        self.blocks.append(S.raw(data))

    def rle(self, value, n):
        self.blocks.append(S.rle(value, n))

    def sequences(self, seqs, specs=(None, None, None), pad=0, bad_desc=None):
        """the sequences section. specs, per table: None (predefined), ("rle", symbol), ("fse", norm, log) or "repeat".
        bad_desc: (modes, bytes) written as they are, for a table nobody may accept; the bits are coded as predefined"""
        if not seqs:
            return S._sequences_section((), 0, 0)
        if bad_desc is not None:
            return S._sequences_section(seqs, bad_desc[0], pad, desc=bad_desc[1])
        modes, desc, tabs = 0, b"", []
        for k, sp in enumerate(specs):
            if sp is None:
                mode, t = 0, PREDEF[k]
            elif sp == "repeat":
                mode, t = 3, self.tabs[k]
                assert t is not None
            elif sp[0] == "rle":
                mode, t = 1, ([(sp[1], 0, 0)], 0)
                desc += bytes([sp[1]])
            else:
                mode, t = 2, (S._fse_table(sp[1], sp[2]), sp[2])
                desc += fse_describe(sp[1], sp[2])
            modes |= mode << (6 - 2 * k)
            tabs.append(t)
        self.tabs = tabs
        return S._sequences_section(seqs, modes, pad, tables=tabs, desc=desc)

    def block(self, lits, seqs=(), huf=None, streams=4, tree="direct", log=6, seq_bytes=None, lit_bytes=None, specs=(None, None, None),
              bad_desc=None, **kw):
        """a compressed block. huf: a new code, described by `tree` ("direct", "fse", or the description's own bytes); None:
        treeless under the code in force. tree="raw": raw literals. lit_bytes: the literals section as given"""
        if tree == "raw":
            section = S._literals_section(bytes(lits), False)
        elif lit_bytes is not None:
            section = lit_bytes
        else:
            if huf is not None:
                self.huf = huf
                if tree == "direct":
                    tree = direct_tree(huf.weights[:-1])
                elif tree == "fse":
                    tree = fse_tree(huf.weights[:-1], log)
            else:
                tree = None
                assert self.huf is not None
            section = literals(self.huf, lits, streams, tree, **kw)
        payload = section + (seq_bytes if seq_bytes is not None else self.sequences(list(seqs), specs, bad_desc=bad_desc))
        # ("seq_logs": the accuracy logs of the three tables in force behind this block, None before any was set)
        self.blocks.append(dict(S.comp(lits, seqs), payload=payload, seq_logs=tuple(t and t[1] for t in self.tabs)))
        return self


def _rng(name):
    return np.random.default_rng(zlib.crc32(("huf:" + name).encode()))


def seqs_for(rng, n, pos, ll_codes, of_codes, ml_codes):
    """n sequences whose codes come from the given sets, at output position pos: (sequences, literals needed, new position).
    Offset codes 2 and up only (new offsets, no repeat codes), each offset inside what has been produced"""
    seqs, nlit = [], 0
    for _ in range(n):
        lc, oc, mc = int(rng.choice(sorted(ll_codes))), int(rng.choice(sorted(of_codes))), int(rng.choice(sorted(ml_codes)))
        ll = S.LL_BASE[lc] + int(rng.integers(0, 1 << S.LL_BITS[lc]))
        ml = S.ML_BASE[mc] + int(rng.integers(0, 1 << S.ML_BITS[mc]))
        assert oc >= 2 and (1 << oc) - 3 <= pos + ll, (oc, pos, ll)
        ov = min((1 << oc) + int(rng.integers(0, 1 << oc)), pos + ll + 3)
        seqs.append((ll, ml, ov))
        nlit += ll
        pos += ll + ml
    return seqs, nlit, pos


def norm_for(rng, codes, log, also=(), less_than_one=()):
    """a distribution with accuracy log `log` over the codes (and the symbols in `also`, which no sequence uses)"""
    hist = {c: int(rng.integers(1, 20)) for c in set(codes) | set(also)}
    return normalise(hist, log, less_than_one=less_than_one)


# ---- the cases -----------------------------------------------------------------------------------------------------------
SKEWED = (0x20, 0x65, 0x74, 0x61, 0x6F, 0x0A, 0x2C, 0x41, 0x7F)  # a small alphabet with a spread of code lengths
_shared = {}


def table12():
    """a code of 256 symbols with codes of 12 bits, by FSE-compressed weights: what hufsyms-fse256-max12 leaves behind and
    treeless-stale-4streams is coded under"""
    if "t12" not in _shared:
        _shared["t12"] = make_huf(_rng("table12"), range(256), 12)
    return _shared["t12"]


def _one(name, huf, n, streams, tree="direct", log=6, **kw):
    f = Frame()
    f.block(huf.draw(_rng(name), n), huf=huf, streams=streams, tree=tree, log=log, **kw)
    return f.blocks


def _hufmax(name, maxlen, streams):
    rng = _rng(name)
    nsym = {1: 2, 2: 3, 8: 40, 11: 100, 12: 120, 13: 128}[maxlen]
    # (13: no weight above 12 among them, the shortest code has 2 bits: refused for the table's depth alone)
    huf = make_huf(rng, rng.permutation(129)[:nsym], maxlen, 2 if maxlen == 13 else 1)
    return _one(name, huf, 300, streams)


def _hufsyms(name, kind):
    rng = _rng(name)
    if kind == "sym2":  # one direct weight: an odd count
        return _one(name, make_huf(rng, (0, 1), 1), 260, 1)
    if kind == "sym3":  # two direct weights: an even count
        return _one(name, make_huf(rng, (0, 1, 2), 2), 260, 4)
    if kind in ("direct127", "direct128"):  # 128 and 129 symbols: the most a header byte can name
        return _one(name, make_huf(rng, range(int(kind[6:]) + 1), 9), 400, 4)
    if kind in ("fse129", "fse255", "fse256"):  # 128 weights end on the second state, 254 too, 255 on the first
        return _one(name, make_huf(rng, range(int(kind[3:])), 10), 600, 4, tree="fse")
    if kind == "fse256-max12":
        return _one(name, table12(), 700, 4, tree="fse")
    if kind in ("end-first", "end-second"):  # 5 weights: the last from the first state; 6: from the second
        return _one(name, make_huf(rng, range(6 if kind == "end-first" else 7), 4), 200, 1, tree="fse", log=5)
    if kind in ("log5", "log6", "log7"):  # the accuracy log of the weights' table: 7 is above what the format allows (6)
        return _one(name, make_huf(rng, range(40), 8), 300, 4, tree="fse", log=int(kind[3:]))
    if kind == "weights256":  # 256 weights name 257 symbols
        lens = code_lengths(257, 11)
        body = fse_tree([12 - v for v in lens[:256]], 6)
        return _one(name, make_huf(rng, range(256), 11), 300, 1, tree=body)
    if kind == "dominant":  # one weight holds most of the table: states of 0 bits, whose update cannot end the stream
        huf = make_huf(rng, range(200), 9)
        hist = {w: huf.weights[:-1].count(w) for w in set(huf.weights[:-1])}
        norm = normalise(hist, 6)
        assert max(norm) > 32
        return _one(name, huf, 400, 4, tree=fse_tree(huf.weights[:-1], 6, norm=norm))
    assert kind == "sparse"  # long zero runs among the weights
    return _one(name, make_huf(rng, (3, 70, 71, 200, 255), 3), 300, 4, tree="fse", log=5)


def _hufbad(name, kind):
    rng = _rng(name)
    good = make_huf(rng, range(8), 4)  # what the stream is coded under: it would decode if the table were taken
    if kind == "incomplete":  # 4 + 1 = 5 of 8: what is left, 3, is no power of two
        tree = direct_tree([3, 1])
    elif kind == "weight13":
        tree = direct_tree([13, 1, 1])
    elif kind == "all-zero":
        tree = direct_tree([0, 0, 0, 0])
    elif kind == "incomplete-fse":
        tree = fse_tree([3, 1, 0, 0, 3], 5)
    elif kind == "fse-no-stream":  # the description takes all of the header's bytes: cons >= h
        tree = fse_tree(good.weights[:-1], 5, stream=False)
    elif kind == "fse-header-0":
        tree = b"\x00"
    else:
        tree = None
    if kind == "direct-overlong":  # 100 weights named, 10 bytes there: the header reaches beyond the section
        sec = (2 | 300 << 4 | 11 << 14).to_bytes(3, "little") + bytes([127 + 100]) + bytes([0x11] * 10)
        return Frame().block(good.draw(rng, 300), lit_bytes=sec).blocks
    if kind == "fse-overlong":
        sec = (2 | 300 << 4 | 11 << 14).to_bytes(3, "little") + bytes([100]) + fse_tree(good.weights[:-1], 5)[1:11]
        return Frame().block(good.draw(rng, 300), lit_bytes=sec).blocks
    f = Frame()
    f.huf = good
    lits = good.draw(rng, 300)
    return f.block(lits, lit_bytes=literals(good, lits, 1, tree)).blocks


def _hufend(name, maxlen, streams, which, spare, short):
    rng = _rng("hufend-%d-%d" % (maxlen, streams))  # one code and one content per (maxlen, streams): only the end differs
    huf = make_huf(rng, range(maxlen + 6), maxlen)
    sp, sh = [0] * 4, [0] * 4
    sp[which], sh[which] = spare, short
    return _one("hufend-%d-%d" % (maxlen, streams), huf, 301, streams, spare=sp, short=sh)


def _hufgeom(name, kind, arg=0):
    rng = _rng(name)
    huf = make_huf(rng, SKEWED, 5)
    if kind == "regen":  # 5: three streams of 2 symbols are more than 5
        return _one(name, huf, arg, 4)
    if kind == "fmt":
        return _one(name, huf, arg[0], arg[1], fmt=arg[2])
    if kind == "jump":  # the three lengths of the jump table sum to one more than the bytes behind it
        f = Frame()
        lits = huf.draw(rng, 300)
        last = len(huf_bits(huf, lits[225:]))
        return f.block(lits, huf=huf, jump_add=(0, 0, last + 1)).blocks
    if kind == "empty":  # a stream of no bytes has no end mark
        return _one(name, huf, 300, 4, empty=(arg,))
    if kind == "empty-1stream":
        return _one(name, huf, 300, 1, empty=(0,))
    assert kind == "dlen5"  # five bytes behind the tree: no room for a jump table
    return _one(name, huf, 300, 4, cut=5)


def _treeless(name, kind):
    rng = _rng(name)
    f = Frame()
    huf = make_huf(rng, SKEWED, 6)
    if kind in ("1to4", "4to1"):
        a, b = (1, 4) if kind == "1to4" else (4, 1)
        f.block(huf.draw(rng, 200), huf=huf, streams=a)
        f.block(huf.draw(rng, 333), streams=b)
        f.block(huf.draw(rng, 97), streams=a)
    elif kind in ("across-raw", "across-rle", "across-rawlit"):
        f.block(huf.draw(rng, 200), huf=huf, streams=4)
        if kind == "across-raw":
            f.raw(rng.integers(0, 256, 100, dtype=np.uint8).tobytes())
        elif kind == "across-rle":
            f.rle(0x77, 100)
        else:
            seqs, nlit, _ = seqs_for(rng, 12, 200, (0, 3, 9), (2, 4, 6), (0, 5, 30))
            f.block(rng.integers(0, 256, nlit + 3, dtype=np.uint8).tobytes(), seqs, tree="raw")
        f.block(huf.draw(rng, 250), streams=4)
        f.block(huf.draw(rng, 50), streams=1)
    elif kind == "after-max12":
        huf = table12()
        f.block(huf.draw(rng, 600), huf=huf, tree="fse")
        f.block(huf.draw(rng, 500), streams=4)
        f.block(huf.draw(rng, 300), streams=1)
    elif kind == "overrun":  # the second block's stream is one bit short under the kept table
        f.block(huf.draw(rng, 200), huf=huf, streams=4)
        f.block(huf.draw(rng, 200), streams=4, short=(0, 0, 1, 0))
    else:
        assert kind == "stale-4streams"  # no table in this frame: RFC 8878 3.1.1.3.1.1, Treeless_Literals_Block needs one
        f.huf = table12()
        f.block(f.huf.draw(rng, 700), streams=4)
    return f.blocks


def _fill_to(b, target, rng):
    """sequences with literal runs from the edges until the literals used reach target exactly"""
    k = 0
    while b.nlit < target:
        ll = min(S.LL_EDGES[k % len(S.LL_EDGES)], target - b.nlit)
        k += 1
        at = b.pos + ll
        b.seq(ll, 3 + k % 5, int(rng.integers(1, at + 1)) if at else 1)


def _huflit(name, streams):
    """four streams of seg = 400 literals. A literal run of 2 spans the first seam (399 .. 401), one of 129 the second, every
    pair of the literal-run edges lies in between, and the tail behind the last sequence spans the third"""
    rng = _rng(name)
    huf = make_huf(rng, SKEWED, 7)
    seg = 400 if streams == 4 else 250
    b = S._Block(rng)
    b.seq(seg - 1, 5, 100)
    b.seq(2, 4, 7)
    for a in S.LL_EDGES:
        for c in S.LL_EDGES[:4]:
            for ll in (a, c):
                if b.nlit + ll < 2 * seg - 40:
                    b.seq(ll, 4, int(rng.integers(1, b.pos + ll + 1)))
    _fill_to(b, 2 * seg - 40, rng)
    b.seq(129, 64, 33)
    _fill_to(b, 3 * seg - 9, rng)
    lits = huf.draw(rng, 4 * seg)
    return Frame().block(lits, b.seqs, huf=huf, streams=streams).blocks


_HEAD = 3000  # a raw block in front, so that every offset code up to 11 has something to reach


def _seq_frame(name):
    rng = _rng(name)
    f = Frame()
    f.raw(rng.integers(0, 256, _HEAD, dtype=np.uint8).tobytes())
    return rng, f


def _bad_table(name, which, mode, desc, cut=0):
    """one block whose table number `which` nobody may accept: the frame is refused before a byte of content is stored. The
    sequences are coded under the predefined tables; cut: bytes of the section dropped behind the description"""
    rng = _rng(name + "/block")
    seqs, nlit, _ = seqs_for(rng, 9, 205, (0, 2, 7), (2, 3, 5), (0, 1, 9))
    seqs = [(200, 5, 10 + 3)] + seqs
    sec = S._sequences_section(seqs, mode << (6 - 2 * which), 0, desc=desc)
    if cut:
        sec = sec[:2 + len(desc) - cut]
    return Frame().block(rng.integers(0, 256, 200 + nlit, dtype=np.uint8).tobytes(), seqs, tree="raw", seq_bytes=sec).blocks


def _tab_log(name, which, log):
    """one table described with the given accuracy log (the other two predefined); above the table's limit: refused"""
    rng, f = _seq_frame(name)
    sets = [(0, 2, 7, 16, 20), (2, 3, 5, 8), (0, 1, 9, 33, 38)]
    if log > MAX_LOG[which]:
        return _bad_table(name, which, 2, fse_describe(norm_for(rng, sets[which], log), log))
    seqs, nlit, _ = seqs_for(rng, 30, _HEAD, *sets)
    specs = [None, None, None]
    specs[which] = fse_table(norm_for(rng, sets[which], log, also=(MAX_SYM[which] - 1,)), log)
    return f.block(rng.integers(0, 256, nlit + 2, dtype=np.uint8).tobytes(), seqs, tree="raw", specs=specs).blocks


def _tab_lto(name):
    """"less than one" probabilities in all three tables, on symbols that sequences use and on symbols that none does"""
    rng, f = _seq_frame(name)
    sets = [(0, 2, 7, 16, 20), (2, 3, 5, 8), (0, 1, 9, 33, 38)]
    seqs, nlit, _ = seqs_for(rng, 40, _HEAD, *sets)
    specs = [fse_table(norm_for(rng, sets[k], 6, also=(MAX_SYM[k], 11), less_than_one=(sets[k][1], sets[k][3], MAX_SYM[k])), 6) for k in range(3)]
    huf = make_huf(rng, SKEWED, 4)
    return f.block(huf.draw(rng, nlit + 5), seqs, huf=huf, streams=1, specs=specs).blocks


def _tab_zero_runs(name):
    """gaps of 2, 3, 4, 6 and 7 zeros between the symbols that are there. The first zero of a gap is written as a probability,
    the rest as 2-bit counts behind it: (1) for 2 zeros, (2) for 3, (3, 0) for 4, (3, 2) for 6 and (3, 3, 0) for 7: the
    last three go on after a count of 3"""
    rng, f = _seq_frame(name)
    ll, of, ml = (0, 4, 11, 19), (2, 7, 11), (0, 5, 9, 17)  # gaps: 3, 6, 7 | 4, 3 | 4, 3, 7
    seqs, nlit, _ = seqs_for(rng, 40, _HEAD, ll, of, ml)
    specs = [fse_table(norm_for(rng, ll, 5), 5), fse_table(norm_for(rng, of, 5), 5), fse_table(norm_for(rng, ml, 7), 7)]
    return f.block(rng.integers(0, 256, nlit, dtype=np.uint8).tobytes(), seqs, tree="raw", specs=specs).blocks


def _tab_last(name, which, past, by):
    """a description that names the table's last symbol (OK), or one symbol more (refused): by a probability, or by a zero run
    that ends behind it"""
    rng, f = _seq_frame(name)
    sets = [(0, 2, 7), (2, 3, 5), (0, 1, 9)]
    seqs, nlit, _ = seqs_for(rng, 10, _HEAD, *sets)
    last = MAX_SYM[which] + (1 if past else 0)
    if by == "proba":
        norm = norm_for(rng, sets[which], 6, also=(last,))
    else:  # ... 0 behind the last used symbol, then zeros up to `last`, then the symbol behind it, which no table has
        norm = norm_for(rng, sets[which], 6, also=(last + 2,))
    lits = rng.integers(0, 256, nlit, dtype=np.uint8).tobytes()
    if not past and by == "proba":
        specs = [None, None, None]
        specs[which] = fse_table(norm, 6)
        return f.block(lits, seqs, tree="raw", specs=specs).blocks
    return _bad_table(name, which, 2, fse_describe(norm, 6))


def _tab_short(name, which):
    """every symbol of the table with probability 1 under accuracy log 9 (8): the symbols run out with most still to give"""
    return _bad_table(name, which, 2, fse_describe([1] * (MAX_SYM[which] + 1), MAX_LOG[which], stop_early=True))


def _tab_truncated(name):
    """a description that the block's end cuts off: the block ends inside the match-length table's description"""
    return _bad_table(name, 2, 2, fse_describe(norm_for(_rng(name), range(40), 9), 9), cut=3)


def _tab_rle(name, which, sym):
    """an RLE table of one symbol: the table's last (OK: literal-length code 35 is a run of 65536 and more, match-length code
    52 a match of 65539 and more, one sequence each) or the one behind it (refused). Offsets: the last code, 31, is a table
    the decoder takes and an offset that no window holds"""
    rng = _rng(name)
    f = Frame()
    huf = make_huf(rng, SKEWED, 5)
    specs = [None, None, None]
    specs[which] = rle_table(sym)
    if which == 0:
        seqs = [(65536 + 123 if sym == 35 else 7, 5, 9 + 3)]
        lits = huf.draw(rng, 66000 if sym == 35 else 300)
    elif which == 2:
        seqs = [(40, 65539 + 4321 if sym == 52 else 9, 17 + 3)]
        lits = huf.draw(rng, 300)
    else:
        seqs = [(40, 9, (1 << 31) + 12345)]
        lits = huf.draw(rng, 300)
    if sym > MAX_SYM[which]:
        return f.block(lits[:300], [(40, 9, 17 + 3)], huf=huf, bad_desc=(1 << (6 - 2 * which), bytes([sym]))).blocks
    return f.block(lits, seqs, huf=huf, specs=specs).blocks


def _tab_offset(name, code, how):
    """an offset code whose offset lies before any window: 24 under the predefined table, 31 under an RLE and a described one"""
    rng = _rng(name)
    f = Frame()
    seqs = [(20, 5, 4 + 3), (3, 6, (1 << code) + 77), (2, 4, 5 + 3)]
    spec = None if how == "predef" else rle_table(code) if how == "rle" else fse_table(norm_for(rng, (2, 3, code), 5), 5)
    if how == "rle":
        seqs = seqs[1:2]
    return f.block(rng.integers(0, 256, 40, dtype=np.uint8).tobytes(), seqs, tree="raw", specs=(None, spec, None)).blocks


def _tab_big(name, which):
    """literal-length code 35 and match-length code 52 under the predefined tables: Huffman literals of more than 65536"""
    rng = _rng(name)
    huf = make_huf(rng, SKEWED, 6)
    if which == 0:
        return Frame().block(huf.draw(rng, 70001), [(65536 + 4000, 7, 100 + 3), (3, 5, 1)], huf=huf).blocks
    return Frame().block(huf.draw(rng, 500), [(400, 65539 + 60000, 300 + 3), (3, 5, 1)], huf=huf).blocks


def _tab_modes(name, kinds):
    """the three tables by the three kinds named, so that each description starts at another offset; then a second block
    that repeats all three, and a third that describes them anew"""
    rng, f = _seq_frame(name)
    sets = [[0, 2, 7, 16, 20], [2, 3, 5, 8], [0, 1, 9, 33, 38]]
    specs = []
    for k, kind in enumerate(kinds):
        if kind == "rle":
            sets[k] = [sets[k][2]]
            specs.append(rle_table(sets[k][0]))
        elif kind == "fse":
            specs.append(fse_table(norm_for(rng, sets[k], 5 + k), 5 + k))
        else:
            specs.append(None)
    pos = _HEAD
    huf = make_huf(rng, SKEWED, 5)
    for blk in range(3):
        seqs, nlit, pos = seqs_for(rng, 25, pos, *sets)
        sp = specs if blk == 0 else ["repeat"] * 3 if blk == 1 else [fse_table(norm_for(rng, sets[k], 6), 6) for k in range(3)]
        if blk == 1:
            f.block(huf.draw(rng, nlit + 4), seqs, huf=huf, streams=4, specs=sp)
        else:
            f.block(rng.integers(0, 256, nlit + 4, dtype=np.uint8).tobytes(), seqs, tree="raw", specs=sp)
        pos += 4
    return f.blocks


def _tab_rle_left(name):
    """one block behind the raw one, all three tables RLE: what the frame leaves in force are three tables of accuracy log 0,
    under which a state is read with read(0)"""
    rng, f = _seq_frame(name)
    seqs, nlit, _ = seqs_for(rng, 25, _HEAD, (7,), (5,), (9,))
    return f.block(rng.integers(0, 256, nlit + 4, dtype=np.uint8).tobytes(), seqs, tree="raw", specs=_RLE_LEFT).blocks


_RLE_LEFT = (rle_table(7), rle_table(5), rle_table(9))


def _tab_stale_rle(name):
    """no table in this frame: behind a raw block, the first compressed block repeats all three tables, and its sequences are
    coded under the RLE tables that seqtab-rle-left leaves, so a decoder that kept them would call the frame OK (RFC 8878
    3.1.1.3.2.1: Repeat_Mode needs a table from a block before in the same frame)"""
    rng = _rng(name)
    f = Frame()
    f.raw(rng.integers(0, 256, 200, dtype=np.uint8).tobytes())
    f.tabs = [([(sp[1], 0, 0)], 0) for sp in _RLE_LEFT]
    seqs, nlit, _ = seqs_for(rng, 10, 200, (7,), (5,), (9,))
    return f.block(rng.integers(0, 256, nlit + 4, dtype=np.uint8).tobytes(), seqs, tree="raw", specs=("repeat",) * 3).blocks


def _seeded(name):
    rng = _rng(name)
    f = Frame()
    f.raw(rng.integers(0, 256, 600, dtype=np.uint8).tobytes())
    pos = 600
    for blk in range(int(rng.integers(1, 4))):
        sets = [sorted({int(v) for v in rng.choice(24, int(rng.integers(1, 6)))}), sorted({int(v) for v in rng.choice(range(2, 9), int(rng.integers(1, 4)))}),
                sorted({int(v) for v in rng.choice(40, int(rng.integers(1, 6)))})]
        specs = []
        for k in range(3):
            kind = int(rng.integers(0, 4))
            if kind == 3 and f.tabs[k] is not None:  # repeat: the codes are those of the table in force
                sets[k] = sorted({e[0] for e in f.tabs[k][0]} & set((range(24), range(2, 10), range(40))[k]))
                specs.append("repeat" if sets[k] else None)
                if not sets[k]:
                    sets[k] = [2, 3]
            elif kind == 1:
                sets[k] = sets[k][:1]
                specs.append(rle_table(sets[k][0]))
            elif kind == 2:
                log = int(rng.integers(5, MAX_LOG[k] + 1))
                lto = tuple(sets[k][:1]) if rng.integers(0, 2) and len(sets[k]) > 1 else ()
                specs.append(fse_table(norm_for(rng, sets[k], log, less_than_one=lto), log))
            else:
                specs.append(None)
        seqs, nlit, pos = seqs_for(rng, int(rng.integers(1, 80)), pos, *sets)
        tail = int(rng.choice((0, 1, 65)))
        pos += tail
        how = int(rng.integers(0, 5))
        if how == 0:
            f.block(rng.integers(0, 256, nlit + tail, dtype=np.uint8).tobytes(), seqs, tree="raw", specs=specs)
        elif how == 1 and f.huf is not None and nlit + tail > 0:
            streams = 4 if nlit + tail >= 6 and rng.integers(0, 2) else 1
            f.block(f.huf.draw(rng, nlit + tail), seqs, streams=streams if nlit + tail < 1000 else 4, specs=specs)
        else:
            maxlen = int(rng.choice((2, 5, 9, 11)))
            nsym = int(rng.integers(maxlen + 1, min(1 << maxlen, 256) + 1))
            huf = make_huf(rng, rng.permutation(256)[:nsym], maxlen)
            n = max(nlit + tail, 4)
            pos += n - (nlit + tail)
            direct = len(huf.weights) <= 129 and rng.integers(0, 2)
            streams = 4 if n >= 6 and (n >= 1000 or rng.integers(0, 2)) else 1
            f.block(huf.draw(rng, n), seqs, huf=huf, streams=streams, tree="direct" if direct else "fse", log=int(rng.integers(5, 7)), specs=specs)
    return f.blocks


def _plan():
    """(name, status, builder) of every case, in the order of the golden file; the rule that refuses a case stands beside it"""
    out = []

    def add(name, fn, *a, status=OK):
        out.append((name, status, lambda: fn(name, *a)))

    for maxlen in (1, 2, 8, 11, 12, 13):  # above HUF_LOG_MAX: refused (RFC 8878 4.2.1: Max_Number_of_Bits is 11)
        for streams in (1, 4):
            add("hufmax-%d-%dstream" % (maxlen, streams), _hufmax, maxlen, streams, status=OK if maxlen <= HUF_LOG_MAX else BAD_FRAME)
    for kind in ("sym2", "sym3", "direct127", "direct128", "fse129", "fse255", "fse256", "fse256-max12", "end-first", "end-second",
                 "log5", "log6", "sparse", "dominant"):
        add("hufsyms-" + kind, _hufsyms, kind)
    add("hufsyms-log7", _hufsyms, "log7", status=BAD_FRAME)        # RFC 8878 4.2.1.2: Max_Accuracy_Log of the weights is 6
    add("hufsyms-weights256", _hufsyms, "weights256", status=BAD_FRAME)  # 257 symbols: a byte has 256 values
    for kind in ("incomplete", "weight13", "all-zero", "incomplete-fse", "fse-no-stream", "fse-header-0", "direct-overlong", "fse-overlong"):
        add("hufbad-" + kind, _hufbad, kind, status=BAD_FRAME)
    # the end of a stream: fewer spare bits than the table's depth are let pass (zstd_decode.h, huf_stream), as many or more
    # are refused, and so is a stream that lacks a bit
    for maxlen in (4, 11):
        ends = [(0, 0, OK), (1, 0, OK), (maxlen - 1, 0, OK), (maxlen, 0, BAD_FRAME), (maxlen + 1, 0, BAD_FRAME), (0, 1, BAD_FRAME)]
        for spare, short, status in ends:
            add("hufend-%d-1stream-%s" % (maxlen, "short1" if short else "spare%d" % spare), _hufend, maxlen, 1, 0, spare, short, status=status)
        add("hufend-%d-4stream-exact" % maxlen, _hufend, maxlen, 4, 0, 0, 0)
        for s in range(4):
            for spare, short, status in ends[1:]:
                add("hufend-%d-4stream-s%d-%s" % (maxlen, s, "short1" if short else "spare%d" % spare), _hufend, maxlen, 4, s, spare, short, status=status)
    for regen in (4, 5, 6, 7, 8):
        add("hufgeom-regen%d" % regen, _hufgeom, "regen", regen, status=BAD_FRAME if regen == 5 else OK)
    for regen, streams, fmt in ((1023, 1, 3), (1023, 4, 3), (1024, 4, 4), (16383, 4, 4), (16384, 4, 5), (300, 4, 4), (300, 4, 5), (1023, 4, 5)):
        add("hufgeom-fmt%d-regen%d-%dstream" % (fmt, regen, streams), _hufgeom, "fmt", (regen, streams, fmt))
    add("hufgeom-regen131072", _hufgeom, "regen", LIT_MAX)
    add("hufgeom-jump-over-by-1", _hufgeom, "jump", status=BAD_FRAME)
    for s in range(4):
        add("hufgeom-empty-s%d" % s, _hufgeom, "empty", s, status=BAD_FRAME)
    add("hufgeom-empty-1stream", _hufgeom, "empty-1stream", status=BAD_FRAME)
    add("hufgeom-dlen5", _hufgeom, "dlen5", status=BAD_FRAME)
    for kind in ("1to4", "4to1", "across-raw", "across-rle", "across-rawlit", "after-max12"):
        add("treeless-" + kind, _treeless, kind)
    add("treeless-overrun", _treeless, "overrun", status=BAD_FRAME)
    add("treeless-stale-4streams", _treeless, "stale-4streams", status=BAD_FRAME)
    add("huflit-4stream", _huflit, 4)
    add("huflit-1stream", _huflit, 1)
    for which, t in enumerate(("ll", "of", "ml")):
        for log in (5, MAX_LOG[which], MAX_LOG[which] + 1):  # RFC 8878 3.1.1.3.2.1: 9, 8 and 9 are the most
            add("seqtab-%s-log%d" % (t, log), _tab_log, which, log, status=OK if log <= MAX_LOG[which] else BAD_FRAME)
        add("seqtab-%s-last" % t, _tab_last, which, False, "proba")
        add("seqtab-%s-past-by-proba" % t, _tab_last, which, True, "proba", status=BAD_FRAME)
        add("seqtab-%s-past-by-zero-run" % t, _tab_last, which, False, "run", status=BAD_FRAME)
        add("seqtab-%s-short" % t, _tab_short, which, status=BAD_FRAME)
    add("seqtab-truncated", _tab_truncated, status=BAD_FRAME)
    add("seqtab-less-than-one", _tab_lto)
    add("seqtab-zero-runs", _tab_zero_runs)
    add("seqtab-ll-rle-35", _tab_rle, 0, 35)
    add("seqtab-ll-rle-36", _tab_rle, 0, 36, status=BAD_FRAME)
    add("seqtab-ml-rle-52", _tab_rle, 2, 52)
    add("seqtab-ml-rle-53", _tab_rle, 2, 53, status=BAD_FRAME)
    add("seqtab-of-rle-31", _tab_rle, 1, 31, status=BAD_FRAME)
    add("seqtab-of-rle-32", _tab_rle, 1, 32, status=BAD_FRAME)
    add("seqtab-ll-code35", _tab_big, 0)
    add("seqtab-ml-code52", _tab_big, 2)
    add("seqtab-of-code24-predef", _tab_offset, 24, "predef", status=BAD_FRAME)
    add("seqtab-of-code31-rle", _tab_offset, 31, "rle", status=BAD_FRAME)
    add("seqtab-of-code31-fse", _tab_offset, 31, "fse", status=BAD_FRAME)
    for kinds in (("rle", "fse", "predef"), ("rle", "predef", "fse"), ("fse", "rle", "predef"), ("fse", "predef", "rle"), ("predef", "rle", "fse"),
                  ("predef", "fse", "rle"), ("rle", "rle", "rle"), ("fse", "fse", "fse"), ("predef", "predef", "predef")):
        add("seqtab-modes-" + "-".join(kinds), _tab_modes, kinds)
    for k in range(36):
        add("seeded-%02d" % k, _seeded)
    add("seqtab-rle-left", _tab_rle_left)  # (behind the seeded ones: a case's mutations are seeded by its place in the list)
    add("seqtab-stale-rle-repeat", _tab_stale_rle, status=BAD_FRAME)
    assert len({n for n, _, _ in out}) == len(out)
    return out


# OK by this decoder's stated limits, an error in libzstd 1.4.8 (reviewed): codes of 12 bits, which that
# release's reader refuses for literals, and fewer spare bits than the table is deep, which it never leaves unused
def ok_here_only(name):
    if name.startswith("hufend-") and "spare" in name:
        return 0 < int(name.rsplit("spare", 1)[1]) < int(name.split("-")[1])
    return name in ("hufmax-12-1stream", "hufmax-12-4stream", "hufsyms-fse256-max12", "treeless-after-max12")


_cache = {}


def cases():
    """every case: dicts with name, status, blocks, frame, content, length, sha256: computed once, shared, not to be changed"""
    if "cases" not in _cache:
        out = []
        for name, status, build in _plan():
            blocks = build()
            if status == OK:
                content = S.execute(blocks)
                fr = S.frame(blocks, len(content))
            else:
                content = b""
                try:
                    declared = len(S.execute(blocks))  # what the frame would be, were it taken
                except AssertionError:
                    declared = 1000  # (an offset that nothing can execute)
                assert declared <= 4096, name
                fr = S.frame(blocks, declared)
            out.append({"name": name, "status": status, "blocks": blocks, "frame": fr, "content": content, "length": len(content),
                        "sha256": hashlib.sha256(content).digest(),
                        # a refused frame of one block is refused before a byte of content is stored: the literals are
                        # decoded into the literal buffer, and the sequences of a batch are resolved before any is executed
                        "stores_nothing": status != OK and len(blocks) == 1})
        _cache["cases"] = out
    return _cache["cases"]


def family(name):
    return name.split("-")[0]


FAMILIES = ("hufmax", "hufsyms", "hufbad", "hufend", "hufgeom", "treeless", "huflit", "seqtab", "seeded")
