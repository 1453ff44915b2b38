"""xxh64.h, zstd_stream.h and the checksum of zstd_encode.h (pbs_plus_amd/csrc) as a CPU program under AddressSanitizer +
UBSan: a stand-alone program with its own main (tests/native/test_zstd_checksum.cpp), nothing loaded into Python, nothing
preloaded. Against tests/golden/zstd_checksum_v1.json: XXH64 at every length class, seed and alignment; libzstd frames
with a checksum, each with a checksum byte and a raw-block byte flipped; whole streams; this project's own frames with
and without the checksum in every encoder mode; every frame and stream through seeded single-byte mutations and
truncations between guard bytes. Where libzstd loads, the comparison runs in both directions."""
import os
import struct
import subprocess
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zstd_checksum_inputs as zi  # noqa: E402
import zstd_inputs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPROC = 4
NMUT_FRAME, NMUT_STREAM = 300, 200
MODES = ("predefined", "tables", "window17", "window17-tables")  # bit 0 tables, bit 1 window

# one bit per branch, in the order of the enum in xxh64.h
BRANCHES = ("xxh_stripes xxh_short xxh_tail_8 xxh_tail_4 xxh_tail_1 xxh_empty sum_good sum_bad sum_absent sum_not_asked "
            "one_frame stream_empty stream_frame stream_second_frame stream_skippable stream_skippable_cut stream_short_tail "
            "stream_frame_fails stream_no_frame enc_sum enc_no_sum enc_sum_no_room").split()
UNREACHED = ()  # every new branch is reached


def _ops():
    """(ops, pieces of the ops file): an op is a dict with kind and what the test expects of it"""
    ops = []
    for n, seed, base, h in zi.golden()["xxh64"]:
        ops.append(dict(kind="X", base=base, seed=seed, data=zi.pattern(base + n), want=int(h, 16)))
    for f in zi.frames():
        for flags in (zi.F_CHECKSUM, zi.F_CHECKSUM | zi.F_STREAM):
            ops.append(dict(kind="D", name=f["name"], flags=flags, room=f["length"], nmut=NMUT_FRAME, cuts=1, data=f["frame"],
                            status=zi.OK, content=f["content"]))
        ops.append(dict(kind="D", name=f["name"] + "-flags0", flags=0, room=f["length"], nmut=0, cuts=0, data=f["frame"],
                        status=zi.OK, content=f["content"]))
        if f["length"]:
            ops.append(dict(kind="D", name=f["name"] + "-small", flags=zi.F_CHECKSUM, room=f["length"] - 1, nmut=0, cuts=0,
                            data=f["frame"], status=zi.BAD_SIZE, content=b""))
    for c in zi.flipped():
        ops.append(dict(kind="D", name=c["name"], flags=zi.F_CHECKSUM, room=c["length"], nmut=0, cuts=0, data=c["frame"],
                        status=zi.BAD_CHECKSUM, content=b""))
        ops.append(dict(kind="D", name=c["name"] + "-stream", flags=zi.F_CHECKSUM | zi.F_STREAM, room=c["length"], nmut=0, cuts=0,
                        data=c["frame"], status=zi.BAD_CHECKSUM, content=b""))
        ops.append(dict(kind="D", name=c["name"] + "-flags0", flags=0, room=c["length"], nmut=0, cuts=0, data=c["frame"],
                        status=zi.OK, content=None))  # the old call's answer: OK, to bytes nobody vouches for
    for s in zi.streams():
        ops.append(dict(kind="D", name=s["name"], flags=zi.F_CHECKSUM | zi.F_STREAM, room=s["room"], nmut=NMUT_STREAM, cuts=1,
                        data=s["stream"], status=s["status"], content=s["content"]))
    two = next(s for s in zi.streams() if s["name"] == "two")
    ops.append(dict(kind="D", name="two-small", flags=zi.F_STREAM, room=two["room"] - 1, nmut=0, cuts=0, data=two["stream"],
                    status=zi.BAD_SIZE, content=b""))
    ops.append(dict(kind="D", name="two-not-a-stream", flags=zi.F_CHECKSUM, room=two["room"], nmut=0, cuts=0, data=two["stream"],
                    status=zi.UNSUPPORTED, content=b""))  # without F_STREAM a second frame is what it always was
    bad = next(s for s in zi.streams() if s["name"] == "second-bad-checksum")
    ops.append(dict(kind="D", name="second-bad-checksum-not-asked", flags=zi.F_STREAM, room=bad["room"], nmut=0, cuts=0,
                    data=bad["stream"], status=zi.OK, content=two["content"]))
    for mode in range(4):
        for name, n in zi.ENC_CONTENTS:
            ops.append(dict(kind="E", mode=mode, name="%s-%d" % (name, n), data=zi.enc_content(name, n)))
    return ops


def _pack(op):
    d = op["data"]
    if op["kind"] == "X":
        return b"X" + struct.pack("<IQQ", op["base"], op["seed"], len(d)) + d
    if op["kind"] == "D":
        return b"D" + struct.pack("<IQIIQ", op["flags"], op["room"], op["nmut"], op["cuts"], len(d)) + d
    return b"E" + struct.pack("<IQ", op["mode"], len(d)) + d


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """builds and runs the program once: (ops, [(exit code, stdout, stderr)], result lines by op, frames by op)"""
    tmp = tmp_path_factory.mktemp("zstd_checksum")
    ops = _ops()
    path = str(tmp / "ops.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(ops)))
        for op in ops:
            f.write(_pack(op))
    exe = str(tmp / "test_zstd_checksum")
    flags = ["-std=c++17", "-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
             "-Wall", "-Wextra"]
    subprocess.run(["g++", *flags, os.path.join(ROOT, "tests", "native", "test_zstd_checksum.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    procs = [subprocess.Popen([exe, path, str(tmp / ("res.%d" % k)), str(tmp / ("frames.%d" % k)), str(NPROC), str(k)],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env) for k in range(NPROC)]
    outs, lines, frames = [], {}, {}
    for k, p in enumerate(procs):
        so, se = p.communicate(timeout=900)
        outs.append((p.returncode, so, se))
        if not os.path.exists(str(tmp / ("res.%d" % k))):
            continue
        dump = open(str(tmp / ("frames.%d" % k)), "rb").read()
        for ln in open(str(tmp / ("res.%d" % k))):
            w = ln.split()
            lines.setdefault(int(w[0]), []).append(w[1:])
            if w[1] == "E" and int(w[4]) == zi.OK:
                frames[int(w[0])] = dump[int(w[8]):int(w[8]) + int(w[5])]
    return ops, outs, lines, frames


def test_the_program_ends_clean_under_the_sanitizers(run):
    ops, outs, lines, frames = run
    for code, so, se in outs:
        assert code == 0 and "zstd-checksum-ok" in so, so[-4000:] + se[-4000:]
        assert "runtime error" not in se and "AddressSanitizer" not in se
    assert sorted(lines) == list(range(len(ops)))


def test_xxh64_matches_xxhash_at_every_length_seed_and_alignment(run):
    ops, outs, lines, frames = run
    seen = 0
    for i, op in enumerate(ops):
        if op["kind"] == "X":
            assert int(lines[i][0][1], 16) == op["want"], (len(op["data"]) - op["base"], op["seed"], op["base"])
            seen += 1
    assert seen == len(zi.XXH_LENGTHS) * len(zi.XXH_SEEDS) * 8


def test_frames_and_streams_decode_to_what_is_recorded(run):
    ops, outs, lines, frames = run
    seen = set()
    for i, op in enumerate(ops):
        if op["kind"] != "D":
            continue
        kind, _, status, decoded, crc = lines[i][0]
        assert kind == "D" and int(status) == op["status"], (op["name"], op["flags"], status)
        if op["content"] is not None:
            assert int(decoded) == len(op["content"]) and int(crc) == zlib.crc32(op["content"]), op["name"]
        assert sum(ln[0] == "M" for ln in lines[i]) == (op["nmut"] if op["data"] else 0)
        seen.add(op["status"])
    assert seen == {zi.OK, zi.BAD_FRAME, zi.BAD_SIZE, zi.UNSUPPORTED, zi.BAD_CHECKSUM}
    # a flipped byte is OK for the call without flags and status 4 with F_CHECKSUM: the same frames, the two answers
    names = {op["name"]: op["status"] for op in ops if op["kind"] == "D"}
    for c in zi.flipped():
        assert names[c["name"]] == zi.BAD_CHECKSUM and names[c["name"] + "-flags0"] == zi.OK


def test_own_frames_carry_the_checksum_in_every_mode(run):
    ops, outs, lines, frames = run
    want = zi.golden()["contents"]
    seen = 0
    for i, op in enumerate(ops):
        if op["kind"] != "E":
            continue
        _, st0, flen0, st1, flen1, st_small, checks, _ = lines[i][0]
        n = len(op["data"])
        what = (MODES[op["mode"]], op["name"])
        assert int(st0) == zi.OK and int(st1) == zi.OK and int(flen1) == int(flen0) + 4 and int(checks) == 7, (what, lines[i][0])
        fr = frames[i]
        assert fr[4] & 4 and int.from_bytes(fr[-4:], "little") == int(want[op["name"]], 16) & 0xFFFFFFFF, what
        bound2 = 5 + (1 if n <= 255 else 2 if n <= 65_791 else 4) + 3 * max(1, -(-n // (128 << 10))) + n + 4
        assert int(flen1) <= bound2
        assert int(st_small) == (zi.OK if int(flen1) <= bound2 - 1 else zi.BAD_SIZE), what
        if op["name"].startswith("rand") or n == 0:
            assert int(flen1) == bound2 and int(st_small) == zi.BAD_SIZE, what  # nothing to gain: exactly the bound
        seen += 1
    assert seen == 4 * len(zi.ENC_CONTENTS)


def test_the_cases_reach_every_new_branch(run):
    ops, outs, lines, frames = run
    cov = 0
    for code, so, se in outs:
        word = [w for w in so.split() if w.startswith("0x")]
        assert word and "of %d bits" % len(BRANCHES) in so, so[-2000:]
        cov |= int(word[0], 16)
    missing = [b for i, b in enumerate(BRANCHES) if not cov >> i & 1]
    print("coverage", hex(cov), "missing", missing)
    assert sorted(missing) == sorted(UNREACHED)


def _input(i, op, ln):
    """the bytes of result line ln of op i, and the position of the mutated byte (None: not a mutation)"""
    d = op["data"]
    if ln[0] == "D":
        return d, None
    if ln[0] == "C":
        return d[:int(ln[1])], None
    at, xor = zstd_inputs.mutation(i, int(ln[1]), len(d))
    return zstd_inputs.mutated(d, at, xor), at


def _header_positions(stream):
    """positions of the Frame_Header_Descriptor and of the byte behind it (the Window_Descriptor of a frame that is not
    single-segment) of every zstd frame of an intact stream, where its second and later zstd frames start, and the byte
    ranges of its frames that carry no checksum"""
    pos, heads, later, nframes, unsummed = 0, set(), [], 0, []
    while pos + 8 <= len(stream):
        magic = int.from_bytes(stream[pos:pos + 4], "little")
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            pos += 8 + int.from_bytes(stream[pos + 4:pos + 8], "little")
            continue
        if magic != 0xFD2FB528:
            break
        heads |= {pos + 4, pos + 5}
        if nframes:
            later.append(pos)
        nframes += 1
        fhd = stream[pos + 4]
        single, fcs_flag, did = fhd >> 5 & 1, fhd >> 6, (0, 1, 2, 4)[fhd & 3]
        p = pos + 5 + (0 if single else 1) + did + (single if fcs_flag == 0 else 1 << fcs_flag)
        while True:
            bh = int.from_bytes(stream[p:p + 3], "little")
            p += 3 + (1 if bh >> 1 & 3 == 1 else bh >> 3)
            if bh & 1:
                break
        if not fhd & 4:
            unsummed.append(range(pos, p))
        pos = p + (4 if fhd & 4 else 0)
    return heads, later, unsummed


def _against_libzstd(run):
    """every base, mutated and truncated input of the ops with both flags through ZSTD_decompress: (compared, accepted by
    both, converse not asked, exceptions as [op, line kind, parameter, direction, class]); None when libzstd does not load.
    Directions: "there-only": libzstd decodes it and this does not give the same bytes with OK; "here-only": OK here and an
    error there. Classes: see the test below; None = in no class."""
    ops, outs, lines, frames = run
    g = zstd_inputs.golden()
    z = g.load_libzstd()
    if z is None:
        return None
    compared = both = not_asked = 0
    exceptions = []
    for i, op in enumerate(ops):
        if op["kind"] != "D" or op["flags"] != (zi.F_CHECKSUM | zi.F_STREAM) or not op["nmut"]:
            continue
        heads, later, unsummed = _header_positions(op["data"])
        for ln in lines[i]:
            data, at = _input(i, op, ln)
            status, decoded, crc = int(ln[2]), int(ln[3]), int(ln[4])
            got, err = g.decompress(z, data, op["room"])
            compared += 1
            here = status == zi.OK
            if got is not None and here and decoded == len(got) and crc == zlib.crc32(got):
                both += 1
                continue
            if got is None and not here:
                continue
            if got is None and here and at is not None and any(at in r for r in unsummed):
                not_asked += 1  # a mutation inside a frame that carries no checksum: nothing vouches for its content
                continue
            cls = None
            if got is None and here and at in heads:
                cls = "window"       # the frame as mutated declares a window that libzstd refuses
            elif got is not None and status == zi.BAD_FRAME and at is not None and later and at >= later[0]:
                cls = "cross-frame"  # an offset of a later frame that reaches into the frame before it
            exceptions.append([op["name"], ln[0], int(ln[1]), "here-only" if here else "there-only", cls])
    return compared, both, not_asked, exceptions


def test_libzstd_and_this_decoder_accept_the_same_inputs(run):
    """For the checksummed frames and the streams, with both flags: what libzstd decodes, this decodes to the same bytes,
    AND what this accepts, libzstd accepts: with the checksum verified the comparison runs in both directions. The converse
    is asked wherever a checksum covers the mutated byte; the one frame without a checksum that two of the streams hold is
    outside it, as every frame was before (tests/test_zstd_core_native.py). Exceptions are allowed by class only
    (DESIGN.md §20), and every one met must fall into one:
      window       OK here, an error there, and the mutated byte is a frame's Frame_Header_Descriptor or the byte behind it:
                   the frame as mutated declares a window that libzstd refuses (above its limit, or smaller than a block
                   it then meets). Here a declared window size is read, not enforced (§15).
      cross-frame  decoded there, BAD_FRAME here, and the mutated byte lies in the second or a later frame of the stream:
                   an offset that reaches in front of its own frame's first byte, into the output of the frame before it,
                   which libzstd's one-shot call keeps as a prefix. Refused here by decision.
    There is no numeric allowance."""
    res = _against_libzstd(run)
    if res is None:
        print("libzstd does not load on this machine: nothing to compare against")
        return
    compared, both, not_asked, exceptions = res
    by_class = {}
    for e in exceptions:
        by_class.setdefault(e[4], []).append(e)
    print("compared", compared, "accepted by both with the same bytes", both, "converse not asked (no checksum)", not_asked,
          "exceptions", {k: len(v) for k, v in by_class.items()})
    assert not by_class.get(None), by_class[None][:20]
    assert compared > 10_000 and both > 100
