"""The ring form of upload_new2 on an engine with the zstd encoder's long-range match finder (zstd_window_log): a ring
chunk's frame is Engine.zstd_encode's frame of the same bytes on the same engine, byte for byte, also when its pages split
it. With a window the seam between a chunk's two pages may lie anywhere in a block's history, so the window kernels read
both parts in place instead of staging one block.

NewConfig(131072) cuts chunks of up to 512 KiB, four blocks, and the ring's pages are 512 KiB. The stream is dots with a
letter every 997 bytes, in which the chunker finds no cut: the cuts asked for and the maximum alone decide, so every chunk
lies where the test puts it. Checked as tests/test_gpu_upload_new2.py checks: the fused call against classify + copy +
blob_encode2 on a twin set, every compressed frame against zstd_encode of the chunk's bytes, every blob back through
blob_decode2 (U._Twins.check)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_upload_new2 as U  # noqa: E402

pytestmark = pytest.mark.gpu
BLOCK = U.BLOCK
PAGE = 4 * BLOCK
NEAR = 10  # the seam this many bytes behind a block's first byte

# chunk starts, from the stream's first byte on; the last entry is the stream's end
CUTS = [0,
        PAGE - 50000,                                   # A: seam inside block 0 of four: in the history of blocks 1 to 3
        PAGE - 50000 + 3 * BLOCK + 5000,
        2 * PAGE - BLOCK,                               # B: seam exactly on the edge between blocks 0 and 1 of three
        2 * PAGE + 2 * BLOCK,
        3 * PAGE - BLOCK - NEAR,                        # C: seam NEAR bytes inside block 1, in a match that begins in its history
        3 * PAGE - BLOCK - NEAR + 2 * BLOCK + 70000,
        4 * PAGE - 200000,                              # D: seam deep inside block 1 of three
        4 * PAGE + 100000,
        4 * PAGE + 140000]
TWO_PAGES = {1: "A", 3: "B", 5: "C", 7: "D"}


@pytest.fixture(autouse=True)
def _short_idle_timeout(monkeypatch):
    monkeypatch.setenv("PBSGPU_RING_IDLE_TIMEOUT_S", "10")


@pytest.mark.parametrize("window_log,tables", [(17, 0), (19, 1)])
def test_seams_in_the_history_on_an_edge_inside_a_block_and_inside_a_crossing_match(gpu_lib, window_log, tables):
    from pbs_plus_amd import Engine, buzhash

    host = U._sparse(CUTS[-1], 3)
    mp = pytest.MonkeyPatch()
    mp.setattr(U, "_engine", lambda avg: Engine(buzhash.NewConfig(avg), device=0, inflight=1, zstd_window_log=window_log,
                                                zstd_seq_tables=tables))
    try:
        eng, ring, sid, recs = U._held(131072, PAGE, 16, host, CUTS[1:-1])
    finally:
        mp.undo()
    try:
        assert [int(e) for e in recs["end"]] == CUTS[1:]  # the cuts asked for and the maximum alone decided
        first, second = U._parts(recs, PAGE)
        assert sorted(np.flatnonzero(second)) == sorted(TWO_PAGES)
        tw = U._Twins(eng, recs[[2, 4, 6]])  # three of the one-page chunks are known
        try:
            flags = tw.check(ring, sid, recs, U._single(host, recs), insert=True)
            assert list(np.flatnonzero(flags == 0)) == [0, 1, 3, 5, 7, 8] and tw.kinds == [0, 6]  # all new ones compressed
            seam = {TWO_PAGES[i]: (int(first[i]), int(recs["size"][i])) for i in TWO_PAGES}
            assert sorted(tw.firsts) == sorted(x for x, _ in seam.values())
            window = 1 << window_log
            # in the history of a later block, and in no block's own bytes from there on
            x, size = seam["A"]
            later = [k * BLOCK for k in range(1, -(-size // BLOCK)) if k * BLOCK - min(k * BLOCK, window) <= x < k * BLOCK]
            assert 0 < x < BLOCK and len(later) >= 1
            # exactly on a block edge
            x, size = seam["B"]
            assert x == BLOCK and size > 2 * BLOCK
            # inside a block
            x, size = seam["D"]
            assert BLOCK < x < 2 * BLOCK < size
            # inside a match that crosses from the history into the block: block 1's first position finds the four dots
            # one byte in front of the block (the highest history position with that hash), and the match runs on through
            # the seam to the next letter
            x, size = seam["C"]
            chunk = host[CUTS[5]:CUTS[6]]
            assert x == BLOCK + NEAR and np.all(chunk[BLOCK - 8:x + 8] == 0x2E)
        finally:
            tw.close()
    finally:
        ring.close_stream(sid)
        ring.close()
        eng.close()
