// Page ring: the kernels of one CUT ROUND and the stop / reset of the persistent SHA-256 services (the services themselves
// and their launchers: kernels.hip; the scan: scan.hip, through launch_scan). Host side: ring.cpp. What a round does, in
// order (scan side and control side on their own HIP streams):
//   k_ring_stage    the round's host-written tables -> device memory, once
//   k_ring_fill     (bench / tests) the synthetic producer writes the round's new pages
//   k_ring_prep_pages / ring_prep (the head of k_ring_control)   page tables, the 128-byte pads that make a page boundary
//                   invisible to the scan window and to a SHA block, and the round's segment table {open chunk start .. new end}
//                   per stream
//   k_scan3         candidates of the NEW pages only (tile -> page through the round's page table)
//   k_ring_control  ONE 1024-thread workgroup: ring_prep, tile prefix scan + compaction (dense ascending candidate list in logical
//                   coordinates), the multi-stream resolve (one wave per stream, single pass), records -> host-visible
//                   record cells + queue descriptors + page reference counts, open-chunk holds, stream state, queue tail
//                   (release), round status. (Round 3 ran this as TEN launch-bound kernels; that chain is gone since round 6.)
// Why only the new pages are scanned: after a round the open chunk [c, end) holds no candidate at or beyond
// c + max(min, 65) (the resolve would have cut there; the one exception, a candidate pre-empted by a suggested boundary
// that lies beyond the bytes seen so far, is carried in the stream state), and earlier ones can never be accepted — so the
// next round needs the open chunk's START (device-resident state), not its bytes' candidates. The bytes stay where they
// are: the pages that hold them are kept by a HOLD reference until the chunk is cut, and the SHA service reads a chunk
// from up to two physical pages.
// A scan tile that finds more candidates than it has slots (periodic / crafted input) is resolved EXACTLY all the same: the
// walk asks such a tile for the first candidate behind a position by re-scanning the stretch on demand (DenseTiles, kernels.h).
// No input fails a stream (rounds 3-5 failed the stream that owned the tile: PBSGPU_E_DENSITY, retired with ABI v5).

#include <algorithm>

#include "fill_word.h"
#include "kernel_util.h"
#include "kernels.h"
#include "resolve_walk.h"
#include "ring_queue.h"

namespace pbsk {

// a ticket for the short queue: true (and the entry written) while the round's allowance lasts. Tickets beyond it are simply
// not used: the tail step publishes min(tickets, allowance) entries, and every ticket below the allowance has written its entry.
__device__ __forceinline__ bool ring_short_ticket(const RingRound &r, const RingDesc &d) {
    const uint32_t idx = atomicAdd(&r.scalars[kRsNshort], 1u);
    if (idx >= r.scalars[kRsShortRoom]) return false;
    ring_desc_encode(r.sdesc_w, (r.q.ctl->stail + idx) & r.q.smask, d);
    return true;
}

// synthetic producer: page bodies of the round that asked for it. A FIXED count of 1024-thread workgroups (RingRound::fill_blocks)
// over an atomic counter, in one of two forms (ring.cpp, ring_enqueue_round, and profiles/ring_cut_partition.log):
//   fill_shared (the default): a 1 KiB LDS tag like every ring-side kernel, two workgroups per cut CU. Nothing runs beside it but
//       the control kernel: it goes in stream order between two scans.
//   whole-CU (pbsgpu_ring_options::fill_cus): each asks for kRingFillLds of LDS it never touches. 96 KiB cannot share a CU's
//       160 KiB with a scan workgroup (64 KiB static + 40 KiB dynamic), with a second refill workgroup, or with a service
//       workgroup (the whole LDS) — so the refill of round n + 1 and the scan of round n, on their own streams, never want the same
//       CU once their two counts add up to no more than the CUs the services leave free. (Until round 6 the refill was
//       npages x 16 light blocks that the dispatcher trickled onto every CU with room, and a scan workgroup — which needs a CU to
//       itself — found none.)
// Work: the round's pages cut into slices of kRingFillSlice bytes, handed out by the counter (RingRound::fill_queue, as
// tile_queue for the scan; zeroed with it by k_ring_prep_pages of the round, which runs behind this kernel). A workgroup that
// finds the counter beyond the last slice leaves; it waits for nothing. The next ticket is fetched while the current slice is
// written (one atomic round trip per slice would otherwise cost as much as the slice). The bytes are a pure function of
// (seed, kind, stream offset), whoever writes them.
constexpr unsigned kRingFillLds = 96u << 10;
constexpr uint32_t kRingFillSlice = 128u << 10;  // two trips of the kind-4 loop (1024 threads x 4 blocks x 16 bytes)
__global__ __launch_bounds__(1024) void k_ring_fill(RingRound r) {
    __shared__ unsigned long long ticket[2];
    const uint32_t tid = threadIdx.x;
    const uint32_t spp = (r.page_bytes + kRingFillSlice - 1u) / kRingFillSlice;  // slices per page (the last one may be partial)
    const unsigned long long nitems = (unsigned long long)r.npages * spp;
    unsigned long long next = 0;
    if (tid == 0) ticket[0] = atomicAdd(r.fill_queue, 1ull);
    __syncthreads();
    for (uint32_t it = 0;; ++it) {
        const unsigned long long item = ticket[it & 1u];
        if (item >= nitems) break;
        if (tid == 0) next = atomicAdd(r.fill_queue, 1ull);
        // (Through this reference the compiler re-reads the seed from the table behind every store of the generator loop. While the
        // table lived in mapped pinned HOST memory (rounds 3-4) those reads went over PCIe and queued up; copying the entry into
        // registers first was tried in round 4 and was SLOWER. Since round 5 r.pages is the device copy k_ring_stage makes.)
        const RingPage &pe = r.pages[item / spp];
        const uint32_t sl = (uint32_t)(item % spp);
        if (pe.do_fill) {
            uint64_t *dst = reinterpret_cast<uint64_t *>(r.arena + pe.phys_off);
            const uint64_t nwords = ((uint64_t)pe.valid + 7u) / 8u;  // a page body is a multiple of 128 bytes: room for the last word
            const uint64_t w0 = pe.fill_off >> 3;
            // 16-byte blocks (page bodies and their stream offsets are 128-aligned); a page is < 2^31 bytes
            const uint32_t nblk = (uint32_t)((nwords + 1u) / 2u);
            const uint32_t b0 = sl * (kRingFillSlice / 16u), b1 = min(nblk, b0 + kRingFillSlice / 16u);
            if (pe.fill_kind == 4u) {
                uint4 *d4 = reinterpret_cast<uint4 *>(dst);
                constexpr uint32_t step = 1024u;
                const uint64_t q0 = w0 >> 1;
                uint32_t i = b0 + tid;
                for (; i + 3u * step < b1; i += 4u * step) {  // four independent blocks per trip: stores and ALU overlap
                    const uint4 a = chacha2_block(q0 + i, pe.fill_seed), b = chacha2_block(q0 + i + step, pe.fill_seed);
                    const uint4 c = chacha2_block(q0 + i + 2u * step, pe.fill_seed), d = chacha2_block(q0 + i + 3u * step, pe.fill_seed);
                    d4[i] = a;
                    d4[i + step] = b;
                    d4[i + 2u * step] = c;
                    d4[i + 3u * step] = d;
                }
                for (; i < b1; i += step) d4[i] = chacha2_block(q0 + i, pe.fill_seed);
            } else if (pe.fill_kind == 5u) {  // piece table: every 16-byte block comes from generator 4 at (piece seed, piece source offset)
                uint4 *d4 = reinterpret_cast<uint4 *>(dst);
                const FillPiece *tab = pe.fill_tab;  // mapped pinned HOST memory: every load is a PCIe round trip — the current piece
                const uint32_t nt = pe.fill_ntab;    // lives in registers and the table is only searched when a block leaves it
                FillPiece pc{~0ull, 0, 0, 0};
                for (uint32_t i = b0 + tid; i < b1; i += 1024u) {
                    const uint64_t x = pe.fill_off + 16ull * i;
                    if (!(x >= pc.dst_off && x - pc.dst_off < pc.len)) {
                        uint32_t lo = 0, hi = nt;
                        while (hi - lo > 1u) {
                            const uint32_t mid = (lo + hi) >> 1;
                            if (tab[mid].dst_off <= x) lo = mid; else hi = mid;
                        }
                        pc = tab[lo];
                    }
                    d4[i] = chacha2_block((pc.src_off + (x - pc.dst_off)) >> 4, pc.seed);
                }
            } else {
                const uint64_t e = min(nwords, 2ull * b1);
                for (uint64_t i = 2ull * b0 + tid; i < e; i += 1024u) dst[i] = fill_word(w0 + i, pe.fill_seed, pe.fill_kind);
            }
        }
        if (tid == 0) ticket[(it + 1u) & 1u] = next;  // (the other word is still being read by slower waves of this trip)
        __syncthreads();
    }
}

// SCAN side (no device state): the head pad of every new page = the last 128 bytes of the stream's previous page, which the
// HOST knows (RingPage::prev_phys). They are the scan's window warm-up for the page's first positions. If the open chunk
// does not reach back over the page boundary the previous page may already serve another stream and the pad is garbage —
// harmlessly: then a cut sits exactly on the boundary, the chunker's window restarts there, and no candidate of the first 64
// bytes behind a cut can ever be accepted (minimum chunk size >= 65).
__global__ __launch_bounds__(64) void k_ring_prep_pages(RingRound r) {
    const uint32_t b = blockIdx.x;
    const int t = threadIdx.x;
    if (b == 0 && t == 0) {
        *r.tile_queue = 0ull;
        *r.fill_queue = 0ull;  // (this round's refill has ended: the scan stream waits for it)
    }
    if (b >= r.npages || t >= 8) return;
    const RingPage &pe = r.pages[b];
    uint4 v = make_uint4(0, 0, 0, 0);
    if (pe.prev_phys != 0xffffffffu)
        v = reinterpret_cast<const uint4 *>(r.arena + (uint64_t)pe.prev_phys * r.stride + 128u + r.page_bytes - 128)[t];
    reinterpret_cast<uint4 *>(r.arena + pe.phys_off - 128)[t] = v;
}

// CONTROL side, in order behind the previous round's control kernel: the head of k_ring_control (its own launch until round 6 —
// 48 us elapsed for 4.5 us of work on the chain that publishes chunks). Items [0, npages): page table entry + TAIL pad of the
// previous page, 16 threads each; then one thread per segment.
__device__ __forceinline__ void ring_prep(const RingRound &r, const uint32_t tid) {
    if (tid < (uint32_t)kRsCount) {  // candidate / record counters
        uint32_t v = 0;
        if (tid == (uint32_t)kRsShortRoom && r.q.short_bytes) {
            // how many short chunks this round may send to the lanes service: what keeps its queue at `short_room` entries.
            // ONE value per round (stail only moves in the control kernels of this stream, shead only grows): every record thread
            // of the control kernel compares its ticket with the same number, so the positions handed out have no holes.
            const unsigned long long sq = __hip_atomic_load(&r.q.ctl->sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t waiting = (uint32_t)sq - (uint32_t)(sq >> 32);
            v = waiting < r.q.short_room ? r.q.short_room - waiting : 0u;
        }
        r.scalars[tid] = v;
    }
    const uint32_t t = tid & 15u;
    for (uint32_t b = tid >> 4; b < r.npages; b += 64u) {
        const RingPage &pe = r.pages[b];
        const RingSeg &sg = r.segs_in[pe.seg];
        RingStreamState *st = r.streams + pe.slot;
        const uint64_t off = pe.logical & kRingOffMask;
        const uint64_t k = off / r.page_bytes;
        const uint8_t *body = r.arena + pe.phys_off;
        // previous page of the stream, if the stream still owns it: inside this round it is the entry before; across
        // rounds the open chunk must reach back over the boundary (else the page may already serve another stream, and
        // its tail pad is not ours to write). The tail pad mirrors the first bytes of this page: a SHA-256 block that
        // starts in the previous page reads on into it.
        const uint8_t *prev = nullptr;
        if (b > sg.first_page) {
            prev = r.arena + r.pages[b - 1].phys_off;
        } else if (k > 0 && !sg.reset && st->c < off) {
            prev = r.arena + (uint64_t)st->pt[(k - 1) % kRingPT] * r.stride + 128u;
        }
        if (t < 8 && prev) {
            uint4 *tailpad = reinterpret_cast<uint4 *>(const_cast<uint8_t *>(prev) + r.page_bytes);
            tailpad[t] = reinterpret_cast<const uint4 *>(body)[t];
        }
        // (pt[k - 1] above is read by the same 16 lanes of one wave, before this store; another page of the round writes pt[k']
        // with k' >= k, which aliases k - 1 only 511 pages on — more than a stream gives one round)
        if (t == 8) st->pt[k % kRingPT] = pe.phys;
    }
    for (uint32_t s = tid; s < r.nseg; s += 1024u) {
        const RingSeg &sg = r.segs_in[s];
        const RingStreamState *st = r.streams + sg.slot;
        const uint64_t c = sg.reset ? 0ull : st->c;
        r.segs[s].offset = ((uint64_t)sg.slot << kRingOffBits) | c;
        r.segs[s].length = sg.new_end - c;
        r.seg_newc[s] = c;   // a segment without records leaves its stream where it was
        r.seg_open[s] = (sg.new_end > c && !sg.final) ? 1u : 0u;
        r.seg_ecand_in[s] = sg.reset ? ~0ull : st->ecand;
        r.seg_ecand[s] = ~0ull;
    }
}

// ---- one record of the round: record cell + queue descriptor + page references ------------------------------------------
// i = dense index of the record in the round (cell cell_base + i); is_last = last record of its segment. Main-queue positions
// are handed out by TICKET (kRsNmain) to the records that stay in the main queue only: a position never stays void. (Until the
// end of round 6 the position was tail0 + i and a chunk that left for the express or the lanes queue — or the round's open
// chunk — left a void descriptor behind; a pair lane that had claimed that position ahead of the tail learned so when the round
// was published and claimed again, behind the tail again: one round of waiting per void, four points of occupancy with the
// lanes tier on — profiles/r06_lanes_service.log. The descriptor carries the cell, so position and cell need not agree.)
__device__ __forceinline__ void ring_order_one(const RingRound &r, const uint32_t i, const pbsgpu_record &rec, const uint32_t s,
                                               const bool is_last) {
    const RingSeg &sg = r.segs_in[s];
    const RingStreamState *st = r.streams + sg.slot;
    const uint64_t Aoff = r.segs[s].offset & kRingOffMask;
    const uint64_t endl = Aoff + rec.end, start = endl - rec.size;
    const uint32_t cell = (r.cell_base + i) & r.cell_mask;
    uint32_t *cw = reinterpret_cast<uint32_t *>(r.q.cells + (uint64_t)cell * kCellBytes);
    if (is_last && r.seg_open[s]) {  // the still-open chunk (resolve_walk decided): no record, no work
        cw[kCellSize] = 0;           // void cell (size 0): the host skips it
        return;
    }
    const uint64_t G = r.page_bytes;
    const uint64_t k1 = start / G, k2 = (endl - 1u) / G;
    const uint32_t o1 = (uint32_t)(start - k1 * G);
    const uint32_t ph1 = st->pt[k1 % kRingPT], ph2 = st->pt[k2 % kRingPT];
    const uint32_t len1 = min(rec.size, (uint32_t)(G - o1));
    const uint64_t p1 = (uint64_t)(uintptr_t)(r.arena + (uint64_t)ph1 * r.stride + 128u + o1);
    uint64_t p2v = p1;
    atomicAdd(&r.q.pending[ph1], 1u);
    uint32_t pages = ph1 | 0xffff0000u;
    if (k2 != k1) {
        p2v = (uint64_t)(uintptr_t)(r.arena + (uint64_t)ph2 * r.stride + 128u) - len1;  // byte `off` of the chunk at p2v + off
        atomicAdd(&r.q.pending[ph2], 1u);
        pages = ph1 | (ph2 << 16);
    }
    // record cell: the service adds digest and flag
    cw[kCellEnd] = (uint32_t)endl;
    cw[kCellEnd + 1] = (uint32_t)(endl >> 32);
    cw[kCellSegment] = sg.slot;
    cw[kCellSize] = rec.size;
    const RingDesc d{p1, p2v, rec.size, len1, cell, pages};
    bool go_long = r.q.long_bytes && rec.size >= r.q.long_bytes;
    if (!go_long && r.q.long_lo && rec.size >= r.q.long_lo) {  // light load: see RingSource::long_lo
        const unsigned long long lq = __hip_atomic_load(&r.q.ctl->lq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t waiting = (uint32_t)lq - (uint32_t)(lq >> 32);
        const uint32_t busy = __hip_atomic_load(&r.q.ctl->xp_busy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + waiting +
                              __hip_atomic_load(&r.scalars[kRsNlong], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        go_long = 4u * busy < 3u * r.q.xp_pairs;
    }
    cw[kCellTier] = 0;  // which queue the chunk went to (0 main, 1 long, 2 short): PBSGPU_RING_F_TIER_TAG, diagnostics
    if (go_long) {
        cw[kCellTier] = 1;
        // a long chunk goes to the queue idle lanes look at first
        ring_desc_encode(r.ldesc_w, (r.q.ctl->ltail + atomicAdd(&r.scalars[kRsNlong], 1u)) & r.q.lmask, d);
    } else if (r.q.short_bytes && rec.size <= r.q.short_bytes &&
               __hip_atomic_load(&r.scalars[kRsNshort], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < r.scalars[kRsShortRoom] &&
               ring_short_ticket(r, d)) {
        // a short chunk for the lanes service (while it has room: RingSource::sdesc)
        cw[kCellTier] = 2;
    } else {
        // only the publish step (same HIP stream) moves the tail
        ring_desc_encode(r.desc_w, (r.q.ctl->tail + atomicAdd(&r.scalars[kRsNmain], 1u)) & r.q.qmask, d);
    }
}

// ---- publish, as three barrier-separated steps of ONE workgroup (tid / nthreads = the workgroup's shape) ------------------
// (1) every ADD before any SUB: a page must never pass through zero while it is still needed
__device__ __forceinline__ void ring_publish_adds(const RingRound &r, const uint32_t tid, const uint32_t nthreads) {
    const uint64_t G = r.page_bytes;
    for (uint32_t s = tid; s < r.nseg; s += nthreads) {
        const RingSeg &sg = r.segs_in[s];
        RingStreamState *st = r.streams + sg.slot;
        const uint64_t end_old = sg.reset ? 0ull : st->end;
        const uint64_t c_new = r.seg_newc[s], end_new = sg.new_end;
        if (r.seg_open[s] && end_new > c_new && sg.npages) {
            const uint64_t first_new = (end_old + G - 1u) / G;                // new pages start here
            uint64_t k = c_new / G;
            if (k < first_new) k = first_new;
            for (; k <= (end_new - 1u) / G; ++k) atomicAdd(&r.q.pending[st->pt[k % kRingPT]], 1u);
        }
    }
}
// (2) holds the OLD open chunk had and the new one does not reach back to; stream state
__device__ __forceinline__ void ring_publish_subs(const RingRound &r, const uint32_t tid, const uint32_t nthreads) {
    const uint64_t G = r.page_bytes;
    for (uint32_t s = tid; s < r.nseg; s += nthreads) {
        const RingSeg &sg = r.segs_in[s];
        RingStreamState *st = r.streams + sg.slot;
        const uint64_t c_old = sg.reset ? 0ull : st->c, end_old = sg.reset ? 0ull : st->end;
        const uint64_t c_new = r.seg_newc[s], end_new = sg.new_end;
        const bool open_new = r.seg_open[s] != 0;
        if (end_old > c_old) {
            const uint64_t last_old = (end_old - 1u) / G;
            for (uint64_t k = c_old / G; k <= last_old; ++k) {
                if (open_new && k >= c_new / G) break;
                ring_release_page(r.q, st->pt[k % kRingPT]);
            }
        }
        st->c = c_new;
        st->end = end_new;
        st->ecand = r.seg_ecand[s];
    }
}
// (3) queue tail (release), round status to the host — thread 0 only
__device__ __forceinline__ void ring_publish_tail(const RingRound &r, const uint32_t n, const uint32_t err) {
    RingCtl *ctl = r.q.ctl;
    uint32_t tail = ctl->tail;
    if (!err) {
        if (r.q.long_bytes)
            __hip_atomic_store(&ctl->ltail, ctl->ltail + r.scalars[kRsNlong], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        if (r.q.short_bytes)
            __hip_atomic_store(&ctl->stail, ctl->stail + min(r.scalars[kRsNshort], r.scalars[kRsShortRoom]), __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_AGENT);
        tail += r.scalars[kRsNmain];
        __hip_atomic_store(&ctl->tail, tail, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    RingRoundStatus *hs = r.status;
    hs->nrec = err ? 0u : n;
    hs->ncand = r.scalars[kRsNcand];
    hs->error = err;
    hs->tail = tail;
    for (int i = 0; i < 6; ++i) hs->probe[i] = __hip_atomic_load(&r.q.probe[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&ctl->rounds_done, ctl->rounds_done + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence_system();
    __hip_atomic_store(&hs->seq, r.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- the control kernel: everything between the scan and the queue tail in ONE 1024-thread workgroup -----------------------
// A round holds <= round_pages x 61 scan tiles (15.6 k), a few dozen streams and a few hundred records: far too little for
// grid-wide launches to pay (each of the ten costs its launch latency while the cut side's CUs idle), small enough for one
// workgroup. The resolve writes every stream's records into a region of `recs` reserved from the HOST's bound on that
// stream's records (RingRound::seg_rec_base), so one walk per stream suffices (no count pass); the dense numbering the
// queue needs comes from a prefix sum over the per-stream counts afterwards.
__device__ __forceinline__ uint32_t block_excl_scan_1024(uint32_t v, uint32_t *wsum /* 16 words of LDS */, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_scan(v, lane);
    __syncthreads();  // wsum may still be read from a previous use
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (int w = 0; w < 16; ++w) {
        const uint32_t x = wsum[w];
        base += (w < wave) ? x : 0u;
        tot += x;
    }
    *total = tot;
    return base + incl - v;
}

// one tile's unordered slots -> ascending END offsets at dense[base ..) (k_compact's two cases, in logical coordinates)
__device__ __forceinline__ void ring_compact_tile(const RingRound &r, const uint64_t t, const uint32_t c, const uint64_t base) {
    const uint32_t *sl = r.tile_slots + t * r.cap;
    const uint64_t tbase = r.pages[t / r.tpp].logical + (t % r.tpp) * (uint64_t)r.tile_bytes;
    if (c <= 48) {
        for (uint32_t j = 0; j < c; ++j) {
            const uint32_t vj = sl[j];
            uint32_t rank = 0;
            for (uint32_t i = 0; i < c; ++i) rank += (sl[i] < vj) ? 1u : 0u;
            if (base + rank < r.dense_cap) r.dense[base + rank] = tbase + vj;
        }
        return;
    }
    const uint32_t strip = r.tile_bytes / 64u;  // dense tile: stable counting sort by lane strip (see k_compact)
    uint32_t cnt[64];
    for (int i = 0; i < 64; ++i) cnt[i] = 0;
    for (uint32_t j = 0; j < c; ++j) cnt[min((sl[j] - 1u) / strip, 63u)]++;
    uint32_t run = 0;
    for (int i = 0; i < 64; ++i) {
        const uint32_t k = cnt[i];
        cnt[i] = run;
        run += k;
    }
    for (uint32_t j = 0; j < c; ++j) {
        const uint32_t vj = sl[j];
        const uint32_t pos = cnt[min((vj - 1u) / strip, 63u)]++;
        if (base + pos < r.dense_cap) r.dense[base + pos] = tbase + vj;
    }
}

__global__ __launch_bounds__(1024) void k_ring_control(RingRound r, SuggFeed fr) {
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t err_s, n_s;
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    RingCtl *ctl = r.q.ctl;
    const unsigned long long tk0 = wall_clock64();  // phase times of this round -> RingRoundStatus::phase_ticks (thread 0)
    ring_prep(r, tid);  // (counted with phase A)
    __threadfence();
    __syncthreads();
    // ---- (A) tile prefix scan + compaction: thread t owns a contiguous run of tiles -------------------------------------
    const uint64_t ntiles = (uint64_t)r.npages * r.tpp;
    const uint64_t per = (ntiles + 1023u) / 1024u;
    const uint64_t t0 = min((uint64_t)tid * per, ntiles), t1 = min(t0 + per, ntiles);
    uint32_t mine = 0, over = 0;
    for (uint64_t tb = t0; tb < t1; tb += 16u) {  // 16 independent loads in flight, not a chain of dependent round trips
        uint32_t v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = (tb + j < t1) ? r.tile_cnt[tb + j] : 0u;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            over |= (v[j] > r.cap) ? 1u : 0u;  // more candidates than slots: the walk re-scans that tile on demand (DenseTiles)
            mine += min(v[j], r.cap);
        }
    }
    uint32_t ncand = 0;
    uint64_t base = block_excl_scan_1024(mine, wsum, &ncand);
    for (uint64_t t = t0; t < t1; ++t) {
        const uint32_t c = min(r.tile_cnt[t], r.cap);
        if (c) ring_compact_tile(r, t, c, base);
        base += c;
    }
    if (tid == 0) r.scalars[kRsNcand] = ncand;
    __threadfence();
    DenseTiles dz{};
    if (__syncthreads_or((int)over)) {
        dz.tile_cnt = r.tile_cnt;
        dz.cap = r.cap;
        dz.tile_bytes = r.tile_bytes;
        dz.table_rot = r.table_rot;
        dz.thr = r.thr;
        dz.base = r.arena;
        dz.pages = r.pages;
        dz.tpp = r.tpp;
    }
    // ---- (B) resolve: one wave per stream, records into the stream's reserved region -------------------------------------
    const unsigned long long tk1 = wall_clock64();
    __builtin_amdgcn_s_setprio(2);
    for (uint32_t seg = (uint32_t)wave; seg < r.nseg; seg += 16u) {
        const uint64_t A = r.segs[seg].offset, B = A + r.segs[seg].length;
        const RingSeg &sgi = r.segs_in[seg];
        SuggFeed f = fr;
        f.open_end = sgi.final ? 0u : 1u;
        f.origin = sgi.origin;
        DenseSeg ds{};
        if (dz.tile_cnt && sgi.npages) {  // the stream's new pages are consecutive entries of the page table, logically contiguous
            ds.L0 = r.pages[sgi.first_page].logical;
            ds.first_tile = (uint64_t)sgi.first_page * r.tpp;
            ds.ntiles = (uint64_t)sgi.npages * r.tpp;
        }
        bool last_real;
        uint64_t last_start, ecand;
        const uint64_t rb = r.seg_rec_base[seg], rcap = r.seg_rec_base[seg + 1u];
        const uint32_t k = resolve_walk<true>(r.dense, ncand, A, B, seg, r.effmin, r.maxsz, rb, r.recs, rcap, r.sugg,
                                              r.sugg ? r.sugg_idx[seg] : 0, r.sugg ? r.sugg_idx[seg + 1u] : 0, r.cmin, f, true,
                                              r.seg_ecand_in[seg], &last_real, &last_start, &ecand, dz, ds);
        if (lane == 0) {
            if (rb + k > rcap) atomicOr(&r.scalars[kRsMaxcnt], 0x80000000u);  // the host's bound was wrong: ring-wide error
            if (k > 0) {
                const bool open = !sgi.final && !last_real;
                r.seg_open[seg] = open ? 1u : 0u;
                r.seg_newc[seg] = (open ? last_start : B) & kRingOffMask;
                r.seg_ecand[seg] = open ? ecand : ~0ull;
            }
            r.seg_cnt[seg] = k;
        }
    }
    __builtin_amdgcn_s_setprio(0);
    __threadfence();
    __syncthreads();
    // ---- (C) dense numbering: prefix over the per-stream counts ---------------------------------------------------------------
    const unsigned long long tk2 = wall_clock64();
    const uint32_t sper = (r.nseg + 1023u) / 1024u;
    const uint32_t s0 = min(tid * sper, r.nseg), s1 = min(s0 + sper, r.nseg);
    uint32_t scount = 0;
    for (uint32_t s = s0; s < s1; ++s) scount += r.seg_cnt[s];
    uint32_t n = 0;
    uint32_t soff = block_excl_scan_1024(scount, wsum, &n);
    for (uint32_t s = s0; s < s1; ++s) {
        r.seg_off[s] = soff;
        soff += r.seg_cnt[s];
    }
    if (tid == 0) {
        uint32_t err = ctl->error;
        if (!err && ((r.scalars[kRsMaxcnt] & 0x80000000u) || n > r.cell_cap)) err = 2u;
        if (err) ctl->error = err;
        err_s = err;
        n_s = n;
        r.scalars[kRsNrec] = n;
    }
    __threadfence();
    __syncthreads();
    const uint32_t err = err_s;
    // ---- (D) records -> cells, descriptors, page references ---------------------------------------------------------------------
    const unsigned long long tk3 = wall_clock64();
    if (!err) {
        for (uint32_t i = tid; i < n; i += 1024u) {
            uint32_t lo = 0, hi = r.nseg;  // last segment with seg_off <= i (empty segments share an offset: take the last)
            while (hi - lo > 1u) {
                const uint32_t mid = (lo + hi) >> 1;
                if (r.seg_off[mid] <= i) lo = mid; else hi = mid;
            }
            const uint32_t s = lo, k = i - r.seg_off[s];
            const pbsgpu_record rec = r.recs[r.seg_rec_base[s] + k];
            ring_order_one(r, i, rec, s, k + 1u == r.seg_cnt[s]);
        }
        ring_publish_adds(r, tid, 1024u);
    }
    __threadfence();
    __syncthreads();
    const unsigned long long tk4 = wall_clock64();
    if (!err) ring_publish_subs(r, tid, 1024u);
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        RingRoundStatus *hs = r.status;
        hs->phase_ticks[0] = (uint32_t)(tk1 - tk0);
        hs->phase_ticks[1] = (uint32_t)(tk2 - tk1);
        hs->phase_ticks[2] = (uint32_t)(tk3 - tk2);
        hs->phase_ticks[3] = (uint32_t)(tk4 - tk3);
        hs->phase_ticks[4] = (uint32_t)(wall_clock64() - tk4);
        hs->phase_ticks[5] = (uint32_t)tk0;
        ring_publish_tail(r, n_s, err);
    }
}

__global__ void k_ring_stop(RingCtl *ctl) { __hip_atomic_store(&ctl->stop, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT); }

// between two service launches (the previous one has ended): positions claimed beyond the tail were never served
__global__ void k_ring_reset(RingCtl *ctl) {
    ctl->head = ctl->tail;
    ctl->lhead = ctl->ltail;  // (equal anyway: the long queue is always emptied before a service ends)
    ctl->xp_busy = 0;
    ctl->shead = ctl->stail;  // (equal anyway: like the long queue, the short queue is emptied before a service ends)
    ctl->stop = 0;
}

hipError_t launch_ring_stop(RingCtl *ctl, hipStream_t st) {
    hipLaunchKernelGGL(k_ring_stop, dim3(1), dim3(1), 0, st, ctl);
    return hipGetLastError();
}

hipError_t launch_ring_reset(RingCtl *ctl, hipStream_t st) {
    hipLaunchKernelGGL(k_ring_reset, dim3(1), dim3(1), 0, st, ctl);
    return hipGetLastError();
}

// Dynamic LDS the round's kernels ask for although they never touch it: the SHA service's workgroups take the WHOLE
// LDS of their CUs (launch_ring_service), so any kernel that needs even one LDS granule is placed on the other CUs —
// the chip is partitioned between the service's serial chains and everything else without CU masks.
constexpr unsigned kRingLdsTag = 1024;

// The round's tables travel ONCE over PCIe: up to four spans of the host-written input block -> its device mirror (grid.y =
// span). Every later kernel of the round — the refill's generator loop, the scan's tile -> page indirection, prep, the control
// kernel's walks — then reads device memory (round 5: the refill re-read its page entry from mapped host memory behind every
// store and ran at the latency of those reads, 3.7 us per page in small rounds, 8-11 in large ones; the control kernel paid
// ~20 dependent PCIe round trips per round).
__global__ __launch_bounds__(256) void k_ring_stage(RingStage s) {
    const uint32_t sp = blockIdx.y;
    const uint32_t n16 = (s.len[sp] + 15u) / 16u;
    const uint4 *a = reinterpret_cast<const uint4 *>(s.src + s.off[sp]);
    uint4 *b = reinterpret_cast<uint4 *>(s.dst + s.off[sp]);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += gridDim.x * blockDim.x) b[i] = a[i];
}

hipError_t launch_ring_round(const RingRound &r, int num_cus, hipStream_t st, hipStream_t fill_st, hipEvent_t fill_ev,
                             hipStream_t scan_st, hipEvent_t scan_ev, const RingStage *stage) {
    // Two in-order chains per round: SCAN side (head pads -> scan; needs only the pages' bytes) on `sst`, CONTROL side
    // (tail pads / page table / segments from the device-resident stream state -> control kernel) on `st` behind it. With
    // two streams the scan of round n + 1 runs while the one-workgroup control kernel of round n resolves and publishes —
    // 0.17 ms per round during which the cut side's other CUs used to idle (17 % of its time, profiles/README.md round 3).
    hipStream_t sst = scan_st ? scan_st : st;
    bool any_fill = false;
    const RingPage *hp = stage ? stage->pages_host : r.pages;  // mapped pinned: host-readable
    for (uint32_t i = 0; i < r.npages; ++i) any_fill |= hp[i].do_fill != 0;
    if (stage) {  // first kernel of the round, on the stream whose kernels read the tables first
        uint32_t mx = 1;
        for (int k = 0; k < 4; ++k) mx = std::max(mx, (stage->len[k] / 16u + 255u) / 256u);
        hipLaunchKernelGGL(k_ring_stage, dim3(std::min(mx, 8u), 4), dim3(256), kRingLdsTag, (any_fill && fill_st) ? fill_st : sst, *stage);
    }
    if (any_fill) {
        // the synthetic producer runs on its own HIP stream: the refill of round n + 1 overlaps the cut of round n (both
        // live on the CUs the SHA service leaves free)
        hipError_t fe = allow_lds(&k_ring_fill, kRingFillLds);
        if (fe != hipSuccess) return fe;
        hipLaunchKernelGGL(k_ring_fill, dim3(std::max(1u, r.fill_blocks)), dim3(1024), r.fill_shared ? kRingLdsTag : kRingFillLds,
                           fill_st ? fill_st : sst, r);
        if (fill_st && fill_st != sst) {
            hipError_t e = hipEventRecord(fill_ev, fill_st);
            if (e != hipSuccess) return e;
            e = hipStreamWaitEvent(sst, fill_ev, 0);
            if (e != hipSuccess) return e;
        }
    }
    hipLaunchKernelGGL(k_ring_prep_pages, dim3(r.npages ? r.npages : 1), dim3(64), kRingLdsTag, sst, r);
    const uint64_t ntiles = (uint64_t)r.npages * r.tpp;
    if (ntiles) {
        ScanParams p{};
        p.data_al = r.arena;
        p.lead = 0;
        p.nbytes = ~0ull >> 1;  // the per-page limits come from the page table
        p.ntiles = ntiles;
        p.tile_bytes = r.tile_bytes;
        p.table_rot = r.table_rot;
        p.thr = r.thr;
        p.cap = r.cap;
        p.tile_cnt = r.tile_cnt;
        p.tile_slots = r.tile_slots;
        p.tile_queue = r.tile_queue;
        p.ring_pages = r.pages;
        p.ring_tpp = r.tpp;
        p.max_blocks = r.scan_blocks;
        hipError_t e = launch_scan(p, num_cus, sst);  // (tile_bytes is one of the scan's two tile sizes: shape_ring, ring_plan.h)
        if (e != hipSuccess) return e;
    }
    if (sst != st) {
        hipError_t e = hipEventRecord(scan_ev, sst);
        if (e != hipSuccess) return e;
        e = hipStreamWaitEvent(st, scan_ev, 0);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_ring_control, dim3(1), dim3(1024), kRingLdsTag, st, r, SuggFeed{r.sugg_feed, 0, r.sugg_abs, 0});
    return hipGetLastError();
}

}  // namespace pbsk
