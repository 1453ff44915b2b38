// The min/max resolve walk of one segment by one wave: k_resolve (resolve.hip) and the page ring's control kernel
// (ring_kernels.hip) both run it.
#pragma once

#include "kernels.h"

namespace pbsk {

// =====================================================================================
// (2b) min/max resolution — one wave per segment walks the sorted candidate list
// =====================================================================================
// Serial rule being reproduced (oracle/buzhash_oracle.c shall_break): after a cut at s the
// next cut is the first end e with (e - s >= max) or (e - s >= max(min, 65) and e is a
// candidate); the stream end closes the last chunk. The break test only runs in the
// rolling loop, i.e. from chunk_size 65 on, hence the 65.
// Suggested boundaries (payload chunker, SURVEY.md Appendix A note 3 / E.3; oracle_payload_chunker_scan fed byte by
// byte): a second ascending list per segment. After a cut at s the next cut is the EARLIER of the hash/max cut and
// the first suggested boundary b with min <= b - s <= max; boundaries with b - s < min are dropped for good. For
// min >= 65 they behave exactly like extra candidates; the separate list keeps the min = 64 corner (hash cuts need
// chunk_size >= 65, a suggested one only >= min) exact.
// ---- candidate-dense tiles: the first TRUE candidate of a stretch of one tile, on demand (see DenseTiles, kernels.h) ----
// All 64 lanes call it with the same arguments. q = the byte at the END of the first window (the window of position i is
// q[i - 63 .. i]); n positions. Returns the index of the first position whose window hash passes the break test, ~0u if none.
// One wave, rows of 256 bytes (one aligned dword per lane, coalesced), the prefix form the scan kernels use:
//   Q(x) = rotl(Q(x - 1), 1) ^ t(x)   (t = pre-rotated table value of byte x),   h(x) = Q(x) ^ Q(x - 64)   (64 = 0 mod 32)
// Q inside a lane's 4 bytes is 3 rotate-xor steps; across lanes an inclusive scan with a rotation of 4 bits per lane (six
// shuffle steps: 4, 8, 16, then 32 / 64 / 128 = 0 bits); Q(x - 64) is the same byte of the lane 16 below. Lanes 0-15 of a
// row only warm the prefix up, so rows advance by 192 bytes. A dword that holds no byte of [first window start, last
// window end] is never read (the caller's buffer may begin or end right there). ~90 instructions and 11 shuffles per 192
// positions, a dozen VGPRs: this is the cold path of the resolve walk and must not cost the walk its registers.
__device__ __forceinline__ uint32_t dense_first_hit(const uint8_t *q, const uint32_t n, const uint32_t *__restrict__ tab,
                                                    const uint32_t thr) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint8_t *w0 = q - 63;                                        // first byte of the first window
    const uint32_t sh = (uint32_t)((uintptr_t)w0 & 3u);
    const uint8_t *a0 = w0 - sh - 4;                                   // row 0 starts one dword early: position 0 ends at byte
                                                                       // sh + 67 >= 64 of its row, i.e. in a lane >= 16
    const uintptr_t lo_dw = (uintptr_t)(w0 - sh), hi_dw = (uintptr_t)(q + (n - 1u)) & ~(uintptr_t)3;  // first / last dword with a needed byte
    auto load_row = [&](const uint32_t r) -> uint32_t {
        const uintptr_t A = (uintptr_t)a0 + 192u * (uintptr_t)r + 4u * lane;
        const uintptr_t Ac = min(max(A, lo_dw), hi_dw);
        const uint32_t v = *reinterpret_cast<const uint32_t *>(Ac);
        return (A == Ac) ? v : 0u;
    };
    const uint32_t rows = (n + sh + 3u) / 192u + 1u;                   // positions of row r: 192 r + 4 lane + k - sh - 67
    uint32_t w = load_row(0);
    for (uint32_t r = 0; r < rows; ++r) {
        const uint32_t wn = (r + 1u < rows) ? load_row(r + 1u) : 0u;   // next row's bytes in flight behind this row's arithmetic
        const uint32_t t0 = tab[w & 0xffu], t1 = tab[(w >> 8) & 0xffu], t2 = tab[(w >> 16) & 0xffu], t3 = tab[w >> 24];
        const uint32_t q0 = t0;
        const uint32_t q1 = __builtin_rotateleft32(q0, 1) ^ t1;
        const uint32_t q2 = __builtin_rotateleft32(q1, 1) ^ t2;
        const uint32_t q3 = __builtin_rotateleft32(q2, 1) ^ t3;
        uint32_t X = q3;                                               // inclusive scan over the lanes' 4-byte sums
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(X, d, 64);
            if ((int)lane >= d) X ^= __builtin_rotateleft32(y, (4 * d) & 31);
        }
        uint32_t Xp = __shfl_up(X, 1, 64);
        if (lane == 0) Xp = 0;
        const uint32_t Q[4] = {q0 ^ __builtin_rotateleft32(Xp, 1), q1 ^ __builtin_rotateleft32(Xp, 2),
                               q2 ^ __builtin_rotateleft32(Xp, 3), q3 ^ __builtin_rotateleft32(Xp, 4)};
        uint32_t first = ~0u;
        const uint32_t i0 = 192u * r + 4u * lane - sh - 67u;          // position of byte 0 of this lane (wraps below 0: masked)
#pragma unroll
        for (int k = 3; k >= 0; --k) {
            const uint32_t h = Q[k] ^ __shfl_up(Q[k], 16, 64);
            const uint32_t i = i0 + (uint32_t)k;
            if (lane >= 16u && h >= thr && i < n) first = i;           // (i < n also rejects the wrapped "negative" positions)
        }
        const unsigned long long m = __ballot(first != ~0u);
        if (m) return __shfl(first, __ffsll((long long)m) - 1, 64);    // lanes are in position order
        w = wn;
    }
    return ~0u;
}

// The walk is about to take `c` (first LISTED candidate >= tlo, ~0 = none) as the next hash cut unless the maximum (`lim` =
// min(s + max, B)) comes first. Tiles that overflowed their slots may hold an unlisted candidate before that: the first
// one in [tlo, min(c - 1, lim)] is returned instead of c. Wave-uniform.
__device__ __forceinline__ uint64_t dense_refine(const DenseTiles &d, const DenseSeg &ds, const uint64_t tlo, const uint64_t lim,
                                                 const uint64_t c) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t lo = max(tlo, ds.L0 + 1u);  // (page ring: older pages hold no candidate at or behind tlo)
    const uint64_t hi = min(c - 1u, lim);
    if (ds.ntiles == 0 || lo > hi) return c;
    // tile coordinates x = E - L0 + lead (>= 1): tile k holds the END offsets x in (k * tile_bytes, (k + 1) * tile_bytes]
    const uint64_t lo_x = lo - ds.L0 + ds.lead, hi_x = min(hi - ds.L0 + ds.lead, ds.ntiles * d.tile_bytes);
    if (lo_x > hi_x) return c;
    const uint64_t ta = (lo_x - 1u) / d.tile_bytes, tb = (hi_x - 1u) / d.tile_bytes;
    for (uint64_t t0 = ta; t0 <= tb; t0 += 64u) {
        const uint64_t t = t0 + lane;
        unsigned long long m = __ballot(t <= tb && d.tile_cnt[ds.first_tile + t] > d.cap);
        while (m) {
            const uint64_t tt = t0 + (uint64_t)(__ffsll((long long)m) - 1);
            m &= m - 1ull;
            const uint64_t qlo_x = max(lo_x, tt * d.tile_bytes + 1u), qhi_x = min(hi_x, (tt + 1u) * d.tile_bytes);
            const uint64_t E0 = ds.L0 + qlo_x - ds.lead;  // the stretch's first END offset, in the walk's coordinates
            const uint8_t *q;
            if (d.pages) {
                const RingPage &pe = d.pages[(ds.first_tile + tt) / d.tpp];
                q = d.base + pe.phys_off + (E0 - 1u - pe.logical);
            } else {
                q = d.base + (E0 - 1u);
            }
            const uint32_t r = dense_first_hit(q, (uint32_t)(qhi_x - qlo_x + 1u), d.table_rot, d.thr);
            if (r != ~0u) return E0 + r;
        }
    }
    return c;
}

// The walk of ONE segment by ONE wave (all 64 lanes call it with the same arguments). Returns the number of records;
// WRITE: record k goes to recs[rbase + k] (lane 0), `seg` is stored in its segment field.
// Page-ring rounds (`ring`; ring_kernels.hip): the segment is a stream's open chunk + its new pages in logical
// coordinates ((slot << kRingOffBits) | offset); suggested offsets are relative to the STREAM's byte 0; the segment's end is the
// stream's end only if RingSeg::final; and the walk reports what the round leaves behind: is the last record the still-open
// chunk (it is unless the serial chunker cuts exactly at the current end: a max-size chunk, a candidate or a winning
// suggested boundary there), where that chunk starts, and — reader-buffer rule only — the hash candidate inside it that a
// boundary beyond the bytes seen so far pre-empts. Such a candidate lies in pages the next round does not scan again, so
// it is carried in the stream state and handed back as `ecand_first`.
template <bool WRITE>
__device__ __forceinline__ uint32_t resolve_walk(const uint64_t *cands, const uint64_t n, const uint64_t A, const uint64_t B,
                                                 const uint32_t seg, const uint32_t effmin, const uint32_t maxsz,
                                                 const uint64_t rbase, pbsgpu_record *recs, const uint64_t rec_cap,
                                                 const uint64_t *sugg, const uint64_t sbeg, const uint64_t send,
                                                 const uint32_t cmin, const SuggFeed fr, const bool ring,
                                                 const uint64_t ecand_first, bool *last_real_out, uint64_t *last_start_out,
                                                 uint64_t *ecand_out, const DenseTiles &dz, const DenseSeg &ds) {
    const int lane = threadIdx.x & 63;
    uint64_t s = A;
    uint32_t k = 0;
    // WRITE: record k waits in the registers of lane k mod 64 and 64 records leave with ONE store instruction. (Until round 6 lane 0
    // stored every record as it was cut — and the loop's header waits for vmcnt(0), a loaded window may be pending there, which
    // on this ISA also counts the stores: every record paid a store round trip, ~1.2 us beside the ring's streaming traffic;
    // 87 of the control kernel's 147 us per round: profiles/r06_control_kernel_phases.log.)
    [[maybe_unused]] uint64_t my_end = 0;
    [[maybe_unused]] uint32_t my_size = 0;
    // coordinates of the suggested offsets / of the absolute reader grid: the segment start, or (ring) the stream's byte 0
    const uint64_t P = ring ? (A & ~kRingOffMask) : A;
    bool last_real = true;
    uint64_t last_start = A, last_ecand = ~0ull;

    // first candidate index with value >= A + effmin (uniform binary search)
    uint64_t lo = 0, hi = n;
    const uint64_t first = A + effmin;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (cands[mid] < first) lo = mid + 1; else hi = mid;
    }
    uint64_t wb = lo;  // window base: lane holds cands[wb + lane]
    uint64_t cv = (wb + lane < n) ? cands[wb + lane] : ~0ull;
    // suggested boundaries of this segment: same wave-wide window walk
    uint64_t swb = sbeg;
    uint64_t sv = (swb + lane < send) ? P + sugg[swb + lane] : ~0ull;

    while (s < B) {
        const uint64_t tlo = s + effmin, thi = s + maxsz;
        uint64_t c;
        for (;;) {
            const unsigned long long m = __ballot(cv >= tlo);
            if (m) {
                const int j = __ffsll((long long)m) - 1;
                c = __shfl(cv, j, 64);
                break;
            }
            wb += 64;
            // none of these 64 and none of the next 64 either: candidate-dense data lists thousands of candidates per MiB (a
            // subset of an overflowed tile's: DenseTiles) — jump to the first one >= tlo by binary search instead of stepping
            // (a stream whose every position is a candidate: 41 us per cut stepping through ~8 k entries, measured)
            if (wb + 63 < n && cands[wb + 63] < tlo) {
                uint64_t l2 = wb + 64, h2 = n;
                while (l2 < h2) {
                    const uint64_t mid = (l2 + h2) >> 1;
                    if (cands[mid] < tlo) l2 = mid + 1; else h2 = mid;
                }
                wb = l2;
            }
            cv = (wb + lane < n) ? cands[wb + lane] : ~0ull;
        }
        if (__builtin_expect(dz.tile_cnt != nullptr, 0)) c = dense_refine(dz, ds, tlo, min(thi, B), c);  // (some tile overflowed its slots)
        if (s == A && ecand_first != ~0ull) c = ecand_first;  // older than every listed candidate, >= tlo by construction
        const uint64_t e0 = (c < thi) ? c : thi;  // where the hash / max rule cuts, were the bytes there
        uint64_t e = (e0 > B) ? B : e0;
        bool real = e0 <= B;
        uint64_t ec = ~0ull;
        if (send > sbeg) {  // segment-uniform
            const uint64_t slo = s + cmin;
            uint64_t b;
            for (;;) {
                const unsigned long long m = __ballot(sv >= slo);  // lanes past the list hold ~0: always terminates
                if (m) {
                    b = __shfl(sv, __ffsll((long long)m) - 1, 64);
                    break;
                }
                swb += 64;
                sv = (swb + lane < send) ? P + sugg[swb + lane] : ~0ull;
            }
            if (fr.feed <= 1) {
                if (b <= e) {  // b >= s + min and b <= e <= s + max: a legal chunk (b == e: the same position, and a cut)
                    e = b;
                    real = true;
                }
            } else if (b <= B && b - s <= maxsz) {
                // the reference's payload chunker sees `feed` bytes per scan call: a boundary inside the call's buffer is
                // taken before the hash scan of that buffer runs, so it also wins over an EARLIER hash cut in the same
                // buffer; buffers are counted from the last cut, or (absolute) from the stream start
                const uint64_t ob = fr.absolute ? fr.origin + (b - P) : b - s, oe = fr.absolute ? fr.origin + (e - P) : e - s;
                const uint64_t jb = (ob - 1) / fr.feed, je = (oe - 1) / fr.feed;
                if (jb <= je) {
                    e = b;
                    real = true;
                }
            } else if (fr.open_end && b != ~0ull && b > B && b - s <= maxsz) {
                const uint64_t ob = fr.absolute ? fr.origin + (b - P) : b - s, oe = fr.absolute ? fr.origin + (e - P) : e - s;
                if ((ob - 1) / fr.feed <= (oe - 1) / fr.feed) {  // the cut is at b, beyond the bytes that are here: open chunk
                    if (e0 <= B && e0 == c) ec = c;              // ... and the hash cut it pre-empts still counts if the stream ends first
                    e = B;
                    real = false;
                }
            }
        }
        if (WRITE) {
            if (lane == (int)(k & 63u)) {
                my_end = e - A;
                my_size = (uint32_t)(e - s);
            }
            if ((k & 63u) == 63u) {  // records k - 63 .. k
                const uint64_t idx = rbase + (uint64_t)(k - 63u) + (uint64_t)lane;
                if (idx < rec_cap) {
                    pbsgpu_record *r = recs + idx;
                    r->end = my_end;
                    r->segment = seg;
                    r->size = my_size;
                }
            }
        }
        last_real = real;
        last_start = s;
        last_ecand = ec;
        ++k;
        s = e;
    }
    if (WRITE) {  // the last, partial group
        const uint32_t rest = k & 63u;
        const uint64_t idx = rbase + (uint64_t)(k - rest) + (uint64_t)lane;
        if ((uint32_t)lane < rest && idx < rec_cap) {
            pbsgpu_record *r = recs + idx;
            r->end = my_end;
            r->segment = seg;
            r->size = my_size;
        }
    }
    *last_real_out = last_real;
    *last_start_out = last_start;
    *ecand_out = last_ecand;
    return k;
}

}  // namespace pbsk
