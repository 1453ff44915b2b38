// The cut side's first two steps on gfx950: (1) the Buzhash candidate scan, the exclusive prefix scan over the tiles'
// counts, (2a) the compaction of the tiles' slots into one ascending candidate list. (Decomposition: kernels.h.)
#include <algorithm>
#include <type_traits>

#include "kernel_util.h"
#include "kernels.h"

namespace pbsk {

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// =====================================================================================
// (1) Buzhash candidate scan
// =====================================================================================
// h(i) = XOR_{k=0..63} rotl(T[b[i-k]], k mod 32): a pure function of the last 64 bytes, so every position is tested
// independently. The table is pre-rotated by r = 32-bits on the host: rotation commutes with the recurrence, and
// (h & mask) >= break_min becomes the single unsigned compare rotl(h,r) >= break_min << r, so no AND is needed per byte.
// (Rounds 1-5 kept two earlier kernels selectable for A/B runs — an LDS-tiled one, 2.28 TB/s, and a per-lane register
// streaming one, 4.36 TB/s: docs/NOTES.md. Gone with round 6: k_scan3 below is the scan.)
// -------------------------------------------------------------------------------------
// Candidate scan, cooperative-load form. Per-lane streaming of whole lines is bound by the texture addresser
// (64 distinct 128-byte lines per load instruction: 4.14 TB/s for pure loads, profiles/
// r01_ubench_load_pattern_ceiling.log), so here the four lanes of a quad fetch 64 CONTIGUOUS bytes of one
// strip per instruction (16 lines per instruction; 6.0 TB/s ceiling) and a small per-wave LDS stage
// transposes each 64-byte half-line back to "one lane = one strip": 4 ds_write_b128 at
// [strip][piece] with an 80-byte strip pitch, 4 ds_read_b128 of the lane's own row (pitch 5 slots, odd:
// conflict-free). A half-line is exactly one revolution of the 64-entry window ring, so ring indices
// stay static. D half-lines per wave are kept in flight (D x 4 KiB: memory-level parallelism). The hash
// runs in rolling form over two alternating rings of table values (see scan3_tile); pre-rotated 64x
// replicated table (every lane of a ds_read_b32 hits its own bank whatever the data byte), batched lookups, per-tile slot lists.
// Index algebra restated on CPU: tests/helpers.py::scan_coop_model.
#define PBS_LOOKUP3(w, k) \
    (*reinterpret_cast<const uint32_t *>(lds0 + __builtin_amdgcn_perm((w), lane4, 0x0c0c0400u | ((uint32_t)(k) << 8))))

// one tile of k_scan3. INTERIOR = the whole tile and its 64-byte warm-up lie inside the buffer (wave-uniform by
// construction): the check-free instantiation
template <int LINES, int D, bool INTERIOR>
__device__ __forceinline__ void scan3_tile(const ScanParams &p, const uint64_t t_idx, const uint64_t wbase, const uint64_t A,
                                           const int lane, const uint8_t *lds0, uint8_t *stage, uint32_t *wcnt) {
    constexpr uint32_t SL = LINES * 128;
    constexpr int PITCH = 80;
    constexpr int HALVES = LINES * 2;
    const uint64_t sbase = wbase + (uint64_t)lane * SL;
    const uint32_t thr = p.thr;
    const uint32_t lane4 = (uint32_t)lane << 2;
    const int q4 = lane & ~3, ql = lane & 3;

    // quad-cooperative fetch of half-line `hl` (64-byte units from the strip start; -1 = warm-up window):
    // instruction j serves strip q4 + j, this lane brings piece ql of it
    auto gfetch = [&](uint4 (&G)[4], const int hl) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t a = (int64_t)wbase + (int64_t)(q4 + j) * SL + (int64_t)hl * 64 + ql * 16;
            if constexpr (INTERIOR) {
                const uint4 v = *reinterpret_cast<const uint4 *>(p.data_al + a);
                G[j] = make_uint4(v.x, v.y, v.z, v.w);  // component-wise: a whole-struct store keeps G[][] in scratch
            } else {  // branch-free (a branch per load would force vmcnt(0) waits): clamp the address, select zero
                const bool in = a >= 0 && (uint64_t)a < A;
                const uint4 v = *reinterpret_cast<const uint4 *>(p.data_al + (in ? a : 0));
                G[j] = make_uint4(in ? v.x : 0u, in ? v.y : 0u, in ? v.z : 0u, in ? v.w : 0u);
            }
        }
    };
    // LDS transpose: [strip][piece] in, own row out (LDS operations of one wave execute in order)
    auto transpose = [&](const uint4 (&G)[4], uint4 (&X)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<uint4 *>(stage + (q4 + j) * PITCH + ql * 16) = G[j];
        wave_sync();
#pragma unroll
        for (int k = 0; k < 4; ++k) X[k] = *reinterpret_cast<const uint4 *>(stage + lane * PITCH + k * 16);
        wave_sync();
    };

    // Rolling form (window 64 == two 32-bit turns, so the outgoing term needs no rotation):
    //   h_i = rotl(h_{i-1}, 1) ^ t_i ^ t_{i-64},   t = pre-rotated table value of the byte
    // The table values of the previous 64 bytes live in a register ring; a half-line is exactly one turn of it,
    // so two rings alternate roles per half-line (lookups land directly in the "new" ring, no copies) and a
    // byte costs: 1 v_perm (LDS address) + 1 ds_read + 1 rotate + 1 three-input xor + 1/2 max3.
    uint32_t ring[2][64];
    uint32_t hc = 0;
    uint4 G[D][4], X[4];
    gfetch(G[0], -1);
    transpose(G[0], X);
#pragma unroll
    for (int d = 0; d < D; ++d) {
        gfetch(G[d], d);
        __builtin_amdgcn_sched_barrier(0);  // keep stage order: the loop's vmcnt waits assume oldest stage first
    }
    {   // warm-up over the 64 bytes before the strip (plays half-line -1: fills ring[1])
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const uint32_t w[4] = {X[g].x, X[g].y, X[g].z, X[g].w};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const uint32_t t = PBS_LOOKUP3(w[k >> 2], k & 3);
                ring[1][g * 16 + k] = t;
                hc = __builtin_rotateleft32(hc, 1) ^ t;
            }
        }
    }
    // one half-line: transpose stage d, (REFILL) put the stage's next half-line in flight, hash 64 bytes per lane
    auto half = [&](const int d, const int hl, auto refill_c) {
        uint32_t(&rn)[64] = ring[d & 1];        // hl and d have the same parity (D and the loop step are even)
        const uint32_t(&ro)[64] = ring[(d & 1) ^ 1];
        transpose(G[d], X);
        if constexpr (decltype(refill_c)::value) gfetch(G[d], hl + D);
        auto issue = [&](const int batch) {
            const uint4 &v = X[batch >> 1];
            const uint32_t w0 = (batch & 1) ? v.z : v.x, w1 = (batch & 1) ? v.w : v.y;
#pragma unroll
            for (int k = 0; k < 4; ++k) rn[batch * 8 + k] = PBS_LOOKUP3(w0, k);
#pragma unroll
            for (int k = 0; k < 4; ++k) rn[batch * 8 + 4 + k] = PBS_LOOKUP3(w1, k);
        };
        issue(0);
        uint32_t h[16];
        uint32_t acc = 0;
#pragma unroll
        for (int batch = 0; batch < 8; ++batch) {
            if (batch < 7) {
                issue(batch + 1);
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_waitcnt(0xC87F);  // lgkmcnt(8)
            } else {
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < 8; k += 2) {
                const int pos = batch * 8 + k;  // byte within the half-line == ring index
                const uint32_t h0 = __builtin_amdgcn_bitop3_b32(__builtin_rotateleft32(hc, 1), rn[pos], ro[pos], 0x96);
                const uint32_t h1 = __builtin_amdgcn_bitop3_b32(__builtin_rotateleft32(h0, 1), rn[pos + 1], ro[pos + 1], 0x96);
                h[pos & 15] = h0;
                h[(pos + 1) & 15] = h1;
                hc = h1;
                asm("v_max3_u32 %0, %1, %2, %3" : "=v"(acc) : "v"(acc), "v"(h0), "v"(h1));  // the compiler splits half of these
            }
            if (batch & 1) {
                if (__builtin_expect(acc >= thr, 0)) {  // rare: compact (mask + ctz loop), the hot loop has to stay small
                    uint32_t m = 0;
#pragma unroll
                    for (int k = 0; k < 16; ++k) m |= (h[k] >= thr) ? (1u << k) : 0u;
                    while (m) {
                        const uint32_t k = (uint32_t)__builtin_ctz(m);
                        m &= m - 1;
                        const uint64_t ea = sbase + (uint64_t)hl * 64u + (uint32_t)((batch >> 1) * 16) + k + 1u;
                        if (ea >= (uint64_t)p.lead + kWindow && ea <= A) {
                            const uint32_t slot = atomicAdd(wcnt, 1u);
                            if (slot < p.cap) p.tile_slots[t_idx * p.cap + slot] = (uint32_t)(ea - wbase);
                        }
                    }
                }
                acc = 0;
            }
        }
    };
    // steady state: every stage is refilled unconditionally (a conditional refill makes the compiler's vmcnt
    // bookkeeping pessimistic: it then waits for younger stages too); the last D half-lines are peeled
#pragma unroll 1
    for (int hl0 = 0; hl0 < HALVES - D; hl0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) half(d, hl0 + d, std::true_type{});
    }
#pragma unroll
    for (int d = 0; d < D; ++d) half(d, HALVES - D + d, std::false_type{});
}

template <int LINES, int D>
__global__ __launch_bounds__(512, 2) void k_scan3(ScanParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ __attribute__((aligned(1024))) uint32_t tab[256 * 64];  // [entry][lane]
    constexpr uint32_t SL = LINES * 128;
    constexpr uint64_t TILE = 64ull * SL;
    constexpr int PITCH = 80;
    static_assert((LINES * 2) % D == 0 && D % 2 == 0, "the half-line loop is unrolled by the (even) prefetch depth");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t *counters = reinterpret_cast<uint32_t *>(smem);
    uint8_t *stage = smem + 64 + wave * (64 * PITCH);
    for (int i = tid; i < 256 * 64; i += 512) tab[i] = p.table_rot[i >> 6];
    __syncthreads();

    uint32_t *wcnt = counters + wave;
    const uint64_t A = p.nbytes + p.lead;
    const uint8_t *lds0 = reinterpret_cast<const uint8_t *>(tab);

    // tiles_per_wave > 0: the workgroup retires after that many tiles per wave, so that the chip's dispatcher can place
    // other kernels' workgroups (the small resolve-chain kernels and SHA launches of the other batches in flight) on the
    // CU every fraction of a millisecond instead of after the whole scan (see launch_scan3)
    for (uint32_t done = 0; p.tiles_per_wave == 0 || done < p.tiles_per_wave; ++done) {
        unsigned long long g0 = 0;
        if (lane == 0) g0 = atomicAdd(p.tile_queue, 1ull);
        const uint64_t t_idx = __shfl(g0, 0, 64);
        if (t_idx >= p.ntiles) break;
        // flat range: tile t starts at t * TILE. Page ring: the tile's page comes from the round's page table — the
        // page's body is preceded by a 128-byte pad that holds the last bytes of the stream's previous page (the
        // window warm-up of the page's first strip), and only its `valid` bytes take part
        uint64_t wbase = t_idx * TILE, At = A;
        if (p.ring_pages) {
            const RingPage &pe = p.ring_pages[t_idx / p.ring_tpp];
            wbase = pe.phys_off + (t_idx % p.ring_tpp) * TILE;
            At = pe.phys_off + pe.valid;
        }
        if (lane == 0) *wcnt = 0;
        wave_sync();
        if (wbase < At) {
            if ((wbase >= 64) && (wbase + TILE <= At))
                scan3_tile<LINES, D, true>(p, t_idx, wbase, At, lane, lds0, stage, wcnt);
            else
                scan3_tile<LINES, D, false>(p, t_idx, wbase, At, lane, lds0, stage, wcnt);
        }
        wave_sync();
        if (lane == 0) p.tile_cnt[t_idx] = *wcnt;
        wave_sync();
    }
}
#undef PBS_LOOKUP3

template <int LINES, int D>
static hipError_t launch_scan3(const ScanParams &p, int num_cus, hipStream_t st) {
    constexpr size_t lds = 64 + 8 * 64 * 80;  // counters + 8 per-wave stages (40 KiB: also keeps SHA workgroups off this CU)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_scan3<LINES, D>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    uint64_t blocks = (p.ntiles + 7) / 8;
    // A scan workgroup fills its CU completely (244 VGPRs x 2 waves per SIMD, 104 KiB LDS). With PERSISTENT workgroups
    // (one per CU draining the tile queue) no other kernel can place a single wave anywhere for the 15-25 ms of a 64 GiB
    // scan — measured with 4 batches in flight: the small resolve-chain kernels of the OTHER batches took 11 ms instead
    // of 0.4-4.9 and their SHA launches started ~24 ms late. Hence a few CUs are never taken (16 of 256). (Workgroups that
    // retire after a few tiles so that the dispatcher interleaves everyone else were measured too: the resolve chains drop
    // from 13 to 9 ms but the scans stretch from 25 to 40 ms, no net gain — ScanParams::tiles_per_wave stays 0.)
    const uint64_t usable = (uint64_t)std::max(1, num_cus - (num_cus >= 64 ? 16 : 0));
    if (blocks > usable) blocks = usable;
    if (p.max_blocks && blocks > p.max_blocks) blocks = p.max_blocks;
    hipLaunchKernelGGL((k_scan3<LINES, D>), dim3((unsigned)blocks), dim3(512), lds, st, p);
    return hipGetLastError();
}

// half-lines in flight per wave: 4 (at 2 the kernel measured 4.66 instead of 4.90 TB/s, at 1 it is latency-bound: 3.96)
template <int LINES>
static hipError_t launch_scan3_any(const ScanParams &p, int num_cus, hipStream_t st) {
    return launch_scan3<LINES, 4>(p, num_cus, st);
}

uint32_t scan_tile_bytes(uint64_t nbytes) {
    return nbytes < (48ull << 20) ? 64u * 4u * 128u : 64u * 34u * 128u;  // (small batches: small tiles, so that the chip fills)
}

hipError_t launch_scan(const ScanParams &p, int num_cus, hipStream_t st) {
    if (p.ntiles == 0) return hipSuccess;
    if (p.tile_bytes == 64u * 34u * 128u) return launch_scan3_any<34>(p, num_cus, st);
    if (p.tile_bytes == 64u * 4u * 128u) return launch_scan3_any<4>(p, num_cus, st);
    return hipErrorInvalidValue;
}

// =====================================================================================
// exclusive scan of uint32 counts (three small kernels; inputs are <= a few M entries)
// =====================================================================================
constexpr int kScanBlockElems = 1024;  // 256 threads x 4

// block-wide exclusive scan of one value per thread (256 threads); returns exclusive prefix,
// *block_total gets the sum
__device__ __forceinline__ uint32_t block_excl_scan_256(uint32_t v, uint32_t *block_total) {
    __shared__ uint32_t wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_scan(v, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < wave; ++w) base += wsum[w];
    *block_total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    return base + incl - v;
}

__global__ __launch_bounds__(256) void k_scan_sums(const uint32_t *in, uint64_t n, uint32_t clamp, uint32_t *bsum,
                                                   uint32_t *maxval) {
    const uint64_t base = (uint64_t)blockIdx.x * kScanBlockElems + (uint64_t)threadIdx.x * 4;
    uint32_t s = 0, m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (base + k < n) {
            const uint32_t v = in[base + k];
            m = max(m, v);
            s += min(v, clamp);
        }
    }
    uint32_t total;
    (void)block_excl_scan_256(s, &total);
    // block max via wave reduce + atomic (rarely contended: one atomic per wave, only if it raises the max)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor(m, d, 64));
    if ((threadIdx.x & 63) == 0 && maxval && m > 0) atomicMax(maxval, m);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// single block: in-place exclusive scan of bsum[0..nb), total -> *total
__global__ __launch_bounds__(256) void k_scan_bsums(uint32_t *bsum, uint64_t nb, uint32_t *total) {
    __shared__ uint32_t carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (uint64_t c = 0; c < nb; c += 256) {
        const uint64_t i = c + threadIdx.x;
        const uint32_t v = (i < nb) ? bsum[i] : 0u;
        uint32_t tot;
        const uint32_t ex = block_excl_scan_256(v, &tot);
        const uint32_t carry = carry_s;
        if (i < nb) bsum[i] = carry + ex;
        __syncthreads();
        if (threadIdx.x == 0) carry_s = carry + tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry_s;
}

__global__ __launch_bounds__(256) void k_scan_apply(const uint32_t *in, uint64_t n, uint32_t clamp,
                                                    const uint32_t *bsum, uint32_t *out) {
    const uint64_t base = (uint64_t)blockIdx.x * kScanBlockElems + (uint64_t)threadIdx.x * 4;
    uint32_t v[4];
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = (base + k < n) ? min(in[base + k], clamp) : 0u;
        s += v[k];
    }
    uint32_t total;
    uint32_t ex = block_excl_scan_256(s, &total) + bsum[blockIdx.x];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (base + k < n) out[base + k] = ex;
        ex += v[k];
    }
}

size_t scan_tmp_words(uint64_t n) { return (size_t)((n + kScanBlockElems - 1) / kScanBlockElems) + 8; }

hipError_t launch_exclusive_scan(const uint32_t *in, uint64_t n, uint32_t clamp, uint32_t *out, uint32_t *total,
                                 uint32_t *maxval, uint32_t *tmp, hipStream_t st) {
    if (n == 0) return hipMemsetAsync(total, 0, sizeof(uint32_t), st);
    const uint64_t nb = (n + kScanBlockElems - 1) / kScanBlockElems;
    hipLaunchKernelGGL(k_scan_sums, dim3((unsigned)nb), dim3(256), 0, st, in, n, clamp, tmp, maxval);
    hipLaunchKernelGGL(k_scan_bsums, dim3(1), dim3(256), 0, st, tmp, nb, total);
    hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nb), dim3(256), 0, st, in, n, clamp, tmp, out);
    return hipGetLastError();
}

// =====================================================================================
// (2a) compaction: per-tile unordered slots -> dense ascending END offsets (caller coords)
// =====================================================================================
__global__ __launch_bounds__(256) void k_compact(const uint32_t *tile_cnt, const uint32_t *tile_off,
                                                 const uint32_t *tile_slots, uint32_t cap, uint64_t ntiles,
                                                 uint32_t lead, uint64_t *dense, uint64_t dense_cap,
                                                 uint32_t tile_bytes) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntiles) return;
    const uint32_t c = min(tile_cnt[t], cap);  // (a tile that found more keeps the first `cap` it recorded: see DenseTiles)
    if (c == 0) return;
    const uint32_t *sl = tile_slots + t * cap;
    const uint64_t base = tile_off[t];
    const uint64_t tbase = t * (uint64_t)tile_bytes;
    if (c <= 48) {  // the normal case (a handful of candidates per tile): rank by comparison
        for (uint32_t j = 0; j < c; ++j) {
            const uint32_t vj = sl[j];
            uint32_t rank = 0;
            for (uint32_t i = 0; i < c; ++i) rank += (sl[i] < vj) ? 1u : 0u;  // offsets within a tile are distinct
            if (base + rank < dense_cap) dense[base + rank] = tbase + vj - lead;
        }
        return;
    }
    // Dense tile (periodic / crafted input; the capacity-retry path): linear-time stable counting sort by lane strip.
    // A lane appends its own hits in ascending order (it walks its strip forwards and its LDS atomics execute in
    // program order), so the slot list is ascending WITHIN each strip and only interleaved ACROSS strips.
    const uint32_t strip = tile_bytes / 64u;
    uint32_t cnt[64];
    for (int i = 0; i < 64; ++i) cnt[i] = 0;
    for (uint32_t j = 0; j < c; ++j) cnt[min((sl[j] - 1u) / strip, 63u)]++;  // END offsets: 1..tile_bytes
    uint32_t run = 0;
    for (int i = 0; i < 64; ++i) {
        const uint32_t k = cnt[i];
        cnt[i] = run;
        run += k;
    }
    for (uint32_t j = 0; j < c; ++j) {
        const uint32_t vj = sl[j];
        const uint32_t pos = cnt[min((vj - 1u) / strip, 63u)]++;
        if (base + pos < dense_cap) dense[base + pos] = tbase + vj - lead;
    }
}

hipError_t launch_compact(const uint32_t *tile_cnt, const uint32_t *tile_off, const uint32_t *tile_slots,
                          uint32_t cap, uint64_t ntiles, uint32_t lead, uint64_t nbytes, uint64_t *dense,
                          uint64_t dense_cap, uint32_t tile_bytes, hipStream_t st) {
    (void)nbytes;
    if (ntiles == 0) return hipSuccess;
    const uint64_t nb = (ntiles + 255) / 256;
    hipLaunchKernelGGL(k_compact, dim3((unsigned)nb), dim3(256), 0, st, tile_cnt, tile_off, tile_slots, cap, ntiles,
                       lead, dense, dense_cap, tile_bytes);
    return hipGetLastError();
}

}  // namespace pbsk
