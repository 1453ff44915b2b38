// =====================================================================================
// XXH3-64 (seed 0, default secret) of many byte ranges — the per-file hash the reference tees
// new file bodies through (xxh3.New(), internal/pxarmount/commit_reuse.go:450-461) and re-checks
// after the commit (commit_orchestrate.go:485-562).
// =====================================================================================
// One wave per byte range (see xxh::blocks below); inputs <= 240 bytes take the scalar formulas.
#include <algorithm>

#include "kernels.h"

namespace pbsk {

__device__ constexpr uint8_t kXxhSecret[192] = {
    0xb8, 0xfe, 0x6c, 0x39, 0x23, 0xa4, 0x4b, 0xbe, 0x7c, 0x01, 0x81, 0x2c, 0xf7, 0x21, 0xad, 0x1c, 0xde, 0xd4, 0x6d, 0xe9,
    0x83, 0x90, 0x97, 0xdb, 0x72, 0x40, 0xa4, 0xa4, 0xb7, 0xb3, 0x67, 0x1f, 0xcb, 0x79, 0xe6, 0x4e, 0xcc, 0xc0, 0xe5, 0x78,
    0x82, 0x5a, 0xd0, 0x7d, 0xcc, 0xff, 0x72, 0x21, 0xb8, 0x08, 0x46, 0x74, 0xf7, 0x43, 0x24, 0x8e, 0xe0, 0x35, 0x90, 0xe6,
    0x81, 0x3a, 0x26, 0x4c, 0x3c, 0x28, 0x52, 0xbb, 0x91, 0xc3, 0x00, 0xcb, 0x88, 0xd0, 0x65, 0x8b, 0x1b, 0x53, 0x2e, 0xa3,
    0x71, 0x64, 0x48, 0x97, 0xa2, 0x0d, 0xf9, 0x4e, 0x38, 0x19, 0xef, 0x46, 0xa9, 0xde, 0xac, 0xd8, 0xa8, 0xfa, 0x76, 0x3f,
    0xe3, 0x9c, 0x34, 0x3f, 0xf9, 0xdc, 0xbb, 0xc7, 0xc7, 0x0b, 0x4f, 0x1d, 0x8a, 0x51, 0xe0, 0x4b, 0xcd, 0xb4, 0x59, 0x31,
    0xc8, 0x9f, 0x7e, 0xc9, 0xd9, 0x78, 0x73, 0x64, 0xea, 0xc5, 0xac, 0x83, 0x34, 0xd3, 0xeb, 0xc3, 0xc5, 0x81, 0xa0, 0xff,
    0xfa, 0x13, 0x63, 0xeb, 0x17, 0x0d, 0xdd, 0x51, 0xb7, 0xf0, 0xda, 0x49, 0xd3, 0x16, 0x55, 0x26, 0x29, 0xd4, 0x68, 0x9e,
    0x2b, 0x16, 0xbe, 0x58, 0x7d, 0x47, 0xa1, 0xfc, 0x8f, 0xf8, 0xb8, 0xd1, 0x7a, 0xd0, 0x31, 0xce, 0x45, 0xcb, 0x3a, 0x8f,
    0x95, 0x16, 0x04, 0x28, 0xaf, 0xd7, 0xfb, 0xca, 0xbb, 0x4b, 0x40, 0x7e};

namespace xxh {
constexpr uint64_t P32_1 = 0x9E3779B1ull, P32_2 = 0x85EBCA77ull, P32_3 = 0xC2B2AE3Dull;
constexpr uint64_t P64_1 = 0x9E3779B185EBCA87ull, P64_2 = 0xC2B2AE3D27D4EB4Full, P64_3 = 0x165667B19E3779F9ull;
constexpr uint64_t P64_4 = 0x85EBCA77C2B2AE63ull, P64_5 = 0x27D4EB2F165667C5ull;
constexpr uint64_t PMX1 = 0x165667919E3779F9ull, PMX2 = 0x9FB21C651E98DF25ull;

__device__ __forceinline__ uint64_t sec64(int off) {  // little-endian 8 bytes of the secret (any offset)
    uint64_t v = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) v |= (uint64_t)kXxhSecret[off + b] << (8 * b);
    return v;
}
__device__ __forceinline__ uint64_t sec64_dyn(int off) {
    uint64_t v = 0;
    for (int b = 0; b < 8; ++b) v |= (uint64_t)kXxhSecret[off + b] << (8 * b);
    return v;
}
__device__ __forceinline__ uint64_t rd64(const uint8_t *p) {  // byte-safe little-endian load
    uint64_t v = 0;
    for (int b = 0; b < 8; ++b) v |= (uint64_t)p[b] << (8 * b);
    return v;
}
__device__ __forceinline__ uint32_t rd32(const uint8_t *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__device__ __forceinline__ uint64_t rotl64(uint64_t x, int n) { return (x << n) | (x >> (64 - n)); }
__device__ __forceinline__ uint64_t fold128(uint64_t a, uint64_t b) { return (a * b) ^ __umul64hi(a, b); }
__device__ __forceinline__ uint64_t avalanche(uint64_t h) {
    h ^= h >> 37;
    h *= PMX1;
    return h ^ (h >> 32);
}
__device__ __forceinline__ uint64_t avalanche64(uint64_t h) {
    h ^= h >> 33;
    h *= P64_2;
    h ^= h >> 29;
    h *= P64_3;
    return h ^ (h >> 32);
}
__device__ __forceinline__ uint64_t mix16(const uint8_t *d, int so) {
    return fold128(rd64(d) ^ sec64_dyn(so), rd64(d + 8) ^ sec64_dyn(so + 8));
}
// inputs of 0..240 bytes (one lane)
__device__ uint64_t short_hash(const uint8_t *d, uint64_t n) {
    if (n == 0) return avalanche64(sec64(56) ^ sec64(64));
    if (n <= 3) {
        const uint32_t comb = ((uint32_t)d[0] << 16) | ((uint32_t)d[n >> 1] << 24) | (uint32_t)d[n - 1] | ((uint32_t)n << 8);
        const uint32_t flip = (uint32_t)sec64(0) ^ (uint32_t)(sec64(0) >> 32);
        return avalanche64((uint64_t)(comb ^ flip));
    }
    if (n <= 8) {
        const uint64_t in1 = rd32(d), in2 = rd32(d + n - 4);
        uint64_t h = (in2 + (in1 << 32)) ^ (sec64(8) ^ sec64(16));
        h ^= rotl64(h, 49) ^ rotl64(h, 24);
        h *= PMX2;
        h ^= (h >> 35) + n;
        h *= PMX2;
        return h ^ (h >> 28);
    }
    if (n <= 16) {
        const uint64_t lo = rd64(d) ^ (sec64(24) ^ sec64(32));
        const uint64_t hi = rd64(d + n - 8) ^ (sec64(40) ^ sec64(48));
        return avalanche(n + __builtin_bswap64(lo) + hi + fold128(lo, hi));
    }
    if (n <= 128) {
        uint64_t acc = n * P64_1;
        if (n > 32) {
            if (n > 64) {
                if (n > 96) acc += mix16(d + 48, 96) + mix16(d + n - 64, 112);
                acc += mix16(d + 32, 64) + mix16(d + n - 48, 80);
            }
            acc += mix16(d + 16, 32) + mix16(d + n - 32, 48);
        }
        acc += mix16(d, 0) + mix16(d + n - 16, 16);
        return avalanche(acc);
    }
    uint64_t acc = n * P64_1;
    for (int i = 0; i < 8; ++i) acc += mix16(d + 16 * i, 16 * i);
    acc = avalanche(acc);
    const int rounds = (int)(n / 16);
    for (int i = 8; i < rounds; ++i) acc += mix16(d + 16 * i, 16 * (i - 8) + 3);
    acc += mix16(d + n - 16, 136 - 17);
    return avalanche(acc);
}
}  // namespace xxh

// ---- long inputs (> 240 bytes): one WAVE per byte range ---------------------------------------------------
// XXH3's 512-bit state is 8 u64 accumulators; inside a 1 KiB block (16 stripes of 64 bytes) the update is a SUM
//   acc[i] += data64[i ^ 1] + lo32(data64[i] ^ key[s][i]) * hi32(data64[i] ^ key[s][i])
// and only the per-block scramble is non-linear. So all 64 lanes take part: lane = (stripe-in-half-block s8 =
// lane >> 3, accumulator i = lane & 7) adds its two stripes of the block (two fully coalesced 512-byte wave loads),
// the 8 partial sums per accumulator are reduced with three butterfly steps, and every lane applies the scramble to
// its (replicated) accumulator. Loads are byte-aligned 8-byte loads (gfx950 global loads are alignment-free).
namespace xxh {

// streaming state of ONE open byte range (the stream writer's per-file tee); hist sits directly in front of pend so
// that the final stripe (the last 64 bytes of the whole input) can be read at pend + pend_len - 64 even when fewer
// than 64 bytes are pending
struct State {
    uint64_t acc[8];
    uint64_t total;      // bytes seen so far
    uint32_t pend_len;   // bytes waiting in pend (1..1024 once anything was seen)
    uint32_t started;
    uint8_t hist[64];
    uint8_t pend[1024];
};

struct Keys {
    uint64_t k0, k1;     // stripe keys of this lane for the two half-blocks: secret[8 * (s8 + 8h) + 8 i ..]
    uint64_t scr, last, merge;
};

__device__ __forceinline__ Keys make_keys(int lane) {
    const int i = lane & 7, s8 = lane >> 3;
    Keys k;
    k.k0 = sec64_dyn(8 * s8 + 8 * i);
    k.k1 = sec64_dyn(8 * (s8 + 8) + 8 * i);
    k.scr = sec64_dyn(128 + 8 * i);
    k.last = sec64_dyn(121 + 8 * i);
    k.merge = sec64_dyn(11 + 8 * i);
    return k;
}

__device__ __forceinline__ uint64_t ld64(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

__device__ __forceinline__ uint64_t stripe_term(uint64_t v, uint64_t key) {
    const uint64_t nb = __shfl_xor(v, 1, 64);  // the neighbour accumulator's data word
    const uint64_t k = v ^ key;
    return nb + (uint64_t)(uint32_t)k * (uint64_t)(uint32_t)(k >> 32);
}

__device__ __forceinline__ uint64_t reduce_stripes(uint64_t part) {  // sum over the 8 lanes that share `i`
    part += __shfl_xor(part, 8, 64);
    part += __shfl_xor(part, 16, 64);
    part += __shfl_xor(part, 32, 64);
    return part;
}

// Phase A — block sums. S_b[i] = sum over the 16 stripes of block b of the accumulate term; it does not depend on the
// accumulators, so every block of every input is an independent unit of work for any wave of the grid (perfect load
// balance whatever the file-size mix). Returned in all lanes (replicated over the 8 lanes with equal i).
__device__ __forceinline__ uint64_t block_sum(const uint8_t *blk, const Keys &k, int lane) {
    const uint8_t *q = blk + 8 * lane;  // 64 * s8 + 8 * i == 8 * lane
    return reduce_stripes(stripe_term(ld64(q), k.k0) + stripe_term(ld64(q + 512), k.k1));
}

// Phase B — the only serial part of a long input: acc = scramble(acc + S_b), block after block (~10 instructions each).
// S entries are 8 u64 per block; the next entries are in flight while one is applied.
__device__ __forceinline__ void chain(uint64_t &acc, const uint64_t *S, uint64_t nblk, const Keys &k, int lane) {
    const uint64_t *q = S + (lane & 7);
    constexpr int U = 8;
    uint64_t b = 0;
    for (; b + U <= nblk; b += U) {
        uint64_t v[U];
#pragma unroll
        for (int j = 0; j < U; ++j) v[j] = q[(b + j) * 8];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            acc += v[j];
            acc ^= acc >> 47;
            acc ^= k.scr;
            acc *= P32_1;
        }
    }
    for (; b < nblk; ++b) {
        acc += q[b * 8];
        acc ^= acc >> 47;
        acc ^= k.scr;
        acc *= P32_1;
    }
}

// the tail of a long input: `rem` = the R (1..1024) bytes behind the last full block, n = total length (> 240);
// the 64 bytes in front of rem must be readable when R < 64 (the input itself, or State::hist)
__device__ __forceinline__ uint64_t finish_long(uint64_t acc, const uint8_t *rem, uint32_t R, uint64_t n, const Keys &k,
                                                int lane) {
    const int i = lane & 7, s8 = lane >> 3;
    const uint32_t nstripes = (R - 1) / 64;  // full stripes that are NOT the last one
    uint64_t part = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t st = (uint32_t)s8 + 8u * h;
        const bool on = st < nstripes;                       // octet-uniform
        const uint64_t v = on ? ld64(rem + 64 * st + 8 * i) : 0;
        const uint64_t t = stripe_term(v, h ? k.k1 : k.k0);  // shuffles stay wave-converged
        part += on ? t : 0;
    }
    acc += reduce_stripes(part);
    acc += stripe_term(ld64(rem + R - 64 + 8 * i), k.last);  // last stripe: the final 64 bytes of the input
    const uint64_t mine = acc ^ k.merge;
    const uint64_t other = __shfl_xor(mine, 1, 64);
    uint64_t fold = ((i & 1) == 0) ? fold128(mine, other) : 0;
    fold += __shfl_xor(fold, 2, 64);
    fold += __shfl_xor(fold, 4, 64);
    return avalanche(n * P64_1 + fold);
}

__device__ __forceinline__ uint64_t init_acc(int lane) {
    const uint64_t init[8] = {P32_3, P64_1, P64_2, P64_3, P64_4, P32_2, P64_5, P32_1};
    uint64_t a = init[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) a = ((lane & 7) == j) ? init[j] : a;
    return a;
}

// whole input in one piece; S = its block sums (phase A)
__device__ __forceinline__ uint64_t one_shot(const uint8_t *d, uint64_t n, const uint64_t *S, const Keys &k, int lane) {
    if (n <= 240) return short_hash(d, n);  // every lane computes it (wave-uniform branch); cheap
    uint64_t acc = init_acc(lane);
    const uint64_t nblk = (n - 1) / 1024;
    chain(acc, S, nblk, k, lane);
    return finish_long(acc, d + nblk * 1024, (uint32_t)(n - nblk * 1024), n, k, lane);
}

// global memory written by some lanes of this wave is about to be read by others (or the reverse): complete the
// outstanding accesses first (workgroup-scope fences: one L1 per CU, no cache maintenance, just the waits)
__device__ __forceinline__ void mem_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ void wave_copy(uint8_t *dst, const uint8_t *src, uint32_t n, int lane) {
    for (uint32_t j = lane; j < n; j += 64) dst[j] = src[j];
}

// one piece of an input that arrives in several pieces (stream windows). flags: 1 = first piece, 2 = last piece.
// Blocks are consumed only while at least one more byte is known to follow (XXH3 treats the final <= 1024 bytes
// specially), so between pieces 1..1024 bytes wait in State::pend. The HOST mirrors the pending length (pure
// arithmetic on the piece lengths) and passes it with the number of blocks to consume now (nproc); phase A has already
// completed the pending block in place (if any) and summed all nproc blocks into S.
__device__ __forceinline__ bool piece(State *st, const uint8_t *p, uint64_t L, uint32_t flags, uint32_t pend,
                                      uint64_t nproc, const uint64_t *S, const Keys &k, int lane, uint64_t *result) {
    const bool first = (flags & 1u) != 0;
    uint64_t acc = first ? init_acc(lane) : st->acc[lane & 7];
    const uint64_t before = first ? 0ull : st->total;
    const uint64_t T = (uint64_t)pend + L;
    if (nproc) {
        chain(acc, S, nproc, k, lane);
        const uint64_t used = nproc * 1024 - pend;  // bytes of p inside the consumed blocks
        // history = the 64 bytes in front of the new pending tail
        uint8_t hb;
        if (used >= 64) hb = p[used - 64 + lane];
        else hb = (lane < 64 - (int)used) ? st->pend[1024 - (64 - used) + lane] : p[lane - (64 - used)];
        mem_sync();  // the completed pending block has been read by every lane before it is overwritten
        st->hist[lane] = hb;
        const uint32_t rest = (uint32_t)(L - used);
        wave_copy(st->pend, p + used, rest, lane);
        pend = rest;
    } else if (L) {
        wave_copy(st->pend + pend, p, (uint32_t)L, lane);
        pend = (uint32_t)T;
    }
    const uint64_t total = before + L;
    if (lane < 8) st->acc[lane] = acc;
    if (lane == 0) { st->total = total; st->pend_len = pend; st->started = 1; }
    mem_sync();  // pend / hist written by other lanes are read below
    if (!(flags & 2u)) return false;
    if (total <= 240) *result = short_hash(st->pend, total);  // nothing was ever consumed: pend holds the whole input
    else *result = finish_long(acc, st->pend, pend, total, k, lane);
    return true;
}
}  // namespace xxh

// Work item of the XXH3 kernels: hash bytes [ptr, ptr + len). flags bit0 = first piece of its input, bit1 = last piece;
// both set = a whole input (no state). Pieces of one input must be issued in order on one stream. pend / nproc / s_off
// are filled by the host (xxh3_plan): pending bytes in front of this piece, full 1 KiB blocks to consume now, index of
// the item's first block-sum entry.
// Phase A: one unit = kRun consecutive blocks of the global block list (all inputs back to back).
constexpr uint32_t kXxhRun = 16;
__global__ __launch_bounds__(256) void k_xxh3_sums(const XxhItem *items, uint32_t nitems, uint64_t total_blocks,
                                                   xxh::State *states, uint64_t *S) {
    using namespace xxh;
    const int lane = threadIdx.x & 63;
    const Keys k = make_keys(lane);
    const uint64_t nunits = (total_blocks + kXxhRun - 1) / kXxhRun;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t u = wave; u < nunits; u += nwaves) {
        uint64_t g = u * kXxhRun;
        const uint64_t gend = min(g + kXxhRun, total_blocks);
        // item that owns block g: last item with s_off <= g (items are in s_off order; empty items share an offset)
        uint32_t lo = 0, hi = nitems;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (items[mid].s_off <= g) lo = mid; else hi = mid;
        }
        uint32_t it = lo;
        while (g < gend) {
            while (it + 1 < nitems && (items[it].nproc == 0 || g >= items[it].s_off + items[it].nproc)) ++it;
            const XxhItem item = items[it];
            const uint64_t j = g - item.s_off;  // block of this item
            const uint8_t *blk;
            if (item.pend) {
                State *st = states + item.state;
                const uint32_t take = 1024u - item.pend;
                if (j == 0) {  // complete the pending block in place (this wave is its only reader in this phase)
                    wave_copy(st->pend + item.pend, item.ptr, take, lane);
                    mem_sync();
                    blk = st->pend;
                } else {
                    blk = item.ptr + take + (j - 1) * 1024;
                }
            } else {
                blk = item.ptr + j * 1024;
            }
            const uint64_t sum = block_sum(blk, k, lane);
            if (lane < 8) S[g * 8 + lane] = sum;
            ++g;
        }
    }
}

// Phase B: one wave per item
__global__ __launch_bounds__(256) void k_xxh3(const XxhItem *items, uint32_t nitems, xxh::State *states, const uint64_t *S,
                                              uint64_t *out, uint32_t *queue) {
    using namespace xxh;
    const int lane = threadIdx.x & 63;
    const Keys k = make_keys(lane);
    for (;;) {
        uint32_t idx = 0;
        if (lane == 0) idx = atomicAdd(queue, 1u);
        idx = __shfl(idx, 0, 64);
        if (idx >= nitems) break;
        const XxhItem it = items[idx];
        uint64_t h = 0;
        bool done;
        if ((it.flags & 3u) == 3u) {
            h = one_shot(it.ptr, it.len, S + it.s_off * 8, k, lane);
            done = true;
        } else {
            done = piece(states + it.state, it.ptr, it.len, it.flags, it.pend, it.nproc, S + it.s_off * 8, k, lane, &h);
        }
        if (done && lane == 0) out[it.out] = h;
    }
}

// fills pend-independent plan fields of whole inputs and returns the total number of blocks (host side)
uint64_t xxh3_plan_whole(XxhItem *items, uint32_t n) {
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        items[i].pend = 0;
        items[i].nproc = items[i].len > 240 ? (uint32_t)((items[i].len - 1) / 1024) : 0u;
        items[i].s_off = total;
        total += items[i].nproc;
    }
    return total;
}

size_t xxh3_state_bytes() { return sizeof(xxh::State); }

hipError_t launch_xxh3_items(const XxhItem *items, uint32_t nitems, uint64_t total_blocks, void *states, uint64_t *sums,
                             uint64_t *out, uint32_t *queue, int num_cus, hipStream_t st) {
    if (nitems == 0) return hipSuccess;
    if (total_blocks) {
        const uint64_t units = (total_blocks + kXxhRun - 1) / kXxhRun;
        unsigned grid = (unsigned)std::min<uint64_t>((units + 3) / 4, (uint64_t)num_cus * 8u);
        hipLaunchKernelGGL(k_xxh3_sums, dim3(grid), dim3(256), 0, st, items, nitems, total_blocks, (xxh::State *)states, sums);
    }
    unsigned grid = (unsigned)num_cus * 2u;  // 8 waves per CU
    const unsigned need = (nitems + 3) / 4;
    if (grid > need) grid = need;
    hipLaunchKernelGGL(k_xxh3, dim3(grid), dim3(256), 0, st, items, nitems, (xxh::State *)states, (const uint64_t *)sums, out,
                       queue);
    return hipGetLastError();
}

}  // namespace pbsk
