// (3) SHA-256 of the chunks on gfx950, and nothing else: the four kernel families (one lane per chunk, the lanes service,
// wave pairs, the express form), the longest-first queue order, and their launchers for the batch path and for the page
// ring's persistent services. Every SHA-256 kernel is instantiated here and nowhere else, so this file's object changes
// only when SHA-256 does. (Decomposition and the other kernel files: kernels.h.)
#include "kernel_util.h"
#include "kernels.h"
#include "ring_queue.h"
#include "sha256_suffix.h"

#include <type_traits>

namespace pbsk {

// =====================================================================================
// (3) SHA-256 — one lane per byte range, lanes pull ranges from a queue
// =====================================================================================
__device__ __forceinline__ uint32_t rotr(uint32_t x, int n) { return __builtin_rotateright32(x, n); }

// gfx950 has v_bitop3_b32 (any 3-input bitwise op in one instruction): XOR3 = 0x96, MAJ = 0xE8.
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}
__device__ __forceinline__ uint32_t maj3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8);
}
__device__ __forceinline__ uint32_t ch3(uint32_t e, uint32_t f, uint32_t g) { return g ^ (e & (f ^ g)); }  // v_bfi

__device__ constexpr uint32_t kSha256K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

// message schedule step: W[i & 15] <- sigma1(W[i-2]) + W[i-7] + sigma0(W[i-15]) + W[i-16]
__device__ __forceinline__ uint32_t sha256_sched(uint32_t (&W)[16], int i) {
    const uint32_t w15 = W[(i + 1) & 15], w2 = W[(i + 14) & 15];
    const uint32_t s0 = xor3(rotr(w15, 7), rotr(w15, 18), w15 >> 3);
    const uint32_t s1 = xor3(rotr(w2, 17), rotr(w2, 19), w2 >> 10);
    const uint32_t w = W[i & 15] + s0 + W[(i + 9) & 15] + s1;
    W[i & 15] = w;
    return w;
}

// one round given wk = W[t] + K[t]; 14 VALU instructions (3+1 Sigma1, bfi, 2 adds, 3+1 Sigma0, maj, 2 adds)
#define SHA256_ROUND(a, b, c, d, e, f, g, h, wk)                                   \
    do {                                                                           \
        const uint32_t t1_ = (h) + xor3(rotr(e, 6), rotr(e, 11), rotr(e, 25)) + ch3(e, f, g) + (wk); \
        const uint32_t t2_ = xor3(rotr(a, 2), rotr(a, 13), rotr(a, 22)) + maj3(a, b, c); \
        (d) += t1_;                                                                \
        (h) = t1_ + t2_;                                                           \
    } while (0)

__device__ __forceinline__ void sha256_compress(uint32_t (&H)[8], uint32_t (&W)[16]) {
    uint32_t a = H[0], b = H[1], c = H[2], d = H[3], e = H[4], f = H[5], g = H[6], h = H[7];
#pragma unroll
    for (int i = 0; i < 64; i += 8) {
        uint32_t wk[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) wk[j] = ((i + j < 16) ? W[i + j] : sha256_sched(W, i + j)) + kSha256K[i + j];
        SHA256_ROUND(a, b, c, d, e, f, g, h, wk[0]);
        SHA256_ROUND(h, a, b, c, d, e, f, g, wk[1]);
        SHA256_ROUND(g, h, a, b, c, d, e, f, wk[2]);
        SHA256_ROUND(f, g, h, a, b, c, d, e, wk[3]);
        SHA256_ROUND(e, f, g, h, a, b, c, d, wk[4]);
        SHA256_ROUND(d, e, f, g, h, a, b, c, wk[5]);
        SHA256_ROUND(c, d, e, f, g, h, a, b, wk[6]);
        SHA256_ROUND(b, c, d, e, f, g, h, a, wk[7]);
    }
    H[0] += a; H[1] += b; H[2] += c; H[3] += d; H[4] += e; H[5] += f; H[6] += g; H[7] += h;
}

__device__ __forceinline__ void sha256_iv(uint32_t (&H)[8]) {
    H[0] = 0x6a09e667; H[1] = 0xbb67ae85; H[2] = 0x3c6ef372; H[3] = 0xa54ff53a;
    H[4] = 0x510e527f; H[5] = 0x9b05688c; H[6] = 0x1f83d9ab; H[7] = 0x5be0cd19;
}

// What a producer lane WITHOUT a data block requests in a step (and ignores). The request itself is unconditional, FIVE
// loads in every step of every lane: only then does the number of requests issued after a slot's own five not depend on
// the path taken, and the compiler can await a slot with `s_waitcnt vmcnt(5)` — the other slot's requests stay in flight
// — instead of vmcnt(0). (A branch around the loads, even a wave-uniform one, brings the vmcnt(0) back.)
__device__ uint32_t kIdleBlock[32];

// Request the 64 bytes at p (+ the 4 behind them if p is not 4-byte aligned) as raw little-endian dwords; `sel` = the
// v_perm selector that byte-swaps and funnels them into big-endian message words.
__device__ __forceinline__ void sha256_request_block(const uint8_t *p, uint32_t (&R)[17], uint32_t &sel) {
    const uint32_t o = (uint32_t)((uintptr_t)p & 3u);
    const gvec4_ptr q = (gvec4_ptr)(p - o);
    const u32x4_a4 v0 = q[0], v1 = q[1], v2 = q[2], v3 = q[3];
    R[0] = v0.x; R[1] = v0.y; R[2] = v0.z; R[3] = v0.w;
    R[4] = v1.x; R[5] = v1.y; R[6] = v1.z; R[7] = v1.w;
    R[8] = v2.x; R[9] = v2.y; R[10] = v2.z; R[11] = v2.w;
    R[12] = v3.x; R[13] = v3.y; R[14] = v3.z; R[15] = v3.w;
    R[16] = ((gword_ptr)(p - o))[o ? 16 : 15];  // aligned: nothing behind the block is touched (the word is not selected)
    sel = ((o) << 24) | ((o + 1) << 16) | ((o + 2) << 8) | (o + 3);
}

// Raw little-endian words of a block that is NOT 64 full data bytes (the last data bytes + 0x80 marker, zero fill, and
// the big-endian bit length in the final block): the funnel-shifted data words come from aligned dword loads whose
// addresses are clamped to the range's last valid dword (nothing beyond the chunk is touched), then everything behind the
// data is masked off and the marker / length are or-ed in. ~130 instructions with 17 independent loads in flight — the
// byte-at-a-time assembly this replaces cost dozens of DEPENDENT byte loads per tail, which at small chunk sizes (a tail
// every ~1000 blocks per lane, i.e. one per ~16 wave iterations) is what held the hash kernels back.
__device__ __forceinline__ void sha256_tail_words(const uint8_t *base, uint64_t len, uint64_t off, bool last, uint32_t (&R)[17]) {
    const int64_t rem = (int64_t)len - (int64_t)off;                // data bytes from `off` on (<= 0: padding-only block)
    const uint32_t valid = rem <= 0 ? 0u : (rem >= 64 ? 64u : (uint32_t)rem);
    uint32_t q[17];
#pragma unroll
    for (int j = 0; j < 17; ++j) q[j] = 0;
    uint32_t o = 0;
    if (valid) {
        const uint8_t *p = base + off;
        o = (uint32_t)((uintptr_t)p & 3u);
        const gword_ptr a = (gword_ptr)(p - o);
        const uint32_t jmax = (o + valid - 1u) >> 2;               // last dword that holds a valid byte
#pragma unroll
        for (int j = 0; j < 17; ++j) q[j] = a[min((uint32_t)j, jmax)];
    }
    const uint32_t sh = o * 8u;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        uint32_t w = sh ? ((q[j] >> sh) | (q[j + 1] << (32u - sh))) : q[j];  // bytes off+4j .. off+4j+3, little-endian
        const int32_t k = (int32_t)valid - 4 * j;                  // valid bytes in this word
        const uint32_t mask = k >= 4 ? 0xffffffffu : (k <= 0 ? 0u : ((1u << (8 * k)) - 1u));
        w &= mask;
        if (rem >= 0 && rem < 64 && k >= 0 && k < 4) w |= 0x80u << (8 * k);  // the marker byte sits at position len
        R[j] = w;
    }
    if (last) {  // big-endian bit length in bytes 56..63 (R is little-endian raw)
        const uint64_t bits = len * 8;
        R[14] = __builtin_bswap32((uint32_t)(bits >> 32));
        R[15] = __builtin_bswap32((uint32_t)bits);
    }
    R[16] = 0;
}

// Work source for the SHA kernel: item i -> (byte pointer, length, digest destination)
struct RecordSource {
    static constexpr bool kRing = false;
    pbsgpu_record *recs;
    // queue position -> {chunk address lo, hi, size, record index}, longest chunks first (k_order). ONE 16-byte load
    // per chunk a lane takes from the queue: the chain order[i] -> record -> segment offset was three dependent round
    // trips (~1-2 us each under load) at every chunk boundary of every lane, and all pairs of a workgroup wait at the
    // block barrier while one producer sits in them.
    const uint4 *qdesc;
    __device__ __forceinline__ void get(uint32_t i, const uint8_t *&ptr, uint64_t &len, uint8_t *&dst) const {
        const uint4 d = qdesc[i];
        ptr = reinterpret_cast<const uint8_t *>(((uint64_t)d.y << 32) | d.x);
        len = d.z;
        dst = recs[d.w].digest;
    }
};
struct SegmentSource {
    static constexpr bool kRing = false;
    const uint8_t *data;
    const pbsgpu_segment *segs;
    uint8_t *digests;
    __device__ __forceinline__ void get(uint32_t i, const uint8_t *&ptr, uint64_t &len, uint8_t *&dst) const {
        ptr = data + segs[i].offset;
        len = segs[i].length;
        dst = digests + (uint64_t)i * 32;
    }
};

// KEYED digests, SHA-256(content || id_key): the index digest of an encrypted backup's chunk. The keyed twins
// of the two batch sources carry the key's eight words (device memory of a pbsgpu_id_key, never written while a kernel runs:
// read through the constant address space, i.e. with scalar loads, inside the tail branch only) and the compile-time count of
// suffix bytes. A source WITHOUT kSuffixBytes (RecordSource, SegmentSource, RingSource: not edited) has none, and every
// `if constexpr` below then leaves exactly the code there was: the plain kernels' ISA does not change.
template <typename S, typename = void>
struct SuffixOf {
    static constexpr uint32_t kBytes = 0;
};
template <typename S>
struct SuffixOf<S, std::void_t<decltype(S::kSuffixBytes)>> {
    static constexpr uint32_t kBytes = S::kSuffixBytes;
};
struct KeyedRecordSource : RecordSource {
    static constexpr uint32_t kSuffixBytes = pbss::kSuffixBytes;
    const uint32_t *key;
};
struct KeyedSegmentSource : SegmentSource {
    static constexpr uint32_t kSuffixBytes = pbss::kSuffixBytes;
    const uint32_t *key;
};
typedef const __attribute__((address_space(4))) uint32_t *kword_ptr;

// sha256_tail_words for a keyed chunk: the same clamped dword loads and funnel shift for the data words, then
// pbss::sha256_suffix_block (sha256_suffix.h: registers only, the CPU test runs the same function) decides what every byte
// of the block is. At most two such blocks per chunk (63 + 32 + 9 < 128).
__device__ __forceinline__ void sha256_tail_words_keyed(const uint8_t *base, uint64_t len, uint64_t off, bool last, const uint32_t *key,
                                                        uint32_t (&R)[17]) {
    const int64_t rem = (int64_t)len - (int64_t)off;                // data bytes from `off` on: < 64 here, <= 0 = none
    const uint32_t valid = rem <= 0 ? 0u : (uint32_t)rem;
    uint32_t q[17];
#pragma unroll
    for (int j = 0; j < 17; ++j) q[j] = 0;
    uint32_t o = 0;
    if (valid) {
        const uint8_t *p = base + off;
        o = (uint32_t)((uintptr_t)p & 3u);
        const gword_ptr a = (gword_ptr)(p - o);
        const uint32_t jmax = (o + valid - 1u) >> 2;               // last dword that holds a valid byte
#pragma unroll
        for (int j = 0; j < 17; ++j) q[j] = a[min((uint32_t)j, jmax)];
    }
    const uint32_t sh = o * 8u;
    uint32_t d[16], k[pbss::kSuffixWords], out[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) d[j] = sh ? ((q[j] >> sh) | (q[j + 1] << (32u - sh))) : q[j];
#pragma unroll
    for (int j = 0; j < (int)pbss::kSuffixWords; ++j) k[j] = ((kword_ptr)key)[j];
    pbss::sha256_suffix_block(d, valid, len, off, k, last, out);
#pragma unroll
    for (int j = 0; j < 16; ++j) R[j] = out[j];
    R[16] = 0;
}

// The page ring's SHA-256 SERVICE (ring.cpp): one persistent launch whose lanes pull chunk descriptors from a
// device-resident FIFO that the cut rounds of ALL streams append to (k_ring_order / k_ring_publish), so a chunk starts
// hashing the moment it has been cut, whichever round, stream or page it came from, and every lane that finishes a chunk
// takes the next one — no batch-granular makespan, no batch-granular buffer release.
//   * a lane CLAIMS queue positions with one wave-level atomicAdd on `head` and then waits for `tail` to pass its
//     position (positions are unique and every position is eventually published, or `stop` is raised);
//   * a chunk may cross from one physical page into another (pages of a stream are not adjacent): the descriptor
//     carries both piece addresses; a block that starts in the first piece reads on into the page's 128-byte tail pad,
//     which mirrors the first bytes of the stream's next page;
//   * when a lane has LOADED the last block of a chunk it drops the chunk's reference on its page(s); the lane that
//     brings a page to zero reports it to the host through a FIFO in mapped pinned memory — the page can take new
//     bytes while the consumer wave is still compressing the chunk's last blocks;
//   * the consumer writes the digest straight into the host-visible record cell and raises the cell's flag.
// (RingCtl / RingSource: kernels.h; the queue protocol shared with the cut side: ring_queue.h)

// the services' regime probe (RingSource::probe): called once per block step by the service's probe wave, wave-uniform
struct RingProbe {
    uint32_t n = 0, idle = 0, act = 0;
    unsigned long long c0 = 0, w0 = 0;
};
// (`active`: lanes of the probe wave that carried a block in this step -> probe[8] for the pair service: how full its lanes are,
// pbsgpu_ring_debug)
__device__ __forceinline__ void ring_probe_step(const RingSource &src, RingProbe &pb, const bool busy, const int slot, const int lane,
                                                const uint32_t active = 0) {
    pb.idle |= busy ? 0u : 1u;
    pb.act += active;
    if (++pb.n < kRingProbeSteps) return;
    const unsigned long long c = clock64(), w = wall_clock64();
    if (!pb.idle && pb.w0 != 0ull && lane == 0 && src.probe) {
        atomicAdd(src.probe + slot, (unsigned long long)kRingProbeSteps);
        atomicAdd(src.probe + slot + 1, c - pb.c0);
        atomicAdd(src.probe + slot + 2, w - pb.w0);
        if (slot == 0) atomicAdd(src.probe + 8, (unsigned long long)pb.act);
    }
    pb.n = 0;
    pb.act = 0;
    pb.idle = 0;
    pb.c0 = c;
    pb.w0 = w;
}

// Each lane streams one byte range through SHA-256. Per loop trip every busy lane consumes
// one 64-byte block: the raw dwords of the NEXT block are requested before the current
// block is compressed, so the HBM/L2 latency of a lane's private stream hides behind the
// ~1700 VALU ops of the compression even with a single wave on the SIMD.
template <typename Source>
__global__ __launch_bounds__(64) void k_sha256(Source src, const uint32_t *nitems_p, uint32_t nitems_imm,
                                               uint32_t *queue, const uint32_t *wg_limit, uint32_t whole_chip) {
    // k_order's budget counts 128-lane workgroups of the pair kernel = two of these waves; waves beyond it leave
    // their SIMD slot to the other batches in flight (the queue is dynamic, the remaining waves drain it).
    // whole_chip (dense launches): every wave works unless k_order said "skip this pass" (0)
    if (wg_limit) {
        const uint32_t lim = *wg_limit;
        if (whole_chip ? lim == 0 : blockIdx.x >= lim * 2u) return;
    }
    const int lane = threadIdx.x & 63;
    const uint32_t nitems = nitems_p ? *nitems_p : nitems_imm;

    // "next" block descriptor (what R holds / will hold)
    const uint8_t *base = nullptr;  // start of the lane's byte range
    uint64_t len = 0;               // its length
    uint64_t blk = 0, nblk = 0;     // index of the block in R, total blocks incl. padding
    uint8_t *dst = nullptr;
    bool have = false;              // R holds a valid block
    bool exhausted = false;         // queue is empty for this lane

    uint32_t R[17];                 // raw little-endian dwords of the next block (+1 for misalignment)
    uint32_t sel = 0x00010203u;     // v_perm selector: byte swap + misalignment shift
#pragma unroll
    for (int j = 0; j < 17; ++j) R[j] = 0;

    uint32_t H[8];
    sha256_iv(H);

    // loads block `blk` of (base,len) into R (raw) and sets sel
    // (`key`: empty for a plain source, the key's words for a keyed one. An argument, not `src.key`: with `src` named inside
    // this lambda, even in a branch an instance discards, the plain instances compiled to ISA with a few instructions and
    // registers swapped; with the argument pack their ISA text is what it was, byte for byte — DESIGN.md §23)
    auto load_block = [&](auto... key) {
        const uint64_t off = blk * 64;
        if (off + 64 <= len) {  // pure data block: aligned dword loads + per-lane funnel selector
            const uint8_t *p = base + off;
            const uint32_t o = (uint32_t)((uintptr_t)p & 3u);
            const gvec4_ptr q = (gvec4_ptr)(p - o);
            const u32x4_a4 v0 = q[0], v1 = q[1], v2 = q[2], v3 = q[3];
            R[0] = v0.x; R[1] = v0.y; R[2] = v0.z; R[3] = v0.w;
            R[4] = v1.x; R[5] = v1.y; R[6] = v1.z; R[7] = v1.w;
            R[8] = v2.x; R[9] = v2.y; R[10] = v2.z; R[11] = v2.w;
            R[12] = v3.x; R[13] = v3.y; R[14] = v3.z; R[15] = v3.w;
            R[16] = o ? ((gword_ptr)(p - o))[16] : 0u;
            sel = ((o) << 24) | ((o + 1) << 16) | ((o + 2) << 8) | (o + 3);
        } else {  // tail / padding block (at most two per range)
            if constexpr (sizeof...(key) != 0) sha256_tail_words_keyed(base, len, off, blk + 1 == nblk, key..., R);
            else sha256_tail_words(base, len, off, blk + 1 == nblk, R);
            sel = 0x00010203u;
        }
    };

    // acquire a new range for lanes that need one
    auto acquire = [&](bool need) {
        const unsigned long long m = __ballot(need);
        if (m == 0) return;
        const uint32_t first = wave_claim(queue, m, (uint32_t)__popcll(m), lane);
        if (need) {
            const uint32_t i = first + wave_rank(m, lane);
            if (i < nitems) {
                src.get(i, base, len, dst);
                blk = 0;
                if constexpr (SuffixOf<Source>::kBytes != 0) nblk = pbss::sha256_blocks(len, SuffixOf<Source>::kBytes);
                else nblk = (len + 8) / 64 + 1;
                have = true;
            } else {
                exhausted = true;
                have = false;
            }
        }
    };

    acquire(true);
    if (have) {
        if constexpr (SuffixOf<Source>::kBytes != 0) load_block(src.key);
        else load_block();
    }

    while (__any(have)) {
        // current block = R; convert to big-endian message words
        uint32_t W[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) W[j] = __builtin_amdgcn_perm(R[j + 1], R[j], sel);
        const bool cur = have;
        const bool cur_last = have && (blk + 1 == nblk);
        uint8_t *cur_dst = dst;

        // advance to the next block / next range and request its bytes
        if (have) {
            if (!cur_last) ++blk; else have = false;
        }
        acquire(!have && !exhausted);
        if (have) {
            if constexpr (SuffixOf<Source>::kBytes != 0) load_block(src.key);
            else load_block();
        }

        if (cur) sha256_compress(H, W);

        if (cur_last) {
            uint32_t *o = reinterpret_cast<uint32_t *>(cur_dst);  // digest is 4-byte aligned in both sources
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = __builtin_bswap32(H[j]);
            sha256_iv(H);
        }
    }
}

// -------------------------------------------------------------------------------------
// SHA-256, LANES service of the page ring (RingSource::sdesc): the single-wave form above on the ring's protocol. One lane per
// chunk, schedule and rounds in the same wave, no LDS hand-over and no barrier: four independent waves per CU (the launch takes
// the CU's whole LDS like the other services). 81 chain-blocks per us and CU against the pair form's 74 — and 3.2 us per block for
// every chain, which is why only SHORT chunks come here and only while this service has room (k_ring_control). The queue is a
// compare-and-swap queue like the long one: a lane never claims a position it then has to wait at.
__global__ __launch_bounds__(512) void k_sha256_lanes(RingSource src) {
    const int lane = threadIdx.x & 63;
    const uint8_t *base = nullptr, *base2 = nullptr;
    uint64_t len = 0, blk = 0, nblk = 0;
    uint32_t len1 = 0, pages = 0xffffffffu, poll_ctr = 0;
    uint8_t *dst = nullptr;
    bool have = false, exhausted = false;
    uint32_t R[17];
    uint32_t sel = 0x00010203u;
#pragma unroll
    for (int j = 0; j < 17; ++j) R[j] = 0;
    uint32_t H[8];
    sha256_iv(H);

    auto load_block = [&]() {  // request block `blk` of the lane's chunk (k_sha256_pair's prep)
        const uint64_t off = blk * 64;
        const uint8_t *bb = (off < len1) ? base : base2;  // which physical page holds this block
        if (off + 64 <= len) {
            sha256_request_block(bb + off, R, sel);
        } else {
            sha256_tail_words(bb, len, off, blk + 1 == nblk, R);
            sel = 0x00010203u;
        }
    };
    auto acquire = [&](bool need) {
        if (__ballot(need) == 0) return;
        if (__ballot(have) != 0 && ((++poll_ctr) & src.poll_mask) != 0u) return;
        uint32_t sh;
        const int32_t avail = ring_queue_avail(&src.ctl->sq, sh);
        const unsigned long long mn = __ballot(need);
        if (avail > 0) {
            const uint32_t cnt = min((uint32_t)__popcll(mn), (uint32_t)avail);
            const uint32_t first = ring_cas_claim(&src.ctl->shead, sh, cnt, mn, lane);
            if (first != 0xffffffffu) {
                const uint32_t rank = wave_rank(mn, lane);
                const bool got = need && rank < cnt;
                uint4 e0, e1;
                ring_desc_load(src.sdesc, (first + rank) & src.smask, got, e0, e1);
                ring_desc_take(src, got, e0, e1, base, base2, len, len1, dst, pages);
                blk = got ? 0ull : blk;
                nblk = got ? ((uint64_t)e0.z + 8u) / 64u + 1u : nblk;
                have = have | got;
            }
        } else if (ring_stop_raised(src) && ring_drained_after_stop(&src.ctl->sq)) {
            exhausted = exhausted | need;
        }
    };

    // regime probe of this service (pbsgpu_ring_debug): workgroup 0's first wave, steps and 100 MHz ticks of the intervals in which
    // it carried a block in every step -> probe[6], probe[7]
    const bool probe_on = src.probe != nullptr && blockIdx.x == 0 && threadIdx.x < 64;
    uint32_t pn = 0, pidle = 0, pact = 0;
    unsigned long long pw0 = 0;
    acquire(true);
    if (have) load_block();
    for (;;) {
        if (probe_on) {
            const unsigned long long hm = __ballot(have);
            pidle |= hm ? 0u : 1u;
            pact += (uint32_t)__popcll(hm);
            if (++pn >= kRingProbeSteps) {
                const unsigned long long w = wall_clock64();
                if (!pidle && pw0 != 0ull && lane == 0) {
                    atomicAdd(src.probe + 6, (unsigned long long)kRingProbeSteps);
                    atomicAdd(src.probe + 7, w - pw0);
                    atomicAdd(src.probe + 9, (unsigned long long)pact);
                }
                pn = 0; pidle = 0; pact = 0; pw0 = w;
            }
        }
        if (!__any(have)) {  // the wave holds nothing: leave once every lane has seen `stop` with the queue empty, else nap and look again
            if (__ballot(!exhausted) == 0ull) break;
            __builtin_amdgcn_s_sleep(48);
            poll_ctr = 0;
            acquire(!exhausted);
            if (have) load_block();
            continue;
        }
        uint32_t W[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) W[j] = __builtin_amdgcn_perm(R[j + 1], R[j], sel);
        const bool cur = have;
        const bool cur_last = have && (blk + 1 == nblk);
        uint8_t *cur_dst = dst;
        if (have) {
            if (!cur_last) ++blk; else have = false;
        }
        if (cur_last) ring_release_pages(src, pages);  // the chunk's last block is in registers
        acquire(!have && !exhausted);
        if (have) load_block();
        if (cur) sha256_compress(H, W);
        if (cur_last) {  // record cell in mapped pinned memory: digest first, then its flag
            PBSK_GLOBAL uint32_t *o = (PBSK_GLOBAL uint32_t *)cur_dst;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = __builtin_bswap32(H[j]);
            ring_cell_publish(o);
            sha256_iv(H);
        }
    }
}

// -------------------------------------------------------------------------------------
// SHA-256, wave-pair form. The ingest workload is parallelism-starved on this chip: at a
// 4 MiB average chunk even a full 288 GB of HBM holds ~70 k chunks, while 256 CUs x 4 SIMDs
// x 2 waves offer 131 k lanes, and a lone wave only issues one instruction every ~4 cycles.
// A batch therefore finishes when its LONGEST chunk does (max = 16 MiB = 262 144 dependent
// compressions), so what matters is the number of instructions on that serial chain. A
// workgroup is two waves on two SIMDs: the PRODUCER wave owns the byte streams (queue,
// loads, tail/padding, byte swap, message schedule, + K) and hands W[t]+K[t] through LDS;
// the CONSUMER wave executes nothing but the 64 rounds (14 VALU each) and the digest store.
// One s_barrier per block; LDS double-buffered (2 x 16 KiB).
// DENSE form (second instantiation, chosen per launch by the host: sha256_dense_pays): when a job holds more work than
// the two pairs can finish within its longest chain, the chain no longer bounds the job — issue slots do, and a pair
// leaves them unused: the producers' SIMDs idle part of every step. The workgroup is then EIGHT waves (4 pairs):
// waves 4,5 = producers of pairs 2,3 (they land on the SIMDs of consumers 0,1), waves 6,7 = consumers of pairs 2,3
// (on the SIMDs of producers 0,1; placement verified with HW_ID, profiles/r02_probe_simd_placement.log), so every SIMD
// hosts one consumer and one producer. The gain is bounded by the instruction counts: per block the consumer issues
// ~935 instructions and the producer ~860 (744 VALU: 48 x 11 schedule + K adds + perms + addressing), so four pairs
// per ~1800 issue slots against two pairs per ~935 is +7 % at best; measured +5 % (SHA alone 65.3 -> 62.0 ms for
// 64 GiB at 64 KiB average). Each chain is ~1.9x slower in this form, so it is used only when the chain does not bound.
template <typename Source, bool DENSE>
__global__ __launch_bounds__(DENSE ? 512 : 256) void k_sha256_pair(Source src, const uint32_t *nitems_p, uint32_t nitems_imm,
                                                                   uint32_t *queue, const uint32_t *wg_limit) {
    // The HOST picks the form per launch (sha256_dense_pays: from the batch's byte count and the chunker's maximum —
    // k_order could decide more exactly on the device, but then both forms have to be enqueued and the idle one still
    // waits for CUs with room for its LDS before it can leave: measured 2.7 ms avg / 14 ms max per batch on the default
    // workload, 46 ms at 64 KiB average). Two instantiations rather than a run-time switch: launch bounds and LDS
    // differ, and the sparse code stays exactly what was tuned (one 512-thread kernel with a switch ran the sparse chain
    // at 463-465 ms per 64 GiB against 433-458; within box-to-box spread). Sparse: workgroups beyond
    // k_order's budget leave at once so their CUs can host another batch's kernel; dense: the budget is the whole
    // chip, only k_order's "skip this pass" (0) is honoured.
    if (wg_limit) {
        const uint32_t lim = *wg_limit;
        if (DENSE ? lim == 0 : blockIdx.x >= lim) return;
    }
    // One workgroup per CU (sparse: 69 KB static LDS + the launch's padding; dense: 137 KB).
    // waves 0,1 = consumers of pair 0,1; waves 2,3 = their producers;
    // dense only: waves 4,5 = producers of pair 2,3; waves 6,7 = their consumers.
    constexpr int NP = DENSE ? 4 : 2;
    __shared__ uint4 wkbuf_[NP][2][16][64];  // [pair][buffer][4 rounds][lane] -> 16 B per lane, contiguous rows
    __shared__ uint32_t ctrl_[NP][2][64];    // bit0 block valid, bit1 last block of its range
    __shared__ uint8_t *dstp_[NP][2][64];    // digest destination (valid when bit1)
    __shared__ uint32_t alive[NP][2];        // [pair][buffer]: producer still had blocks
    __shared__ uint32_t curw[NP][2];         // [pair][buffer]: the pair had a block in this step (ring service: who may nap)
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int pr = (wave & 1) | (wave >= 4 ? 2 : 0);
    const bool producer = (wave >= 2 && wave < 6);
    auto &wkbuf = wkbuf_[pr];
    auto &ctrl = ctrl_[pr];
    auto &dstp = dstp_[pr];
    auto any_alive = [&](const int pb) -> uint32_t {
        uint32_t a = alive[0][pb] | alive[1][pb];
        if constexpr (DENSE) a |= alive[2][pb] | alive[3][pb];
        return a;
    };

    if (producer) {
        const uint32_t nitems = nitems_p ? *nitems_p : nitems_imm;
        // byte-stream state of this lane
        const uint8_t *base = nullptr;
        uint64_t len = 0, blk = 0, nblk = 0;  // blk = next block to fetch
        uint8_t *dst = nullptr;
        bool have = false, exhausted = false;
        // ring service only: second piece of a chunk that crosses into another physical page (virtual base: the byte at
        // chunk offset `off >= len1` lives at base2 + off), the chunk's page references, the lane's claimed queue position
        [[maybe_unused]] const uint8_t *base2 = nullptr;
        [[maybe_unused]] uint32_t len1 = 0, pages = 0xffffffffu, claim = 0;
        [[maybe_unused]] uint32_t claimed = 0;  // (a word, not a bool: two bool flags set in sibling branches get their stores
                                                // merged through a selected pointer by the optimiser, which puts both in scratch)
        [[maybe_unused]] unsigned long long idle_since = 0;
        [[maybe_unused]] uint32_t hb_seen = 0;
        // FIFO of raw blocks in flight: a block is requested D iterations before it is expanded, so
        // HBM/TLB latency of the lane-private streams stays off the serial chain
        // (round 6: D = 4 in the ring's service — is it memory latency that makes the producer the slower half under load, 1.92-1.95
        // against 1.81-1.82 us per step? No: 604-612 GiB/s against 618-619 on the same box, profiles/r06_ab_restored_services_and_fifo_depth.log)
        constexpr int D = 2;  // even (buffer parity is derived from the slot index)
        uint32_t R[D][17];
        uint32_t selv[D], cflag[D];
        uint8_t *dstv[D];
        [[maybe_unused]] uint32_t pagesv[D];
#pragma unroll
        for (int s = 0; s < D; ++s) {
#pragma unroll
            for (int j = 0; j < 17; ++j) R[s][j] = 0;
            selv[s] = 0x00010203u;
            cflag[s] = 0;
            dstv[s] = nullptr;
            pagesv[s] = 0xffffffffu;
        }

        // Dense form: a wave RESERVES kReserve extra queue positions with every atomic and serves its lanes from that
        // reserve, so most chunk boundaries cost no atomic round trip at all (items >> lanes there; a few positions held
        // back by a wave at the very end are handed to its own lanes). The sparse form must not hoard — it has more
        // lanes than chunks, and the longest-first order is what keeps its makespan at the longest chain.
        constexpr uint32_t kReserve = 16;
        uint32_t res_next = 0, res_end = 0;  // the wave's reserved positions [res_next, res_end): same value in every lane
        [[maybe_unused]] uint32_t poll_ctr = 0;
        auto acquire = [&](bool need) {
            if constexpr (Source::kRing) {
                // Lanes without work look at the queue — a device-scope load the wave then WAITS for (0.3-0.5 us: about the
                // slack the producer has against its consumer). With every step of a wave that still carries chunks on its
                // other lanes this made the PRODUCER the slower half of the pair whenever one lane was idle: the chain of a
                // max-size chunk ran at ~1.95 us per block instead of 1.7 in a draining ring (drain floor 0.515 s, one file
                // alone 0.58 s) and in every wave with a starved lane during the feed phase. A wave with work therefore
                // polls on every 8th step only (src.poll_mask, PBSGPU_RING_POLL_EVERY; a free lane waits <= 14 us for its next
                // chunk: 0.02 % of a 4 MiB chunk's chain); a wave with no work at all polls every step, as before.
                if (__ballot(need) == 0) return;
                if (__ballot(have) != 0 && ((++poll_ctr) & src.poll_mask) != 0u) return;
                // (0) LONG chunks first (see RingSource::ldesc; a CAS queue: ring_cas_claim)
                // Who may take a long chunk: a lane that holds NO claim on the main queue — one that has just finished a
                // chunk, or one of the few lanes (1 in 16) that never claim there. A lane that waits at a claimed, not yet
                // published position must not: the chunk published at its position later would then wait for the whole
                // long chain (measured: +0.26-0.40 s on a single file when every idle lane could take long chunks).
                const bool long_only = src.long_bytes != 0u && src.xp == 0u && (lane & 15) == 0;
                const bool elig = need && claimed == 0u;
                if (src.long_bytes && __ballot(elig)) {
                    uint32_t lh;
                    // (spill: what the express service's lanes are left)
                    int32_t avail = ring_queue_avail(&src.ctl->lq, lh) - (int32_t)src.long_spill;
                    // with an express service: only while ALL its lane pairs are busy — a long chunk that waited for one would
                    // finish later than on a pair lane that is free now (configs[2]: half the bytes are 16 MiB chunks)
                    // (safety valve: more long chunks waiting than the express service has pairs — e.g. its workgroups have not
                    // found their CUs yet — are everybody's business)
                    if (avail > 0 && src.xp != 0u && (uint32_t)avail <= src.xp_pairs &&
                        __hip_atomic_load(&src.ctl->xp_busy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < src.xp_pairs)
                        avail = 0;
                    if (avail > 0) {
                        const unsigned long long mn = __ballot(elig);
                        const uint32_t cnt = min((uint32_t)__popcll(mn), (uint32_t)avail);
                        const uint32_t first = ring_cas_claim(&src.ctl->lhead, lh, cnt, mn, lane);
                        if (first != 0xffffffffu) {
                            const uint32_t rank = wave_rank(mn, lane);
                            const bool tk = elig && rank < cnt;
                            uint4 e0, e1;
                            ring_desc_load(src.ldesc, (first + rank) & src.lmask, tk, e0, e1);
                            ring_desc_take(src, tk, e0, e1, base, base2, len, len1, dst, pages);
                            blk = tk ? 0ull : blk;
                            nblk = tk ? ((uint64_t)e0.z + 8u) / 64u + 1u : nblk;
                            have = have | tk;
                            need = need && !tk;
                        }
                    }
                }
                // (1) lanes without a position claim one: ONE atomic per wave
                const bool want = need && !claimed && !long_only;
                const unsigned long long mw = __ballot(want);
                if (mw) {
                    uint32_t first = 0;
                    const int leader = __ffsll((long long)mw) - 1;
                    if (lane == leader) {
                        const uint32_t cnt = (uint32_t)__popcll(mw);
                        first = atomicAdd(&src.ctl->head, cnt);
                        // claim progress for the host's backlog gate (ring.cpp): one posted write to mapped pinned
                        // memory whenever the head crosses a multiple of 256
                        if (((first + cnt) ^ first) >> 8)
                            __hip_atomic_store(const_cast<uint32_t *>(src.heartbeat) + 32, first + cnt, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_SYSTEM);
                    }
                    first = __shfl(first, leader, 64);
                    if (want) {
                        claim = first + wave_rank(mw, lane);
                        claimed = 1u;
                    }
                }
                // (2) has the queue reached the lane's position? {tail, stop} in one relaxed load; the acquire fence only
                // when some lane takes a descriptor
                if (__ballot(need) == 0) return;
                const unsigned long long ts = __hip_atomic_load(&src.ctl->tail_stop,
                                                                __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t tail = (uint32_t)ts, stop = (uint32_t)(ts >> 32);
                const bool ready = need && claimed != 0u && (int32_t)(tail - claim) > 0;
                if (__ballot(ready)) __atomic_thread_fence(__ATOMIC_ACQUIRE);
                uint4 d0, d1;
                ring_desc_load(src.desc, claim & src.qmask, ready, d0, d1);
                // size 0 = a void position (the open chunk of a round): the lane takes another one next time
                const bool got = ready && d0.z != 0u;
                claimed = ready ? 0u : claimed;
                ring_desc_take(src, got, d0, d1, base, base2, len, len1, dst, pages);
                blk = got ? 0ull : blk;
                nblk = got ? ((uint64_t)d0.z + 8u) / 64u + 1u : nblk;
                have = have | got;
                // stop: nothing will ever be published at this position (without an express service the long queue is
                // this service's too: looked at once more)
                bool leave = need && !ready && stop != 0u;
                if (src.long_bytes && src.xp == 0u && __ballot(leave) && !ring_drained_after_stop(&src.ctl->lq)) leave = false;
                exhausted = exhausted | leave;
                return;
            }
            const unsigned long long m = __ballot(need);
            if (m == 0) return;
            uint32_t first = 0;
            uint32_t avail = 0;
            if constexpr (DENSE) {
                const uint32_t cnt = (uint32_t)__popcll(m);
                avail = res_end - res_next;
                if (cnt > avail) first = wave_claim(queue, m, cnt - avail + kReserve, lane);
            } else {
                first = wave_claim(queue, m, (uint32_t)__popcll(m), lane);
            }
            if (need) {
                uint32_t i = first + wave_rank(m, lane);
                if constexpr (DENSE) {
                    const uint32_t r = wave_rank(m, lane);
                    i = r < avail ? res_next + r : first + (r - avail);
                }
                if (i < nitems) {
                    if constexpr (!Source::kRing) src.get(i, base, len, dst);
                    blk = 0;
                    if constexpr (SuffixOf<Source>::kBytes != 0) nblk = pbss::sha256_blocks(len, SuffixOf<Source>::kBytes);
                    else nblk = (len + 8) / 64 + 1;
                    have = true;
                } else {
                    exhausted = true;
                    have = false;
                }
            }
            if constexpr (DENSE) {
                const uint32_t cnt = (uint32_t)__popcll(m);
                if (cnt > avail) {
                    res_next = first + (cnt - avail);
                    res_end = res_next + kReserve;
                } else {
                    res_next += cnt;
                }
            }
        };
        // request the lane's next block into FIFO slot s (compile-time s); `key`: as for k_sha256's load_block
        auto prep = [&](const int s, auto... key) {
            acquire(!have && !exhausted);
            uint32_t c = 0;
            const uint8_t *p = reinterpret_cast<const uint8_t *>(kIdleBlock);
            const uint8_t *bb = base;
            uint64_t off = 0;
            bool tail = false, last = false;
            if (have) {
                off = blk * 64;
                if constexpr (Source::kRing) bb = (off < len1) ? base : base2;  // which physical page holds this block
                last = blk + 1 == nblk;
                if (off + 64 <= len) p = bb + off;  // pure data block: 4-byte aligned vector loads + funnel selector
                else tail = true;                   // tail / padding block (<= 2 per range)
                c = 1u | (last ? 2u : 0u);
                dstv[s] = dst;
                if constexpr (Source::kRing) pagesv[s] = pages;
                if (++blk == nblk) have = false;
            }
            sha256_request_block(p, R[s], selv[s]);
            if (tail) {
                if constexpr (sizeof...(key) != 0) sha256_tail_words_keyed(bb, len, off, last, key..., R[s]);
                else sha256_tail_words(bb, len, off, last, R[s]);
                selv[s] = 0x00010203u;
            }
            cflag[s] = c;
        };

#pragma unroll
        for (int s = 0; s < D; ++s) {
            if constexpr (SuffixOf<Source>::kBytes != 0) prep(s, src.key);
            else prep(s);
        }
        // ONE exit, behind the last slot's step. Every path from a slot's requests back to the perm that consumes them then
        // passes the other slot's five requests, and the slot is awaited with vmcnt(5). (An exit in the middle — a test of
        // `running` per slot, or a return — is routed through the loop's latch by the structuriser: an edge from slot 0's
        // barrier to the loop's head on which nothing follows slot 0's requests, and the wait at the head is vmcnt(0).)
        // If the pairs drain at slot 0's barrier, slot 1's step is one empty step whose barrier only the producer waves
        // still reach: the consumers have ended, and s_barrier waits for the surviving waves of a workgroup only.
        bool drained = false;
        [[maybe_unused]] bool wg_busy = false;  // some pair of this workgroup had a block in the previous step
        [[maybe_unused]] RingProbe probe;
        [[maybe_unused]] const bool probe_on = blockIdx.x == 0 && wave == 2;
        while (!drained) {
#pragma unroll
            for (int s = 0; s < D; ++s) {
                {
                    constexpr int kBufMask = 1;
                    const int pb = s & kBufMask;  // D is even: buffer parity is static
                    uint32_t W[16];
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        W[j] = __builtin_amdgcn_perm(R[s][j + 1], R[s][j], selv[s]);
                        // pinned HERE (an empty volatile statement is neither sunk into the `any_cur` branch below nor
                        // moved behind prep(s)): the slot's registers must be dead before its refill is requested, or
                        // the refill lands in a second register set that is copied back at the loop's end behind an
                        // s_waitcnt vmcnt(0) — every block would again be awaited in the step that requested it
                        asm volatile("" : "+v"(W[j]));
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    const uint32_t c = cflag[s];
                    uint8_t *cur_dst = dstv[s];
                    if constexpr (Source::kRing) {
                        // The chunk's LAST block has arrived in registers: nothing of the chunk will be read from HBM
                        // again, its pages may go back to the host at once.
                        // (Round 4 tried letting go of a two-page chunk's FIRST page as soon as its last block there was
                        // in: no gain — a max-size chunk lives almost entirely in ONE 16.2 MiB page, which it holds for
                        // its whole 0.46 s either way; configs[2] through the ring 412 vs 422 GiB/s. Removed again.)
                        if (c & 2u) ring_release_pages(src, pagesv[s]);
                    }
                    // refill the slot: the block D iterations ahead
                    if constexpr (SuffixOf<Source>::kBytes != 0) prep(s, src.key);
                    else prep(s);
                    const bool any_cur = __any(c & 1u);
                    if (any_cur) {
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            uint32_t x[4];
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const int t = 4 * q + j;
                                x[j] = ((t < 16) ? W[t] : sha256_sched(W, t)) + kSha256K[t];
                            }
                            wkbuf[pb][q][lane] = make_uint4(x[0], x[1], x[2], x[3]);
                        }
                    }
                    ctrl[pb][lane] = c;
                    dstp[pb][lane] = cur_dst;
                    bool live = any_cur;
                    if constexpr (Source::kRing) {
                        // a service wave stays until `stop` has reached every lane and its block FIFO has drained; with
                        // nothing to do it naps instead of spinning through barriers.
                        // A host that died, or sits in a blocking read for longer than idle_ticks, must not leave a kernel
                        // behind that never ends: the DESIGNATED wave (workgroup 0, first producer) then stops the service on
                        // its own. That must never lose a chunk, i.e. no round may publish positions behind lanes that have
                        // left. Handshake (Dekker, through mapped pinned memory): the wave announces its intent, THEN re-reads
                        // the heartbeat and the host's count of enqueued rounds; the host bumps heartbeat and count FIRST and
                        // THEN looks at the intent flag before it enqueues a round (ring.cpp, ring_service_gate). Either the
                        // wave sees the host and withdraws, or the host sees the intent and waits for the outcome. The stop
                        // is committed only if every enqueued round has been published (rounds_done) — published positions
                        // are always served: a lane leaves only at a position the tail has not reached.
                        const bool wave_done = __ballot(!exhausted) == 0ull;
                        live = any_cur || !wave_done;
                        if (!any_cur && !wave_done) {
                            const unsigned long long now = wall_clock64();
                            if (idle_since == 0) idle_since = now;
                            if (blockIdx.x == 0 && wave == 2 && now - idle_since > src.idle_ticks) {
                                // (the heartbeat lives in HOST memory: it is read once per timeout, not per idle iteration —
                                // hundreds of idle waves polling it over PCIe every few microseconds slowed the ring down 6x)
                                uint32_t *hbw = const_cast<uint32_t *>(src.heartbeat);
                                const uint32_t hb = __hip_atomic_load(hbw + kHbBeat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                                if (hb != hb_seen) {  // alive: it just has nothing for us yet
                                    hb_seen = hb;
                                    idle_since = now;
                                } else {
                                    if (lane == 0) __hip_atomic_store(hbw + kHbIntent, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                                    __atomic_thread_fence(__ATOMIC_SEQ_CST);  // system scope: the intent is out before the re-reads
                                    __threadfence_system();
                                    const uint32_t hb2 = __hip_atomic_load(hbw + kHbBeat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                                    const uint32_t enq = __hip_atomic_load(hbw + kHbRoundsEnq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                                    const uint32_t done = __hip_atomic_load(&src.ctl->rounds_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                    if (hb2 != hb || enq != done) {  // the host is back, or a round is still on its way: withdraw
                                        if (lane == 0) __hip_atomic_store(hbw + kHbIntent, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                                        hb_seen = hb2;
                                        idle_since = now;
                                    } else if (lane == 0) {  // commit: every lane leaves at its next look at {tail, stop}
                                        __hip_atomic_store(&src.ctl->stop, 2u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                                        __hip_atomic_store(hbw + kHbCommitted, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                                    }
                                }
                            }
                            // (nap only while the WHOLE workgroup is idle: the pairs of a workgroup share the block barrier, and
                            // an idle pair that slept 1.3 us per step held its working sibling at 1.9 us per block instead of 1.7
                            // — the chain of every chunk in a draining ring, of every chunk of a lone file)
                            if (!wg_busy) __builtin_amdgcn_s_sleep(48);
                        } else {
                            idle_since = 0;
                        }
                        if (lane == 0) curw[pr][pb] = any_cur ? 1u : 0u;
                        if (probe_on) ring_probe_step(src, probe, any_cur, 0, lane, (uint32_t)__popcll(__ballot(c & 1u)));
                    }
                    if (lane == 0) alive[pr][pb] = live ? 1u : 0u;
                    __syncthreads();
                    drained = drained || __builtin_amdgcn_readfirstlane(any_alive(pb)) == 0u;  // every pair drained
                    if constexpr (Source::kRing) {
                        uint32_t w = curw[0][pb] | curw[1][pb];
                        if constexpr (DENSE) w |= curw[2][pb] | curw[3][pb];
                        wg_busy = w != 0u;
                    }
                }
            }
        }
    } else {
        // CONSUMER: software-pipelined over blocks. After barrier k+1 (producer has published block k+1) it
        // first issues the LDS reads of block k+1 into the OTHER register set and only then runs the 64 rounds
        // of block k from registers, so LDS latency and barrier skew hide behind ~3700 cycles of rounds. The
        // early copy to registers is also what keeps two LDS buffers sufficient.
        uint32_t H[8];
        sha256_iv(H);
        struct Blk {
            uint32_t al, c;
            uint8_t *d;
            uint4 wk[16];
        };
        auto fetch = [&](Blk &x, const int pb) {
            x.al = any_alive(pb);
            x.c = ctrl[pb][lane];
            x.d = dstp[pb][lane];
#pragma unroll
            for (int q = 0; q < 16; ++q) x.wk[q] = wkbuf[pb][q][lane];
        };
        auto rounds = [&](const Blk &x) {
            if (x.c & 1u) {
                uint32_t a = H[0], b = H[1], cc = H[2], dd = H[3], e = H[4], f = H[5], g = H[6], h = H[7];
#pragma unroll
                for (int q = 0; q < 16; q += 2) {
                    SHA256_ROUND(a, b, cc, dd, e, f, g, h, x.wk[q].x);
                    SHA256_ROUND(h, a, b, cc, dd, e, f, g, x.wk[q].y);
                    SHA256_ROUND(g, h, a, b, cc, dd, e, f, x.wk[q].z);
                    SHA256_ROUND(f, g, h, a, b, cc, dd, e, x.wk[q].w);
                    SHA256_ROUND(e, f, g, h, a, b, cc, dd, x.wk[q + 1].x);
                    SHA256_ROUND(dd, e, f, g, h, a, b, cc, x.wk[q + 1].y);
                    SHA256_ROUND(cc, dd, e, f, g, h, a, b, x.wk[q + 1].z);
                    SHA256_ROUND(b, cc, dd, e, f, g, h, a, x.wk[q + 1].w);
                }
                H[0] += a; H[1] += b; H[2] += cc; H[3] += dd; H[4] += e; H[5] += f; H[6] += g; H[7] += h;
                if (x.c & 2u) {
                    // (a GLOBAL pointer as well: one flat_store anywhere in the kernel — the two roles share one function — leaves
                    // a "flat access may be pending" state on the paths into the producer's loop, and with it every wait
                    // for a block slot becomes vmcnt(0) lgkmcnt(0))
                    PBSK_GLOBAL uint32_t *o = (PBSK_GLOBAL uint32_t *)x.d;
#pragma unroll
                    for (int j = 0; j < 8; ++j) o[j] = __builtin_bswap32(H[j]);
                    if constexpr (Source::kRing) ring_cell_publish(o);  // record cell in mapped pinned memory: digest, then flag
                    sha256_iv(H);
                }
            }
        };
        Blk A, B;
        __syncthreads();  // barrier 0: block 0 is published
        fetch(A, 0);
        for (;;) {
            if (!A.al) break;          // block k is the drained marker: the producers have left after its barrier
            __syncthreads();           // barrier k+1
            fetch(B, 1);
            __builtin_amdgcn_sched_barrier(0);
            rounds(A);
            if (!B.al) break;
            __syncthreads();           // barrier k+2
            fetch(A, 0);
            __builtin_amdgcn_sched_barrier(0);
            rounds(B);
        }
    }
}

// -------------------------------------------------------------------------------------
// SHA-256, EXPRESS form: TWO LANES PER CHUNK, on top of the wave pair. Rounds 1-3 called the chain of a max-size chunk a
// floor: 64 rounds x 14 instructions, one instruction per ~4.2 cycles per wave whatever its lane count, and two WAVES
// cannot share one chain (an LDS round trip >> the 60 cycles of a round). Two LANES of the same wave can: DPP operands
// move a value to the neighbouring lane inside the instruction that uses it. A round's two halves
//     e' = Sigma1(e) + Ch(e,f,g) + [h + d + K + W]        (needs the a-chain only through d = a three rounds ago)
//     a' = Sigma0(a) + Maj(a,b,c) + [e' - d]               (needs the e-chain only through e')
// are the SAME nine instructions on different operands:
//     lane A (even) keeps e,f,g,h = X0..X3, lane B (odd) keeps a,b,c,d and runs TWO rounds behind A, so that ONE
//     register name serves both directions of the exchange: A reads d = a(r-3) from B's X1, B reads e(r-1) from A's X1;
//     Sigma: three v_alignbit by per-lane shift registers (6,11,25 | 2,13,22) + xor3;
//     Ch | Maj: bfi(X0 ^ (X2 & ROLE), X1, X2) — ROLE = 0 gives Ch(e,f,g), ROLE = ~0 gives bfi(a^c, b, c) = Maj(a,b,c);
//     the bracket: NZ = (X3 ^ ROLE) + C (v_xad_u32: h + [K+W] for A with C = K+W; -d for B with C = 1), then
//     P = partner's X1 + NZ (v_add_u32_dpp quad_perm:[1,0,3,2]); X0' = S + F + P (v_add3).
// 9 instructions per round instead of 14, 66 slot-rounds per block (B's two rounds of lag) + 12 for the per-lane
// selects at the block's ends: ~630 issue slots per block against ~946 — the serial chain of a chunk runs 1.5x faster
// (oracle: the formulation was first checked lane by lane in Python against hashlib, scripts/r4_xpair_sim.py).
// The PRODUCER wave needs no cross-lane work at all: the message schedule does not depend on the state, so its two lanes
// of a chunk expand two CONSECUTIVE blocks at once (lane A block 2m, lane B block 2m+1, each with the ordinary code) and
// a producer step (one barrier) feeds two consumer blocks: plane E and plane O of the LDS buffer, both in the row of lane
// A; the rows of the B lanes hold the constant 1 (C above), written once.
// Cost: a wave carries 32 chunks instead of 64, i.e. 0.74 of the pair form's throughput per CU — the form is for the
// chunks whose chain bounds something (the ring's long-chunk queue, a lone file), not for all of them.
// Four slot-rounds in ONE block of fixed order (36 instructions; the start variant adds the two selects that put b and a
// into B's chain). One block, because (1) the DPP operand of a round (its X1) must have been written at least two
// instructions before the v_add_u32_dpp that reads it and the hazard recogniser does not look into inline assembly: X1 is
// an input of the block or the result of a round at least nine instructions earlier; (2) the compiler pads every boundary
// between two assembly statements with an s_nop, and an s_nop costs a whole issue slot of the lone wave.
#define XP_R(n, x0, x1, x2, x3, kw)                                                     \
    "v_xad_u32 %[nz], " x3 ", %[role], " kw "\n\t"                                      \
    "v_alignbit_b32 %[r1], " x0 ", " x0 ", %[sh1]\n\t"                                  \
    "v_alignbit_b32 %[r2], " x0 ", " x0 ", %[sh2]\n\t"                                  \
    "v_add_u32_dpp %[p], " x1 ", %[nz] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t" \
    "v_alignbit_b32 %[r3], " x0 ", " x0 ", %[sh3]\n\t"                                  \
    "v_bitop3_b32 %[sel], " x0 ", " x2 ", %[role] bitop3:0x78\n\t"                      \
    "v_bitop3_b32 %[sg], %[r1], %[r2], %[r3] bitop3:0x96\n\t"                           \
    "v_bitop3_b32 %[f], %[sel], " x1 ", " x2 " bitop3:0xca\n\t"                         \
    "v_add3_u32 " n ", %[sg], %[f], %[p]\n\t"
#define XP_TEMPS                                                                                                   \
    [nz] "=&v"(nz), [r1] "=&v"(r1), [r2] "=&v"(r2), [r3] "=&v"(r3), [p] "=&v"(p), [sel] "=&v"(sel), [sg] "=&v"(sg), \
        [f] "=&v"(f)
struct XpRole {
    uint32_t sh1, sh2, sh3, role;
};
// rounds r .. r+3 of a block; (x0..x3) in: the chain's last four values, newest first; out: the same after four rounds.
// START: r = 0 — B's results of slot-rounds 0 and 1 are replaced by hb1 (= b) and hb0 (= a): its chain starts two late.
template <bool START>
__device__ __forceinline__ void xp_round4(uint32_t &x0, uint32_t &x1, uint32_t &x2, uint32_t &x3, const uint4 kw, const XpRole &R,
                                          const uint32_t hb1 = 0, const uint32_t hb0 = 0) {
    uint32_t n0, n1, n2, n3, nz, r1, r2, r3, p, sel, sg, f;
    if constexpr (START) {
        asm(XP_R("%[n0]", "%[x0]", "%[x1]", "%[x2]", "%[x3]", "%[k0]")
            "v_bitop3_b32 %[n0], %[role], %[hb1], %[n0] bitop3:0xca\n\t"
            XP_R("%[n1]", "%[n0]", "%[x0]", "%[x1]", "%[x2]", "%[k1]")
            "v_bitop3_b32 %[n1], %[role], %[hb0], %[n1] bitop3:0xca\n\t"
            XP_R("%[n2]", "%[n1]", "%[n0]", "%[x0]", "%[x1]", "%[k2]")
            XP_R("%[n3]", "%[n2]", "%[n1]", "%[n0]", "%[x0]", "%[k3]")
            : [n0] "=&v"(n0), [n1] "=&v"(n1), [n2] "=&v"(n2), [n3] "=&v"(n3), XP_TEMPS
            : [x0] "v"(x0), [x1] "v"(x1), [x2] "v"(x2), [x3] "v"(x3), [k0] "v"(kw.x), [k1] "v"(kw.y), [k2] "v"(kw.z), [k3] "v"(kw.w),
              [sh1] "v"(R.sh1), [sh2] "v"(R.sh2), [sh3] "v"(R.sh3), [role] "v"(R.role), [hb1] "v"(hb1), [hb0] "v"(hb0));
    } else {
        asm(XP_R("%[n0]", "%[x0]", "%[x1]", "%[x2]", "%[x3]", "%[k0]")
            XP_R("%[n1]", "%[n0]", "%[x0]", "%[x1]", "%[x2]", "%[k1]")
            XP_R("%[n2]", "%[n1]", "%[n0]", "%[x0]", "%[x1]", "%[k2]")
            XP_R("%[n3]", "%[n2]", "%[n1]", "%[n0]", "%[x0]", "%[k3]")
            : [n0] "=&v"(n0), [n1] "=&v"(n1), [n2] "=&v"(n2), [n3] "=&v"(n3), XP_TEMPS
            : [x0] "v"(x0), [x1] "v"(x1), [x2] "v"(x2), [x3] "v"(x3), [k0] "v"(kw.x), [k1] "v"(kw.y), [k2] "v"(kw.z), [k3] "v"(kw.w),
              [sh1] "v"(R.sh1), [sh2] "v"(R.sh2), [sh3] "v"(R.sh3), [role] "v"(R.role));
    }
    x0 = n3; x1 = n2; x2 = n1; x3 = n0;
}
// the two slot-rounds behind round 63 (B finishes; A idles): K+W is irrelevant to B (its constant is the row of ones)
__device__ __forceinline__ void xp_round2(uint32_t &x0, uint32_t &x1, uint32_t &x2, uint32_t &x3, const uint32_t kw, const XpRole &R) {
    uint32_t n0, n1, nz, r1, r2, r3, p, sel, sg, f;
    asm(XP_R("%[n0]", "%[x0]", "%[x1]", "%[x2]", "%[x3]", "%[k0]")
        XP_R("%[n1]", "%[n0]", "%[x0]", "%[x1]", "%[x2]", "%[k0]")
        : [n0] "=&v"(n0), [n1] "=&v"(n1), XP_TEMPS
        : [x0] "v"(x0), [x1] "v"(x1), [x2] "v"(x2), [x3] "v"(x3), [k0] "v"(kw), [sh1] "v"(R.sh1), [sh2] "v"(R.sh2), [sh3] "v"(R.sh3),
          [role] "v"(R.role));
    x3 = x1; x2 = x0; x1 = n0; x0 = n1;
}
// role ? b : a, bitwise (ROLE is 0 or ~0 per lane)
__device__ __forceinline__ uint32_t xp_sel(uint32_t role, uint32_t a, uint32_t b) { return __builtin_amdgcn_bitop3_b32(role, b, a, 0xCA); }

template <typename Source>
__global__ __launch_bounds__(256) void k_sha256_xpair(Source src, const uint32_t *nitems_p, uint32_t nitems_imm, uint32_t *queue,
                                                      const uint32_t *wg_limit) {
    if (wg_limit && *wg_limit == 0) return;  // k_order: skip this pass (a scan tile overflowed, the batch is re-run)
    // waves 0,1 = consumers of pair 0,1; waves 2,3 = their producers. 32 chunks per pair: chunk ci = lanes 2ci (A), 2ci+1 (B).
    __shared__ uint4 wkbuf_[2][2][2][16][64];  // [pair][buffer][plane E/O][4 rounds][row]: 128 KiB
    __shared__ uint32_t ctrl_[2][2][2][32];    // [pair][buffer][plane][chunk]: bit0 block valid, bit1 last block of its chunk
    __shared__ uint8_t *dstp_[2][2][2][32];    // digest destination (valid when bit1)
    __shared__ uint32_t alive[2][2];           // [pair][buffer]: producer still had blocks
    __shared__ uint32_t curw[2][2];            // [pair][buffer]: the pair had a block in this step
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int pr = wave & 1;
    const bool producer = wave >= 2;
    const bool roleB = (lane & 1) != 0;
    const int ci = lane >> 1;
    auto &wkbuf = wkbuf_[pr];
    auto &ctrl = ctrl_[pr];
    auto &dstp = dstp_[pr];
    auto any_alive = [&](const int pb) -> uint32_t { return alive[0][pb] | alive[1][pb]; };
    // rows of the B lanes: the constant 1 in every plane of every buffer (never written again)
    for (int i = threadIdx.x; i < 2 * 2 * 2 * 16 * 32; i += 256) {
        const int row = 2 * (i & 31) + 1, q = (i >> 5) & 15, pl = (i >> 9) & 1, pb = (i >> 10) & 1, pp = (i >> 11) & 1;
        wkbuf_[pp][pb][pl][q][row] = make_uint4(1u, 1u, 1u, 1u);
    }
    __syncthreads();

    if (producer) {
        const uint32_t nitems = nitems_p ? *nitems_p : nitems_imm;
        const uint8_t *base = nullptr;
        uint64_t len = 0, blk = 0, nblk = 0;  // blk = the lane's next block (A: even blocks, B: odd blocks)
        uint8_t *dst = nullptr;
        bool have = false, exhausted = false;
        [[maybe_unused]] const uint8_t *base2 = nullptr;
        [[maybe_unused]] uint32_t len1 = 0, pages = 0xffffffffu;
        [[maybe_unused]] unsigned long long idle_since = 0;
        [[maybe_unused]] uint32_t poll_ctr = 0;
        constexpr int D = 2;
        uint32_t R[D][17];
        uint32_t selv[D], cflag[D];
        uint8_t *dstv[D];
        [[maybe_unused]] uint32_t pagesv[D];
#pragma unroll
        for (int s = 0; s < D; ++s) {
#pragma unroll
            for (int j = 0; j < 17; ++j) R[s][j] = 0;
            selv[s] = 0x00010203u;
            cflag[s] = 0;
            dstv[s] = nullptr;
            pagesv[s] = 0xffffffffu;
        }
        // `need`: this A lane's PAIR has issued every block of its chunk and wants the next one (B lanes never ask)
        auto acquire = [&](bool need) {
            if (__ballot(need) == 0) return;
            bool got = false;
            if constexpr (Source::kRing) {
                // the ring's LONG-chunk queue only (RingSource::ldesc)
                if (__ballot(have) != 0 && ((++poll_ctr) & src.poll_mask) != 0u) return;
                uint32_t lh;
                const int32_t avail = ring_queue_avail(&src.ctl->lq, lh);
                const unsigned long long mn = __ballot(need);
                if (avail > 0) {
                    const uint32_t cnt = min((uint32_t)__popcll(mn), (uint32_t)avail);
                    const uint32_t first = ring_cas_claim(&src.ctl->lhead, lh, cnt, mn, lane);
                    if (first != 0xffffffffu) {
                        const uint32_t rank = wave_rank(mn, lane);
                        got = need && rank < cnt;
                        uint4 e0, e1;
                        ring_desc_load(src.ldesc, (first + rank) & src.lmask, got, e0, e1);
                        ring_desc_take(src, got, e0, e1, base, base2, len, len1, dst, pages);
                        // (given back when the chunk's last block is in)
                        if (lane == __ffsll((long long)mn) - 1) atomicAdd(&src.ctl->xp_busy, cnt);
                    }
                } else if (ring_stop_raised(src) && ring_drained_after_stop(&src.ctl->lq)) {
                    exhausted = exhausted | need;
                }
            } else {
                const unsigned long long m = __ballot(need);
                const uint32_t first = wave_claim(queue, m, (uint32_t)__popcll(m), lane);
                if (need) {
                    const uint32_t i = first + wave_rank(m, lane);
                    if (i < nitems) {
                        src.get(i, base, len, dst);
                        got = true;
                    } else {
                        exhausted = true;
                    }
                }
            }
            // the chunk (or the end of work) goes to the pair's B lane
            const int srcl = lane & ~1;
            const bool pgot = __shfl((int)got, srcl, 64) != 0;
            exhausted = __shfl((int)exhausted, srcl, 64) != 0;
            if (__ballot(pgot)) {
                const uint64_t b1 = (uint64_t)__shfl((unsigned long long)reinterpret_cast<uintptr_t>(base), srcl, 64);
                const uint64_t ln = (uint64_t)__shfl((unsigned long long)len, srcl, 64);
                const uint64_t ds = (uint64_t)__shfl((unsigned long long)reinterpret_cast<uintptr_t>(dst), srcl, 64);
                if (pgot) {
                    base = reinterpret_cast<const uint8_t *>(b1);
                    len = ln;
                    dst = reinterpret_cast<uint8_t *>(ds);
                }
                if constexpr (Source::kRing) {
                    const uint64_t b2 = (uint64_t)__shfl((unsigned long long)reinterpret_cast<uintptr_t>(base2), srcl, 64);
                    const uint32_t l1 = (uint32_t)__shfl((int)len1, srcl, 64);
                    const uint32_t pg = (uint32_t)__shfl((int)pages, srcl, 64);
                    if (pgot) {
                        base2 = reinterpret_cast<const uint8_t *>(b2);
                        len1 = l1;
                        pages = pg;
                    }
                }
                if (pgot) {
                    if constexpr (SuffixOf<Source>::kBytes != 0) nblk = pbss::sha256_blocks(len, SuffixOf<Source>::kBytes);
                    else nblk = (len + 8) / 64 + 1;
                    blk = roleB ? 1ull : 0ull;
                    have = blk < nblk;
                }
            }
        };
        auto prep = [&](const int s, auto... key) {
            const unsigned long long hm = __ballot(have);
            const bool pair_busy = ((hm >> (lane & ~1)) & 3ull) != 0ull;
            acquire(!roleB && !pair_busy && !exhausted);
            uint32_t c = 0;
            const uint8_t *p = reinterpret_cast<const uint8_t *>(kIdleBlock);  // (unconditional request: k_sha256_pair)
            const uint8_t *bb = base;
            uint64_t off = 0;
            bool tail = false, last = false;
            if (have) {
                off = blk * 64;
                if constexpr (Source::kRing) bb = (off < len1) ? base : base2;
                last = blk + 1 == nblk;
                if (off + 64 <= len) p = bb + off;
                else tail = true;
                c = 1u | (last ? 2u : 0u);
                dstv[s] = dst;
                if constexpr (Source::kRing) pagesv[s] = pages;
                blk += 2;
                if (blk >= nblk) have = false;
            }
            sha256_request_block(p, R[s], selv[s]);
            if (tail) {
                if constexpr (sizeof...(key) != 0) sha256_tail_words_keyed(bb, len, off, last, key..., R[s]);
                else sha256_tail_words(bb, len, off, last, R[s]);
                selv[s] = 0x00010203u;
            }
            cflag[s] = c;
        };
        // where this lane's expanded block goes: plane E (A lanes) or O (B lanes), always the row of the pair's A lane
        const int wrow = lane & ~1, wplane = lane & 1;

#pragma unroll
        for (int s = 0; s < D; ++s) {
            if constexpr (SuffixOf<Source>::kBytes != 0) prep(s, src.key);
            else prep(s);
        }
        bool drained = false;  // (one exit behind the last slot: k_sha256_pair)
        [[maybe_unused]] bool wg_busy = false;
        [[maybe_unused]] RingProbe probe;
        [[maybe_unused]] const bool probe_on = blockIdx.x == 0 && wave == 2;
        while (!drained) {
#pragma unroll
            for (int s = 0; s < D; ++s) {
                {
                    const int pb = s & 1;
                    uint32_t W[16];
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        W[j] = __builtin_amdgcn_perm(R[s][j + 1], R[s][j], selv[s]);
                        // pinned HERE (an empty volatile statement is neither sunk into the `any_cur` branch below nor
                        // moved behind prep(s)): the slot's registers must be dead before its refill is requested, or
                        // the refill lands in a second register set that is copied back at the loop's end behind an
                        // s_waitcnt vmcnt(0) — every block would again be awaited in the step that requested it
                        asm volatile("" : "+v"(W[j]));
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    const uint32_t c = cflag[s];
                    uint8_t *cur_dst = dstv[s];
                    if constexpr (Source::kRing) {
                        // the chunk's LAST block is in registers (the partner's blocks of this step and all earlier ones
                        // too: same load instructions, same wait): the pair is free for the service's accounting, and the
                        // chunk's page references are dropped, as the pair form does
                        {
                            const unsigned long long mdone = __ballot((c & 2u) != 0u);
                            if (mdone && lane == (__ffsll((long long)mdone) - 1)) atomicSub(&src.ctl->xp_busy, (uint32_t)__popcll(mdone));
                        }
                        if (c & 2u) ring_release_pages(src, pagesv[s]);
                    }
                    if constexpr (SuffixOf<Source>::kBytes != 0) prep(s, src.key);
                    else prep(s);
                    const bool any_cur = __any(c & 1u);
                    if (any_cur) {
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            uint32_t x[4];
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const int t = 4 * q + j;
                                x[j] = ((t < 16) ? W[t] : sha256_sched(W, t)) + kSha256K[t];
                            }
                            wkbuf[pb][wplane][q][wrow] = make_uint4(x[0], x[1], x[2], x[3]);
                        }
                    }
                    ctrl[pb][wplane][ci] = c;
                    dstp[pb][wplane][ci] = cur_dst;
                    bool live = any_cur;
                    if constexpr (Source::kRing) {
                        // stays until `stop` has reached every pair and the block FIFO has drained; naps while idle. (The
                        // idle self-stop of a silent host is the pair service's business: it raises `stop` for both.)
                        const bool wave_done = __ballot(!exhausted) == 0ull;
                        live = any_cur || !wave_done;
                        if (!any_cur && !wave_done && !wg_busy) __builtin_amdgcn_s_sleep(48);  // (never while the sibling pair works)
                        if (lane == 0) curw[pr][pb] = any_cur ? 1u : 0u;
                        if (probe_on) ring_probe_step(src, probe, any_cur, 3, lane);  // (a step of this form = TWO blocks per chunk)
                    }
                    if (lane == 0) alive[pr][pb] = live ? 1u : 0u;
                    __syncthreads();
                    drained = drained || __builtin_amdgcn_readfirstlane(any_alive(pb)) == 0u;
                    if constexpr (Source::kRing) wg_busy = (curw[0][pb] | curw[1][pb]) != 0u;
                }
            }
        }
    } else {
        // CONSUMER: lane A = e,f,g,h (H4..H7), lane B = a,b,c,d (H0..H3), lock-step
        const XpRole R{roleB ? 2u : 6u, roleB ? 13u : 11u, roleB ? 22u : 25u, roleB ? 0xffffffffu : 0u};
        const uint32_t role = R.role;
        uint32_t ivr[4];
        ivr[0] = roleB ? 0x6a09e667u : 0x510e527fu;
        ivr[1] = roleB ? 0xbb67ae85u : 0x9b05688cu;
        ivr[2] = roleB ? 0x3c6ef372u : 0x1f83d9abu;
        ivr[3] = roleB ? 0xa54ff53au : 0x5be0cd19u;
        uint32_t HR[4] = {ivr[0], ivr[1], ivr[2], ivr[3]};
        struct Blk {
            uint32_t al, c;
            uint8_t *d;
            uint4 wk[16];
        };
        auto fetch = [&](Blk &x, const int pb, const int plane) {
            x.al = any_alive(pb);
            x.c = ctrl[pb][plane][ci];
            x.d = dstp[pb][plane][ci];
#pragma unroll
            for (int q = 0; q < 16; ++q) x.wk[q] = wkbuf[pb][plane][q][lane];
        };
        auto rounds = [&](const Blk &x) {
            if (x.c & 1u) {
                // slot-round r: A computes e(r+1), B computes a(r-1). B's first two slot-rounds only shift its start
                // values into place (a(-1) = b, a(0) = a), A's last two are idle: per-lane selects at both ends.
                uint32_t x0 = xp_sel(role, HR[0], HR[2]), x1 = xp_sel(role, HR[1], HR[3]), x2 = HR[2], x3 = HR[3];
                xp_round4<true>(x0, x1, x2, x3, x.wk[0], R, HR[1], HR[0]);
#pragma unroll
                for (int g = 1; g < 16; ++g) xp_round4<false>(x0, x1, x2, x3, x.wk[g], R);
                // after slot-round 63: (x0..x3) = results of slot-rounds 63, 62, 61, 60 = A's e(64..61)
                const uint32_t o63 = x0, o62 = x1, o61 = x2, o60 = x3;
                xp_round2(x0, x1, x2, x3, x.wk[15].w, R);
                // ... after 65: x0, x1 = results of 65, 64; B's a(64..61) = results of 65, 64, 63, 62
                HR[0] += xp_sel(role, o63, x0);
                HR[1] += xp_sel(role, o62, x1);
                HR[2] += xp_sel(role, o61, o63);
                HR[3] += xp_sel(role, o60, o62);
                if (x.c & 2u) {
                    // B holds digest words 0..3, A words 4..7: one 16-byte store each
                    PBSK_GLOBAL uint32_t *o = (PBSK_GLOBAL uint32_t *)x.d + (roleB ? 0 : 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = __builtin_bswap32(HR[j]);
                    if constexpr (Source::kRing) ring_cell_publish((PBSK_GLOBAL uint32_t *)x.d);  // both halves, then the flag
#pragma unroll
                    for (int j = 0; j < 4; ++j) HR[j] = ivr[j];
                }
            }
        };
        // Software-pipelined like the pair form: the LDS reads of the NEXT block are issued before the rounds of the current
        // one run from registers. A producer step = two blocks (planes E, O) and one barrier.
        Blk E0, O0, E1, O1;
        __syncthreads();  // barrier 0: step 0 is published (buffer 0)
        fetch(E0, 0, 0);
        for (;;) {
            if (!E0.al) break;
            fetch(O0, 0, 1);
            __builtin_amdgcn_sched_barrier(0);
            rounds(E0);
            __syncthreads();  // step k+1 published (buffer 1); the producer may now overwrite buffer 0: O0 is in registers
            fetch(E1, 1, 0);
            __builtin_amdgcn_sched_barrier(0);
            rounds(O0);
            if (!E1.al) break;
            fetch(O1, 1, 1);
            __builtin_amdgcn_sched_barrier(0);
            rounds(E1);
            __syncthreads();
            fetch(E0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            rounds(O1);
        }
    }
}

// -------------------------------------------------------------------------------------
// Longest-first queue order + workgroup budget for the SHA kernel (one small workgroup).
// A batch's makespan is max(longest chunk, total work / lanes): starting the long chunks first
// and letting lanes pull the short ones afterwards reaches that bound with FEWER lanes than
// chunks, which leaves CUs free for the next batch's kernels (batches overlap on separate
// streams). Counting sort by size class (no comparison sort needed for a scheduling order).
__global__ __launch_bounds__(1024) void k_order(const uint8_t *data, const pbsgpu_segment *segs, const pbsgpu_record *recs,
                                                const uint32_t *nrec_p, uint32_t shift, uint4 *qdesc, uint32_t *wg_limit,
                                                uint32_t max_wgs,
                                                const uint32_t *maxcnt, uint32_t cap, uint32_t slack_pct) {
    // a scan tile overflowed its slot list: this pass will be re-run with a larger capacity, so do not
    // spend a SHA pass on its (incomplete) cut list
    if (maxcnt && *maxcnt > cap) {
        if (threadIdx.x == 0) *wg_limit = 0;
        return;
    }
    constexpr int BINS = 1024;
    __shared__ uint32_t hist[BINS];
    __shared__ uint32_t base[BINS];
    __shared__ unsigned long long tot_blocks;
    __shared__ uint32_t longest;
    const uint32_t n = *nrec_p;
    for (int i = threadIdx.x; i < BINS; i += blockDim.x) hist[i] = 0;
    if (threadIdx.x == 0) { tot_blocks = 0; longest = 0; }
    __syncthreads();
    unsigned long long my_blocks = 0;
    uint32_t my_long = 0;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t sz = recs[i].size;
        uint32_t b = sz >> shift;
        if (b >= BINS) b = BINS - 1;
        atomicAdd(&hist[BINS - 1 - b], 1u);  // descending size
        const uint32_t blocks = (sz + 8) / 64 + 1;
        my_blocks += blocks;
        my_long = max(my_long, blocks);
    }
    atomicAdd(&tot_blocks, my_blocks);
    atomicMax(&longest, my_long);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int i = 0; i < BINS; ++i) { base[i] = run; run += hist[i]; }
        // lanes needed so that total work / lanes stays below the longest chain (slack_pct, default 25 %)
        const unsigned long long lg = longest ? longest : 1;
        unsigned long long lanes = (tot_blocks * (100 + slack_pct) / 100 + lg - 1) / lg;
        uint32_t wgs = (uint32_t)((lanes + 127) / 128);
        const uint32_t need = (n + 127) / 128;
        if (wgs > need) wgs = need;
        if (wgs < 1) wgs = 1;
        if (wgs > max_wgs) wgs = max_wgs;
        *wg_limit = wgs;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        uint32_t b = recs[i].size >> shift;
        if (b >= BINS) b = BINS - 1;
        const uint32_t pos = atomicAdd(&base[BINS - 1 - b], 1u);
        const uint64_t p = (uint64_t)(uintptr_t)(data + segs[recs[i].segment].offset + recs[i].end - recs[i].size);
        qdesc[pos] = make_uint4((uint32_t)p, (uint32_t)(p >> 32), recs[i].size, i);
    }
}

// dense_pct: work per pair-mode lane, in percent of the longest chain, from which the SHA kernel runs its dense (4 pairs
// per CU) form; 0 = never (pbsgpu_engine_options::sha_dense_pct, default 150)
bool sha256_dense_pays(uint64_t total_blocks, uint64_t longest_blocks, int num_cus, uint32_t dense_pct) {
    if (!dense_pct) return false;
    if (longest_blocks < 1) longest_blocks = 1;
    return total_blocks * 100ull > (uint64_t)dense_pct * longest_blocks * 128ull * (uint64_t)num_cus;
}

hipError_t launch_order(const uint8_t *data, const pbsgpu_segment *segs, const pbsgpu_record *recs, const uint32_t *nrec,
                        uint32_t max_chunk, uint4 *qdesc, uint32_t *wg_limit, int num_cus, const uint32_t *maxcnt, uint32_t cap, uint32_t slack_pct,
                        hipStream_t st) {
    uint32_t shift = 0;
    while (((uint64_t)max_chunk >> shift) >= 1024) ++shift;
    hipLaunchKernelGGL(k_order, dim3(1), dim3(1024), 0, st, data, segs, recs, nrec, shift, qdesc, wg_limit, (uint32_t)num_cus,
                       maxcnt, cap, slack_pct);
    return hipGetLastError();
}

// Dynamic-LDS padding: a wave already saturates its SIMD's integer issue rate (one wave64 VALU op
// per ~4 cycles), so a co-resident wave halves the speed of the serial chain. Requesting LDS the
// kernel never touches caps residency at one wave per SIMD (2 pairs / 4 single waves per CU).
constexpr size_t kPairLdsPad = 16u << 10;  // ~69 KB static + 16 KB > 80 KB -> exactly one pair workgroup per CU
constexpr size_t kLaneLdsPad = 36u << 10;  // four single-wave workgroups per CU

// `form` (pbsgpu_engine_options::sha_form): 0 = wave pairs (default), 1 = the single-wave kernel, 2 = the express form (two
// lanes per chunk) for EVERY chunk of the batch path — A/B measurements and the parity tests of those kernels
// host-decided form (descriptor jobs, whole-segment hashing): exactly one launch
template <typename Source>
static hipError_t launch_pair(unsigned grid, bool dense, hipStream_t st, Source src, uint32_t nitems, uint32_t *queue, int form) {
    if (form == 2) {  // (131 KB static LDS: one workgroup per CU without padding)
        hipLaunchKernelGGL((k_sha256_xpair<Source>), dim3(grid * (dense ? 4u : 2u)), dim3(256), 0, st, src, (const uint32_t *)nullptr,
                           nitems, queue, (const uint32_t *)nullptr);
        return hipGetLastError();
    }
    if (dense) {
        hipLaunchKernelGGL((k_sha256_pair<Source, true>), dim3(grid), dim3(512), 0, st, src, (const uint32_t *)nullptr,
                           nitems, queue, (const uint32_t *)nullptr);
    } else {
        const size_t pad = kPairLdsPad;
        hipError_t e = allow_lds(&k_sha256_pair<Source, false>, pad);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((k_sha256_pair<Source, false>), dim3(grid), dim3(256), pad, st, src,
                           (const uint32_t *)nullptr, nitems, queue, (const uint32_t *)nullptr);
    }
    return hipGetLastError();
}

// the keyed twins of the two launchers below (at the end of this file: the keyed instances are the LAST ones this unit
// instantiates, so every kernel that was here before them keeps its place in the object and its ISA text, labels included)
static hipError_t launch_sha256_records_keyed(pbsgpu_record *recs, const uint32_t *nrec, uint32_t *queue, const uint4 *qdesc,
                                              const uint32_t *wg_limit, int num_cus, bool dense, int form, hipStream_t st,
                                              const uint32_t *key);
static hipError_t launch_sha256_segments_keyed(const uint8_t *data, const pbsgpu_segment *segs, uint32_t nseg, uint8_t *digests,
                                               uint32_t *queue, int num_cus, bool dense, int form, hipStream_t st, const uint32_t *key);

hipError_t launch_sha256_records(pbsgpu_record *recs, const uint32_t *nrec, uint32_t *queue, const uint4 *qdesc,
                                 const uint32_t *wg_limit, int num_cus, bool dense, int form, hipStream_t st, const uint32_t *key) {
    if (key) return launch_sha256_records_keyed(recs, nrec, queue, qdesc, wg_limit, num_cus, dense, form, st, key);
    RecordSource src{recs, qdesc};
    if (form == 2) {
        hipLaunchKernelGGL((k_sha256_xpair<RecordSource>), dim3((unsigned)num_cus), dim3(256), 0, st, src, nrec, 0u, queue,
                           wg_limit);
    } else if (form == 0) {
        if (dense) {
            hipLaunchKernelGGL((k_sha256_pair<RecordSource, true>), dim3((unsigned)num_cus), dim3(512), 0, st, src, nrec,
                               0u, queue, wg_limit);
        } else {
            hipError_t e = allow_lds(&k_sha256_pair<RecordSource, false>, kPairLdsPad);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL((k_sha256_pair<RecordSource, false>), dim3((unsigned)num_cus), dim3(256), kPairLdsPad, st, src,
                               nrec, 0u, queue, wg_limit);
        }
    } else {
        hipError_t e = allow_lds(&k_sha256<RecordSource>, kLaneLdsPad);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((k_sha256<RecordSource>), dim3((unsigned)num_cus * 4u), dim3(64), kLaneLdsPad, st, src, nrec, 0u,
                           queue, wg_limit, 0u);
    }
    return hipGetLastError();
}

hipError_t launch_sha256_segments(const uint8_t *data, const pbsgpu_segment *segs, uint32_t nseg, uint8_t *digests,
                                  uint32_t *queue, int num_cus, bool dense, int form, hipStream_t st, const uint32_t *key) {
    if (nseg == 0) return hipSuccess;
    if (key) return launch_sha256_segments_keyed(data, segs, nseg, digests, queue, num_cus, dense, form, st, key);
    SegmentSource src{data, segs, digests};
    if (form != 1) {
        unsigned g2 = (unsigned)num_cus;
        const unsigned need2 = (nseg + (dense ? 255u : 127u)) / (dense ? 256u : 128u);
        if (g2 > need2) g2 = need2;
        return launch_pair(g2, dense, st, src, nseg, queue, form);
    }
    hipError_t e = allow_lds(&k_sha256<SegmentSource>, kLaneLdsPad);
    if (e != hipSuccess) return e;
    // `dense` with this form (sha_form 1 + sha_dense_pct): EIGHT single-wave workgroups per CU, two waves per SIMD — a measurement
    // (profiles/r06_sha_forms_full_lanes.log section 3): with two waves on a SIMD v_add_u32 / v_xor_b32 issue at twice the rate
    // of the three-operand forms (profiles/r01_ubench_opcode_issue_cost.log)
    const size_t pad = dense ? kLaneLdsPad / 2 : kLaneLdsPad;
    unsigned grid = (unsigned)num_cus * (dense ? 8u : 4u);
    const unsigned need = (nseg + 63) / 64;
    if (grid > need) grid = need;
    hipLaunchKernelGGL((k_sha256<SegmentSource>), dim3(grid), dim3(64), pad, st, src, (const uint32_t *)nullptr,
                       nseg, queue, (const uint32_t *)nullptr, 0u);
    return hipGetLastError();
}

// ---- the page ring's services (ring.cpp starts them; the cut rounds that feed them: ring_kernels.hip) ----------------
// The EXPRESS service (k_sha256_xpair: two lanes per chunk, the long-chunk queue only) on its own CUs beside the pair
// service: same LDS rule, same `stop`.
hipError_t launch_ring_service_xp(const RingSource &q, unsigned workgroups, hipStream_t st) {
    hipFuncAttributes fa{};
    hipError_t e = hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(&k_sha256_xpair<RingSource>));
    if (e != hipSuccess) return e;
    size_t pad = (160u << 10) > fa.sharedSizeBytes ? (160u << 10) - fa.sharedSizeBytes : 0;
    pad &= ~(size_t)255;
    e = allow_lds(&k_sha256_xpair<RingSource>, pad);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_sha256_xpair<RingSource>), dim3(workgroups), dim3(256), pad, st, q, (const uint32_t *)nullptr, 0u,
                       (uint32_t *)nullptr, (const uint32_t *)nullptr);
    return hipGetLastError();
}

// The LANES service (k_sha256_lanes: one lane per chunk, the short-chunk queue only) on its own CUs: same LDS rule, same `stop`.
// `dense` (PBSGPU_RING_F_DENSE_LANES): eight waves per workgroup, two per SIMD — 84 chain-blocks per us and CU against 77-81
// (with two waves on a SIMD the two-operand adds and xors issue at twice the rate of the three-operand forms), every chain at
// ~6 us per block (profiles/r06_sha_forms_full_lanes.log section 3)
hipError_t launch_ring_service_lanes(const RingSource &q, unsigned workgroups, hipStream_t st, bool dense) {
    const size_t pad = (size_t)(160u << 10) & ~(size_t)255;
    hipError_t e = allow_lds(&k_sha256_lanes, pad);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sha256_lanes, dim3(workgroups), dim3(dense ? 512 : 256), pad, st, q);
    return hipGetLastError();
}

template <bool DENSE>
static hipError_t launch_ring_service_form(const RingSource &q, unsigned workgroups, hipStream_t st) {
    // the whole LDS of the CU: one workgroup per CU (a co-resident wave on a chain's SIMD halves the chain's speed), and
    // no room for any other kernel that asks for LDS (kRingLdsTag, the scan's table)
    hipFuncAttributes fa{};
    hipError_t e = hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(&k_sha256_pair<RingSource, DENSE>));
    if (e != hipSuccess) return e;
    size_t pad = (160u << 10) > fa.sharedSizeBytes ? (160u << 10) - fa.sharedSizeBytes : 0;
    pad &= ~(size_t)255;
    e = allow_lds(&k_sha256_pair<RingSource, DENSE>, pad);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_sha256_pair<RingSource, DENSE>), dim3(workgroups), dim3(DENSE ? 512 : 256), pad, st, q,
                       (const uint32_t *)nullptr, 0u, (uint32_t *)nullptr, (const uint32_t *)nullptr);
    return hipGetLastError();
}
// dense (PBSGPU_RING_F_DENSE_SERVICE): four pairs per workgroup, two waves per SIMD — DESIGN.md 5.2 for what it buys and costs
hipError_t launch_ring_service(const RingSource &q, unsigned workgroups, hipStream_t st, bool dense) {
    return dense ? launch_ring_service_form<true>(q, workgroups, st) : launch_ring_service_form<false>(q, workgroups, st);
}

// ---- keyed digests (KeyedRecordSource, KeyedSegmentSource): the same launches as launch_sha256_records and
// launch_sha256_segments, over the keyed instances --------------------------------------------------------------------------
static hipError_t launch_sha256_records_keyed(pbsgpu_record *recs, const uint32_t *nrec, uint32_t *queue, const uint4 *qdesc,
                                              const uint32_t *wg_limit, int num_cus, bool dense, int form, hipStream_t st,
                                              const uint32_t *key) {
    KeyedRecordSource src{{recs, qdesc}, key};
    if (form == 2) {
        hipLaunchKernelGGL((k_sha256_xpair<KeyedRecordSource>), dim3((unsigned)num_cus), dim3(256), 0, st, src, nrec, 0u, queue,
                           wg_limit);
    } else if (form == 0) {
        if (dense) {
            hipLaunchKernelGGL((k_sha256_pair<KeyedRecordSource, true>), dim3((unsigned)num_cus), dim3(512), 0, st, src, nrec,
                               0u, queue, wg_limit);
        } else {
            hipError_t e = allow_lds(&k_sha256_pair<KeyedRecordSource, false>, kPairLdsPad);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL((k_sha256_pair<KeyedRecordSource, false>), dim3((unsigned)num_cus), dim3(256), kPairLdsPad, st, src,
                               nrec, 0u, queue, wg_limit);
        }
    } else {
        hipError_t e = allow_lds(&k_sha256<KeyedRecordSource>, kLaneLdsPad);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((k_sha256<KeyedRecordSource>), dim3((unsigned)num_cus * 4u), dim3(64), kLaneLdsPad, st, src, nrec, 0u,
                           queue, wg_limit, 0u);
    }
    return hipGetLastError();
}

static hipError_t launch_sha256_segments_keyed(const uint8_t *data, const pbsgpu_segment *segs, uint32_t nseg, uint8_t *digests,
                                               uint32_t *queue, int num_cus, bool dense, int form, hipStream_t st, const uint32_t *key) {
    KeyedSegmentSource src{{data, segs, digests}, key};
    if (form != 1) {
        unsigned g2 = (unsigned)num_cus;
        const unsigned need2 = (nseg + (dense ? 255u : 127u)) / (dense ? 256u : 128u);
        if (g2 > need2) g2 = need2;
        return launch_pair(g2, dense, st, src, nseg, queue, form);
    }
    hipError_t e = allow_lds(&k_sha256<KeyedSegmentSource>, kLaneLdsPad);
    if (e != hipSuccess) return e;
    const size_t pad = dense ? kLaneLdsPad / 2 : kLaneLdsPad;  // (launch_sha256_segments: eight single-wave workgroups per CU)
    unsigned grid = (unsigned)num_cus * (dense ? 8u : 4u);
    const unsigned need = (nseg + 63) / 64;
    if (grid > need) grid = need;
    hipLaunchKernelGGL((k_sha256<KeyedSegmentSource>), dim3(grid), dim3(64), pad, st, src, (const uint32_t *)nullptr,
                       nseg, queue, (const uint32_t *)nullptr, 0u);
    return hipGetLastError();
}

}  // namespace pbsk
