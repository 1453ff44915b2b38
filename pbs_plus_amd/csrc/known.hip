// Device-resident known-chunk set (pbsgpu_known_*, include/pbsgpu.h): the "known-chunk check" of the backup writer's
// inner loop (scan -> cut -> SHA-256 -> known-chunk check -> upload -> DIDX append). A session loads the
// previous snapshot's indexes (commit_orchestrate.go:127-158) and then asks, batch by batch, which chunks the server
// already has; the first occurrence of a new digest is uploaded, every later one is a reference.
//
// Table: a power-of-two open-addressing table with linear probing, two arrays —
//   tags[slot]    u64: digest bytes 0..7 (little endian), 0 reserved for "empty" and mapped to 1
//   digs[slot][4] u64: the 32 digest bytes
// The home slot comes from a mix of digest bytes 8..31, not from the tag bits, so digests crafted to share 8 or 16
// leading bytes still spread. A tag match is only a filter: equality is always decided on all 32 bytes. The load factor
// stays <= 1/2 (the table is rebuilt twice as large on the device before an insert would pass it).
//
// Exactness (the sequential `set` rule, independent of thread scheduling):
//   1. k_known_lookup (read-only on the table): before[i] = the digest was in the set before the call.
//   2. a stable radix sort of (32-bit digest key, index) pairs, then k_known_mark: dup[i] = an earlier record of this
//      call carries the same digest (equal digests have equal keys, so they share a run, in index order);
//      new[i] = !before[i] && !dup[i], known[i] = !new[i] — a record is new iff it is the first occurrence of a digest the
//      set did not hold.
//   3. k_known_insert (insert = 1), only for new records: their digests are pairwise distinct and absent from the table,
//      so an inserting thread never needs to compare against a slot another thread is writing — it skips every
//      occupied slot and claims an empty one with a 64-bit device-scope CAS on the tag, then writes the 32 bytes.
//   Every read of a slot written by another workgroup happens in a LATER kernel on the same stream: the kernel boundary
//   is the only ordering (no in-kernel acquire / release across the XCDs' L2s).
//
// The batch dedup (pbsgpu_dedup_host / _device) is the same marking with no table: k_known_keys in place of the lookup,
// so every before[i] = 0 and known[i] = dup[i] — an earlier record of the batch carries the same digest.
//
// The pass also comes in pieces (known_enqueue_mark / known_reserve / known_enqueue_insert, engine_internal.h) that run on a
// stream and arrays the caller owns: the fused upload of blob.hip builds its encode plan from known[] between the marking
// and the insert, and gives the insert flags of its own when the blobs do not fit.
#include <rocprim/device/device_radix_sort.hpp>

#include "engine_internal.h"
#include "known_hash.h"

using namespace pbse;

namespace pbsk {

__device__ __forceinline__ bool known_slot_eq(const uint64_t *digs, uint64_t slot, const uint64_t w[4]) {
    const uint64_t *d = digs + slot * 4;
    return d[0] == w[0] && d[1] == w[1] && d[2] == w[2] && d[3] == w[3];
}

__global__ __launch_bounds__(256) void k_known_lookup(const uint8_t *base, uint32_t stride, uint64_t n,
                                                      const uint64_t *tags, const uint64_t *digs, uint64_t mask,
                                                      uint32_t *keys, uint32_t *idx, uint8_t *before) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t w[4];
    known_load(base, stride, i, w);
    const uint64_t h = known_home(w);
    const uint64_t tag = known_tag(w[0]);
    uint8_t found = 0;
    for (uint64_t s = h & mask;; s = (s + 1) & mask) {  // terminates: the table is at most half full
        const uint64_t t = tags[s];
        if (t == 0) break;
        if (t == tag && known_slot_eq(digs, s, w)) {
            found = 1;
            break;
        }
    }
    before[i] = found;
    keys[i] = known_key(h, w);
    idx[i] = (uint32_t)i;
}

// k_known_lookup without a table (the batch dedup): nothing is known before the call
__global__ __launch_bounds__(256) void k_known_keys(const uint8_t *base, uint32_t stride, uint64_t n, uint32_t *keys,
                                                    uint32_t *idx, uint8_t *before) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t w[4];
    known_load(base, stride, i, w);
    before[i] = 0;
    keys[i] = known_key(known_home(w), w);
    idx[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void k_known_mark(const uint8_t *base, uint32_t stride, uint64_t n,
                                                    const uint32_t *keys, const uint32_t *idx, const uint8_t *before,
                                                    uint8_t *known, uint64_t *stats4) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool is_new = false;
    uint64_t size = 0;
    if (j < n) {
        const uint32_t i = idx[j];
        if (stride == 48) size = *reinterpret_cast<const uint32_t *>(base + (uint64_t)i * 48 + 44);
        is_new = !before[i];
        if (is_new) {  // (a record known before needs no walk: it is known either way)
            uint64_t w[4];
            known_load(base, stride, i, w);
            const uint32_t key = keys[j];
            for (uint64_t q = j; q > 0 && keys[q - 1] == key; --q) {
                uint64_t v[4];
                known_load(base, stride, idx[q - 1], v);  // stable sort: idx[q-1] < i
                if (v[0] == w[0] && v[1] == w[1] && v[2] == w[2] && v[3] == w[3]) {
                    is_new = false;
                    break;
                }
            }
        }
        known[i] = is_new ? 0 : 1;
    }
    // stats: [0] records, [1] new, [2] total bytes, [3] new bytes (wave-reduced atomics)
    uint64_t c_all = (j < n) ? 1 : 0, c_new = is_new ? 1 : 0;
    uint64_t b_all = size, b_new = is_new ? size : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        c_all += __shfl_xor(c_all, d, 64);
        c_new += __shfl_xor(c_new, d, 64);
        b_all += __shfl_xor(b_all, d, 64);
        b_new += __shfl_xor(b_new, d, 64);
    }
    if ((threadIdx.x & 63) == 0 && c_all) {
        atomicAdd(reinterpret_cast<unsigned long long *>(stats4 + 0), (unsigned long long)c_all);
        atomicAdd(reinterpret_cast<unsigned long long *>(stats4 + 1), (unsigned long long)c_new);
        atomicAdd(reinterpret_cast<unsigned long long *>(stats4 + 2), (unsigned long long)b_all);
        atomicAdd(reinterpret_cast<unsigned long long *>(stats4 + 3), (unsigned long long)b_new);
    }
}

// skip-occupied insert of a digest that is absent from the table and distinct from every other one inserted beside it
__device__ __forceinline__ void known_put(uint64_t *tags, uint64_t *digs, uint64_t mask, uint64_t h, uint64_t tag,
                                          const uint64_t w[4]) {
    for (uint64_t s = h & mask;; s = (s + 1) & mask) {
        if (tags[s] != 0) continue;
        if (atomicCAS(reinterpret_cast<unsigned long long *>(tags + s), 0ull, (unsigned long long)tag) == 0ull) {
            uint64_t *d = digs + s * 4;
            d[0] = w[0];
            d[1] = w[1];
            d[2] = w[2];
            d[3] = w[3];
            return;
        }
    }
}

__global__ __launch_bounds__(256) void k_known_insert(const uint8_t *base, uint32_t stride, uint64_t n,
                                                      const uint8_t *known, uint64_t *tags, uint64_t *digs,
                                                      uint64_t mask) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || known[i]) return;
    uint64_t w[4];
    known_load(base, stride, i, w);
    known_put(tags, digs, mask, known_home(w), known_tag(w[0]), w);
}

// growth: every stored digest into the larger table (all distinct, the new table starts empty)
__global__ __launch_bounds__(256) void k_known_rehash(const uint64_t *old_tags, const uint64_t *old_digs,
                                                      uint64_t old_slots, uint64_t *tags, uint64_t *digs,
                                                      uint64_t mask) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < old_slots; s += stride) {
        const uint64_t tag = old_tags[s];
        if (tag == 0) continue;
        uint64_t w[4];
        const uint64_t *d = old_digs + s * 4;
        w[0] = d[0];
        w[1] = d[1];
        w[2] = d[2];
        w[3] = d[3];
        known_put(tags, digs, mask, known_home(w), tag, w);
    }
}

}  // namespace pbsk

struct pbsgpu_known {
    pbsgpu_engine *eng = nullptr;
    DevBuf tags, digs;  // exact-size table (slots * 8, slots * 32 bytes)
    uint64_t slots = 0;
    uint64_t count = 0;
};

namespace {

constexpr uint64_t kMinSlots = 1024;
constexpr uint64_t kDefaultCapacity = 1ull << 16;
constexpr uint64_t kMaxCount = 1ull << 32;  // set size stays below 2^32

uint64_t pow2_at_least(uint64_t v) {
    uint64_t p = kMinSlots;
    while (p < v) p <<= 1;
    return p;
}

// an empty table of `slots` slots, enqueued zeroing of the tags on `st`; nothing is touched on failure
int alloc_table(uint64_t slots, hipStream_t st, DevBuf &tags, DevBuf &digs) {
    void *t = nullptr, *d = nullptr;
    if (hipMalloc(&t, slots * 8) != hipSuccess) {
        (void)hipGetLastError();
        return PBSGPU_E_NOMEM;
    }
    if (hipMalloc(&d, slots * 32) != hipSuccess) {
        (void)hipGetLastError();
        dev_free(t);
        return PBSGPU_E_NOMEM;
    }
    tags.p = t;
    tags.cap = slots * 8;
    digs.p = d;
    digs.cap = slots * 32;
    HIPCHK(hipMemsetAsync(tags.p, 0, slots * 8, st));
    return PBSGPU_OK;
}

unsigned blocks_for(uint64_t n) { return (unsigned)((n + 255) / 256); }

// rebuild the table with room for `want` digests at load <= 1/2; the old table stays as it was unless this succeeds
int grow(pbsgpu_known *k, uint64_t want, hipStream_t st) {
    const uint64_t slots = std::max(pow2_at_least(want * 2), k->slots * 2);
    DevBuf tags, digs;
    CHK(alloc_table(slots, st, tags, digs));
    if (k->count) {
        const uint64_t nb = std::min<uint64_t>(blocks_for(k->slots), 16384);
        hipLaunchKernelGGL(pbsk::k_known_rehash, dim3((unsigned)nb), dim3(256), 0, st, k->tags.as<uint64_t>(),
                           k->digs.as<uint64_t>(), k->slots, tags.as<uint64_t>(), digs.as<uint64_t>(), slots - 1);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(st));  // the rehash has read the old table before it goes
    k->tags = std::move(tags);         // (DevBuf move-assign releases the old buffer through dev_free)
    k->digs = std::move(digs);
    k->slots = slots;
    return PBSGPU_OK;
}

}  // namespace

namespace pbse {

int known_sort_bytes(uint64_t n, hipStream_t st, size_t *bytes) {
    size_t tmp_bytes = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                     (uint32_t *)nullptr, (size_t)n, 0, 32, st));
    *bytes = tmp_bytes + 256;
    return PBSGPU_OK;
}

int known_enqueue_mark(const pbsgpu_known *k, const KnownPass &p, hipStream_t st) {
    const uint64_t n = p.n;
    uint32_t *keys_alt = p.keys + n, *idx_alt = p.idx + n;
    const unsigned nb = blocks_for(n);
    size_t tmp_bytes = p.tmp_bytes;
    HIPCHK(hipMemsetAsync(p.stats, 0, 32, st));
    if (k)
        hipLaunchKernelGGL(pbsk::k_known_lookup, dim3(nb), dim3(256), 0, st, p.recs, p.stride, n, k->tags.as<uint64_t>(),
                           k->digs.as<uint64_t>(), k->slots - 1, p.keys, p.idx, p.before);
    else
        hipLaunchKernelGGL(pbsk::k_known_keys, dim3(nb), dim3(256), 0, st, p.recs, p.stride, n, p.keys, p.idx, p.before);
    HIPCHK(hipGetLastError());
    HIPCHK(rocprim::radix_sort_pairs(p.tmp, tmp_bytes, p.keys, keys_alt, p.idx, idx_alt, (size_t)n, 0, 32, st));
    hipLaunchKernelGGL(pbsk::k_known_mark, dim3(nb), dim3(256), 0, st, p.recs, p.stride, n, keys_alt, idx_alt, p.before,
                       p.known, p.stats);
    HIPCHK(hipGetLastError());
    return PBSGPU_OK;
}

bool known_may_grow(const pbsgpu_known *k, uint64_t n) { return k->count + n > k->slots / 2; }

int known_reserve(pbsgpu_known *k, uint64_t nnew, hipStream_t st) {
    if (k->count + nnew >= kMaxCount) return PBSGPU_E_CAPACITY;
    if (k->count + nnew > k->slots / 2) CHK(grow(k, k->count + nnew, st));
    return PBSGPU_OK;
}

int known_enqueue_insert(pbsgpu_known *k, const KnownPass &p, const uint8_t *skip, hipStream_t st) {
    hipLaunchKernelGGL(pbsk::k_known_insert, dim3(blocks_for(p.n)), dim3(256), 0, st, p.recs, p.stride, p.n, skip,
                       k->tags.as<uint64_t>(), k->digs.as<uint64_t>(), k->slots - 1);
    HIPCHK(hipGetLastError());
    return PBSGPU_OK;
}

void known_inserted(pbsgpu_known *k, uint64_t nnew) { k->count += nnew; }

pbsgpu_engine *known_engine(const pbsgpu_known *k) { return k->eng; }

}  // namespace pbse

namespace {

// Records (stride 48) or .didx entries (stride 40), host or device; `known` (host, may be NULL) and `stats` (may be NULL
// for the add paths) as pbsgpu_known_classify_*. k = NULL: no table, and insert is false — the batch dedup.
int known_common(pbsgpu_engine *e, pbsgpu_known *k, const uint8_t *src, uint32_t stride, bool on_device, uint64_t n,
                 bool insert, uint8_t *known, pbsgpu_dedup_stats *stats) {
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n == 0) return PBSGPU_OK;
    CHK(set_device(e));
    AuxLease lease(e);
    Slot *s = lease.s;
    const hipStream_t st = s->stream;
    KnownPass p;
    CHK(known_sort_bytes(n, st, &p.tmp_bytes));
    CHK(s->scalars.ensure(SC_COUNT * 4 + 64));
    CHK(s->h_scalars.ensure(64));
    p.recs = src;
    if (!on_device) CHK(put_table(s, src, (size_t)n * stride, &p.recs));
    p.stride = stride;
    p.n = n;
    p.keys = s->take<uint32_t>((size_t)n * 2);
    p.idx = s->take<uint32_t>((size_t)n * 2);
    p.before = s->take<uint8_t>((size_t)n * 2);  // before | known
    p.tmp = s->take<uint8_t>(p.tmp_bytes);
    CHK(s->taken());
    p.known = p.before + n;
    p.stats = reinterpret_cast<uint64_t *>(s->scalars.as<uint8_t>() + 32);
    const uint64_t *hs = s->h_scalars.as<uint64_t>();
    CHK(known_enqueue_mark(k, p, st));
    HIPCHK(hipMemcpyAsync(s->h_scalars.p, p.stats, 32, hipMemcpyDeviceToHost, st));
    if (insert) {
        // the table can only pass its load limit when the whole batch might be new: only then is the number of new
        // digests read back before the insert (one more synchronisation of the lease's stream)
        if (known_may_grow(k, n)) {
            HIPCHK(hipStreamSynchronize(st));
            CHK(known_reserve(k, hs[1], st));
        }
        CHK(known_enqueue_insert(k, p, p.known, st));
    }
    if (known) HIPCHK(hipMemcpyAsync(known, p.known, (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (insert) known_inserted(k, hs[1]);
    if (stats) {
        stats->nrecords = hs[0];
        stats->nunique = hs[1];
        stats->total_bytes = hs[2];
        stats->unique_bytes = hs[3];
    }
    return PBSGPU_OK;
}

}  // namespace

extern "C" {

extern const uint8_t pbsgpu_didx_magic[8];  // hostonly.cpp

int pbsgpu_known_create(pbsgpu_engine *e, uint64_t capacity, pbsgpu_known **out) {
    if (!e || !out || capacity >= kMaxCount) return PBSGPU_E_INVALID;
    *out = nullptr;
    CHK(set_device(e));
    pbsgpu_known *k = new (std::nothrow) pbsgpu_known();
    if (!k) return PBSGPU_E_NOMEM;
    const uint64_t slots = pow2_at_least(2 * (capacity ? capacity : kDefaultCapacity));
    int st = PBSGPU_OK;
    {
        AuxLease lease(e);
        st = alloc_table(slots, lease.s->stream, k->tags, k->digs);
        if (st == PBSGPU_OK && hipStreamSynchronize(lease.s->stream) != hipSuccess) st = PBSGPU_E_HIP;
    }
    if (st != PBSGPU_OK) {
        k->tags.release();
        k->digs.release();
        delete k;
        return st;
    }
    engine_ref(e);
    k->eng = e;
    k->slots = slots;
    *out = k;
    return PBSGPU_OK;
}

void pbsgpu_known_destroy(pbsgpu_known *k) {
    if (!k) return;
    pbsgpu_engine *e = k->eng;
    if (e) (void)set_device(e);
    k->tags.release();
    k->digs.release();
    delete k;
    if (e) engine_unref(e);
}

int pbsgpu_known_count(const pbsgpu_known *k, uint64_t *n) {
    if (!k || !n) return PBSGPU_E_INVALID;
    *n = k->count;
    return PBSGPU_OK;
}

int pbsgpu_known_add_host(pbsgpu_known *k, const pbsgpu_record *recs, uint64_t n) {
    if (!k || (!recs && n) || n >= kMaxCount) return PBSGPU_E_INVALID;
    return known_common(k->eng, k, reinterpret_cast<const uint8_t *>(recs), sizeof(pbsgpu_record), false, n, true, nullptr,
                        nullptr);
}

int pbsgpu_known_add_device(pbsgpu_known *k, const void *drecs, uint64_t n) {
    if (!k || (!drecs && n) || n >= kMaxCount) return PBSGPU_E_INVALID;
    if (n && !is_device_pointer(drecs)) return PBSGPU_E_INVALID;
    return known_common(k->eng, k, static_cast<const uint8_t *>(drecs), sizeof(pbsgpu_record), true, n, true, nullptr,
                        nullptr);
}

int pbsgpu_known_add_didx(pbsgpu_known *k, const uint8_t *didx, uint64_t nbytes) {
    if (!k || !didx) return PBSGPU_E_INVALID;
    // exactly what pbsgpu_didx_decode validates (the index checksum is not verified)
    if (nbytes < PBSGPU_DIDX_HEADER_SIZE || std::memcmp(didx, pbsgpu_didx_magic, 8) != 0) return PBSGPU_E_INVALID;
    const uint64_t body = nbytes - PBSGPU_DIDX_HEADER_SIZE;
    if (body % 40) return PBSGPU_E_INVALID;
    const uint64_t n = body / 40;
    if (n >= kMaxCount) return PBSGPU_E_INVALID;
    const uint8_t *ent = didx + PBSGPU_DIDX_HEADER_SIZE;
    uint64_t prev = 0;
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t end = 0;
        for (int b = 0; b < 8; ++b) end |= (uint64_t)ent[i * 40 + b] << (8 * b);
        if (end < prev || end - prev > 0xffffffffull) return PBSGPU_E_INVALID;
        prev = end;
    }
    // the 40-byte entries go to the device as they are: the kernels read the digest at offset 8 of either layout
    return known_common(k->eng, k, ent, 40, false, n, true, nullptr, nullptr);
}

int pbsgpu_dedup_host(pbsgpu_engine *e, const pbsgpu_record *recs, uint64_t n, uint8_t *dup,
                      pbsgpu_dedup_stats *stats) {
    if (!e || (!recs && n) || !stats || n >= kMaxCount) return PBSGPU_E_INVALID;
    return known_common(e, nullptr, reinterpret_cast<const uint8_t *>(recs), sizeof(pbsgpu_record), false, n, false,
                        dup, stats);
}

// the records are already in device memory (e.g. the output of an RCCL all-gather): no host round trip of the set
int pbsgpu_dedup_device(pbsgpu_engine *e, const void *drecs, uint64_t n, uint8_t *dup, pbsgpu_dedup_stats *stats) {
    if (!e || (!drecs && n) || !stats || n >= kMaxCount) return PBSGPU_E_INVALID;
    if (n && !is_device_pointer(drecs)) return PBSGPU_E_INVALID;
    return known_common(e, nullptr, static_cast<const uint8_t *>(drecs), sizeof(pbsgpu_record), true, n, false, dup,
                        stats);
}

int pbsgpu_known_classify_host(pbsgpu_known *k, const pbsgpu_record *recs, uint64_t n, int insert, uint8_t *known,
                               pbsgpu_dedup_stats *stats) {
    if (!k || (!recs && n) || !stats || n >= kMaxCount) return PBSGPU_E_INVALID;
    return known_common(k->eng, k, reinterpret_cast<const uint8_t *>(recs), sizeof(pbsgpu_record), false, n,
                        insert != 0, known, stats);
}

int pbsgpu_known_classify_device(pbsgpu_known *k, const void *drecs, uint64_t n, int insert, uint8_t *known,
                                 pbsgpu_dedup_stats *stats) {
    if (!k || (!drecs && n) || !stats || n >= kMaxCount) return PBSGPU_E_INVALID;
    if (n && !is_device_pointer(drecs)) return PBSGPU_E_INVALID;
    return known_common(k->eng, k, static_cast<const uint8_t *>(drecs), sizeof(pbsgpu_record), true, n, insert != 0,
                        known, stats);
}

}  // extern "C"
