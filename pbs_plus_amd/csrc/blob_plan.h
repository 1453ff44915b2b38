// The host plans of the aux calls (blob.hip, and what engine.cpp, zstd.hip and zstd_encode.hip share with it): the layout
// of every packed block that goes to or comes back from the device, the piece table of the CRC kernels, and the plan of a
// restore (pbsgpu_blob_decode*_device) — everything such a call decides between its argument checks and its first
// device buffer. Plain C++, no HIP: tests/native/test_blob_plan.cpp runs it under sanitizers.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/pbsgpu.h"

// ---- what the kernels read: layouts are part of the kernels' contract ------------------------------------------------
namespace pbsk {
namespace crc {

constexpr uint32_t kPieceLog = 16;
constexpr uint64_t kPiece = 1ull << kPieceLog;

struct UpHead {  // the first 64 bytes of the block that goes back to the host
    uint64_t stats[4];  // k_known_mark's
    uint64_t total;     // bytes the blobs need
    uint32_t npieces, nparts, nblob;  // what the CRC pair sees (PartPlan::counts): all 0 when total > dst_cap
    uint32_t over;      // total > dst_cap
    uint64_t pad;
};
struct DecInfo {
    uint32_t hk;      // header bytes (12 / 44; 0 = BAD_MAGIC) | kind << 8
    uint32_t stored;  // the header's CRC
};
struct DecStore {  // data bytes [xlo, xhi) of blob u go to dst + dofs + [xlo, xhi) when the data is `size` bytes long
    int64_t dofs;  // the entry's stream start - range_start (may be negative: the bytes in front are clipped)
    uint64_t xlo, xhi;
    uint32_t size;
    uint32_t u;
};
struct DecEntry {
    uint32_t u;  // the entry's blob among the distinct ones
    uint32_t size;
};
static_assert(sizeof(UpHead) == 64 && sizeof(DecInfo) == 8 && sizeof(DecStore) == 32 && sizeof(DecEntry) == 8,
              "read by the kernels of blob.hip");

}  // namespace crc
namespace zstd {

struct RestoreJob {   // one distinct blob: the room its frame is decoded into if it turns out compressed with a good CRC
    uint64_t place;
    uint32_t room, pad;
};
struct RestoreCopy {  // `len` bytes from `from` to `to` when blob u decoded to exactly `size` bytes
    uint64_t from, to;
    uint32_t len, size, u, pad;
};
static_assert(sizeof(RestoreJob) == 16 && sizeof(RestoreCopy) == 32, "read by the kernels of zstd.hip");
constexpr uint32_t kNotDecoded = 0xffu;
constexpr size_t kLitBytes = 128u << 10;  // literal scratch per workgroup of launch_restore_frames
constexpr size_t kDescBytes = 32;         // per distinct blob, device scratch handed to launch_restore_frames

}  // namespace zstd
}  // namespace pbsk

namespace pbsp {

using namespace pbsk::crc;
using pbsk::zstd::RestoreCopy;
using pbsk::zstd::RestoreJob;

// ---- small shared pieces ----------------------------------------------------------------------------------------------

inline bool ranges_ok(const pbsgpu_segment *segs, uint64_t nseg, uint64_t nbytes) {
    for (uint64_t i = 0; i < nseg; ++i)
        if (segs[i].length > nbytes || segs[i].offset > nbytes - segs[i].length) return false;
    return true;
}

// two non-empty byte ranges share a byte
inline bool overlaps(const void *a, uint64_t alen, const void *b, uint64_t blen) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return alen && blen && a0 < b0 + blen && b0 < a0 + alen;
}

// what sha256_dense_pays decides on: the 64-byte blocks of a batch of messages (padding included) and the longest one
struct ShaWork {
    uint64_t total_blocks = 0, longest = 1;
    void add(uint64_t len) {
        const uint64_t blocks = (len + 8) / 64 + 1;
        total_blocks += blocks;
        longest = std::max(longest, blocks);
    }
};

// one blob of `len` bytes (header included) made from a chunk of chunk_len bytes
inline void count_blob(pbsgpu_encode_stats &st, int kind, uint32_t len, uint64_t chunk_len) {
    st.blobs[kind]++;
    st.blob_bytes[kind] += len;
    st.chunk_bytes[kind] += chunk_len;
    if (kind == PBSGPU_BLOB_COMPRESSED) st.frame_bytes += len - PBSGPU_BLOB_HEADER_SIZE;
    st.crc_bytes += len - PBSGPU_BLOB_HEADER_SIZE;
}

// the same for pbsgpu_blob_encode3_device: four kinds, and the plaintext bytes that were encrypted
inline uint32_t header_of(int kind) {
    return kind >= PBSGPU_BLOB_ENCRYPTED ? PBSGPU_BLOB_ENCRYPTED_HEADER_SIZE : PBSGPU_BLOB_HEADER_SIZE;
}
inline void count_blob3(pbsgpu_encode_stats3 &st, int kind, uint32_t len, uint64_t chunk_len) {
    const uint32_t body = len - header_of(kind);
    st.blobs[kind]++;
    st.blob_bytes[kind] += len;
    st.chunk_bytes[kind] += chunk_len;
    if (kind == PBSGPU_BLOB_COMPRESSED || kind == PBSGPU_BLOB_ENCRYPTED_COMPRESSED) st.frame_bytes += body;
    if (kind >= PBSGPU_BLOB_ENCRYPTED) st.aes_bytes += body;
    st.crc_bytes += body;
}

// The slots of an encode call, back to back: slot i = [offsets[i], offsets[i] + header + segs[i].length), offsets[nseg] =
// *total = the bytes dst needs. header = 12 (the plain kinds) or 44 (the encrypted ones); offsets may be nullptr.
// false: the sum does not fit 64 bits.
inline bool slot_offsets(const pbsgpu_segment *segs, uint32_t nseg, uint32_t header, uint64_t *offsets, uint64_t *total) {
    uint64_t at = 0;
    for (uint32_t i = 0; i < nseg; ++i) {
        if (offsets) offsets[i] = at;
        const uint64_t b = segs[i].length + header;
        if (b < segs[i].length || at + b < at) return false;
        at += b;
    }
    if (offsets) offsets[nseg] = at;
    *total = at;
    return true;
}

// no two of the n 16-byte IVs of a call are equal (pbsgpu_blob_encode3_device refuses a call that repeats one: under one
// key a repeated IV gives away the xor of two plaintexts and the hash key). A sort of the IVs as pairs of words.
inline bool ivs_distinct(const uint8_t *ivs, uint32_t n) {
    struct Iv {
        uint64_t a, b;
    };
    std::vector<Iv> v(n);
    for (uint32_t i = 0; i < n; ++i) std::memcpy(&v[i], ivs + 16 * (size_t)i, 16);
    std::sort(v.begin(), v.end(), [](const Iv &x, const Iv &y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
    for (uint32_t i = 1; i < n; ++i)
        if (v[i].a == v[i - 1].a && v[i].b == v[i - 1].b) return false;
    return true;
}

// ---- the piece table ---------------------------------------------------------------------------------------------------
// Every range is cut into pieces of kPiece bytes. pbase[i] = the index of range i's first piece, pbase[n] = the piece
// count; false: 2^32 pieces or more (256 TiB in one call).
inline uint64_t pieces_of(uint64_t len) { return (len + kPiece - 1) >> kPieceLog; }

template <class LenOf>
bool piece_bases(uint64_t n, LenOf len_of, std::vector<uint64_t> &pbase) {
    pbase.resize((size_t)n + 1);
    uint64_t np = 0;
    for (uint64_t i = 0; i < n; ++i) {
        pbase[i] = np;
        np += pieces_of(len_of(i));
    }
    pbase[n] = np;
    return np < (1ull << 32);
}

// owner[p] = the range that piece p belongs to (pbase.back() entries)
inline void fill_owners(const std::vector<uint64_t> &pbase, uint32_t *owner) {
    for (uint32_t i = 0; i + 1 < pbase.size(); ++i)
        for (uint64_t p = pbase[i]; p < pbase[i + 1]; ++p) owner[p] = i;
}

struct PieceTable {
    std::vector<uint64_t> pbase;  // n + 1
    std::vector<uint32_t> owner;  // np
    uint64_t np = 0;
};
template <class LenOf>
bool piece_table(uint64_t n, LenOf len_of, PieceTable &t) {
    if (!piece_bases(n, len_of, t.pbase)) return false;
    t.np = t.pbase[n];
    t.owner.resize((size_t)t.np);
    fill_owners(t.pbase, t.owner.data());
    return true;
}
// the table of an encode call whose blobs' lengths only the device knows (F_ZSTD, F_AES | F_ZSTD): planned for each slot's
// capacity, the chunk's length; a kernel leaves the planned pieces at or beyond the real length's count alone
inline bool capacity_pieces(const pbsgpu_segment *segs, uint32_t nseg, PieceTable &t) {
    return piece_table(nseg, [&](uint64_t i) { return segs[i].length; }, t);
}

// ---- packed blocks ----------------------------------------------------------------------------------------------------
// Several arrays in one device buffer, so that one copy brings them over or back. A block's struct is built once and
// serves both the device pointers and the host's reading of the block. (Members are initialised in declaration order.)
struct Packer {
    size_t total = 0;
    size_t add(size_t bytes, size_t align) {
        const size_t at = (total + align - 1) & ~(align - 1);
        total = at + bytes;
        return at;
    }
};

// upload_new's return block: UpHead | blob_off u64[n] | crcs u32 (compacted: one per new record) | known u8[n] | with
// F_ZSTD: lens u32 | kinds u8 (both compacted)
struct UpBlock {
    Packer p;
    size_t head, boff, crcs, known, lens, kinds, total;
    UpBlock(size_t n, bool zstd)
        : head(p.add(sizeof(UpHead), 8)), boff(p.add(n * 8, 8)), crcs(p.add(n * 4, 4)), known(p.add(n, 1)),
          lens(zstd ? p.add(n * 4, 4) : 0), kinds(zstd ? p.add(n, 1) : 0), total(p.total) {}
};
struct Enc2Block {  // blob_encode_zstd's return block
    Packer p;
    size_t crcs, lens, kinds, total;
    explicit Enc2Block(size_t n) : crcs(p.add(n * 4, 4)), lens(p.add(n * 4, 4)), kinds(p.add(n, 1)), total(p.total) {}
};
using Enc3Block = Enc2Block;  // pbsgpu_blob_encode3_device's return block: the same three arrays
struct DecTables {  // the restore's upload: pbase u64[nu + 1] | prim[nu] | copies[ncopy] | ents[nidx] | pseg u32[np]
    Packer p;
    size_t pbase, prim, copies, ents, pseg, total;
    DecTables(size_t nu, size_t ncopy, size_t nidx, size_t np)
        : pbase(p.add((nu + 1) * 8, 8)), prim(p.add(nu * sizeof(DecStore), 8)), copies(p.add(ncopy * sizeof(DecStore), 8)),
          ents(p.add(nidx * sizeof(DecEntry), 4)), pseg(p.add(np * 4, 4)), total(p.total) {}
};
struct DecBlock {  // the restore's return block: info[nu] | status u8[nidx] | with F_ZSTD: the frames' results u64[nu] | with
    Packer p;      // F_AES: the AES leg's results u64[nu]
    size_t info, status, zres, ares, total;
    DecBlock(size_t nu, size_t nidx, bool zstd, bool aes = false)
        : info(p.add(nu * sizeof(DecInfo), 4)), status(p.add(nidx, 1)), zres(zstd ? p.add(nu * 8, 8) : 0),
          ares(aes ? p.add(nu * 8, 8) : 0), total(p.total) {}
};
struct ZTables {  // the zstd leg's upload: jobs[nu] | copies[ncopy]
    Packer p;
    size_t jobs, copies, total;
    ZTables(size_t nu, size_t ncopy)
        : jobs(p.add(nu * sizeof(RestoreJob), 8)), copies(p.add(ncopy * sizeof(RestoreCopy), 8)), total(p.total) {}
};
struct ZWork {  // its work block: sha ranges[nu] | digests[32 nu] | the hash queue's counter (64 bytes) | frame descriptors[nu]
    Packer p;
    size_t sha, digs, queue, desc, total;
    explicit ZWork(size_t nu)
        : sha(p.add(nu * sizeof(pbsgpu_segment), 8)), digs(p.add(nu * 32, 1)), queue(p.add(64, 4)),
          desc(p.add(nu * pbsk::zstd::kDescBytes, 1)), total(p.total) {}
};

// ---- the restore plan -------------------------------------------------------------------------------------------------
// The distinct referenced blobs, every entry's part of dst, and per blob the entry whose store rides the CRC pass: the
// first one that has bytes inside the range [rs, re). The arguments have passed blob_decode's checks.
struct Restore {
    std::vector<pbsgpu_segment> ub;  // nu distinct blobs, in the order of their first entry
    std::vector<DecEntry> ents;      // nidx
    std::vector<DecStore> prim, copies;
    std::vector<uint64_t> clip;      // nidx: bytes of entry i inside the range
    PieceTable pieces;               // over the data lengths for the 12-byte header
    ShaWork sha;                     // over the same lengths (exact for uncompressed blobs)
    uint64_t longest_copy = 0;
    // with zstd. Which blobs are compressed is known only on the device, so EVERY distinct blob gets a room planned:
    // straight in dst when its first entry inside the range lies wholly inside it and no entry naming the blob is larger,
    // else in scratch with the largest entry's size. Places are offsets from dst; a blob in scratch has its offset INTO
    // THE SCRATCH BUFFER there until place_scratch() adds where that buffer lies.
    std::vector<uint32_t> zmax;      // nu: the largest entry naming the blob
    std::vector<uint8_t> in_scratch; // nu
    std::vector<RestoreJob> jobs;    // nu
    std::vector<RestoreCopy> zcopies;
    uint32_t lit_groups = 0;         // workgroups of launch_restore_frames: kLitBytes each at the scratch buffer's front
    uint64_t scratch_bytes = 0;      // literal buffers included
    uint32_t longest_zcopy = 0;
    ShaWork zsha;                    // over the rooms

    uint32_t nu() const { return (uint32_t)ub.size(); }
    // scratch_minus_dst = the scratch buffer's address - dst's (wrapping)
    void place_scratch(uint64_t scratch_minus_dst) {
        for (uint32_t u = 0; u < nu(); ++u)
            if (in_scratch[u]) jobs[u].place += scratch_minus_dst;
        for (RestoreCopy &c : zcopies)
            if (in_scratch[c.u]) c.from += scratch_minus_dst;
    }
};

// false: 2^32 pieces or more. lit_groups_max: the most workgroups launch_restore_frames is given.
inline bool plan_restore(const pbsgpu_segment *blobs, uint32_t nblob, const pbsgpu_record *idx, uint64_t nidx,
                         const uint32_t *blob_of, uint64_t rs, uint64_t re, bool zstd, uint64_t lit_groups_max, Restore &r) {
    r = Restore{};
    std::vector<uint32_t> uof(nblob, 0xffffffffu);
    r.ents.resize((size_t)nidx);
    r.clip.resize((size_t)nidx);
    for (uint64_t i = 0; i < nidx; ++i) {
        const uint32_t b = blob_of ? blob_of[i] : (uint32_t)i;
        if (uof[b] == 0xffffffffu) {
            uof[b] = (uint32_t)r.ub.size();
            r.ub.push_back(blobs[b]);
            r.prim.push_back(DecStore{0, 0, 0, 0, uof[b]});
        }
        const uint32_t u = uof[b];
        r.ents[i] = DecEntry{u, idx[i].size};
        const uint64_t start = idx[i].end - idx[i].size;
        const uint64_t lo = std::max(start, rs), hi = std::min<uint64_t>(idx[i].end, re);
        r.clip[i] = hi > lo ? hi - lo : 0;
        if (!r.clip[i]) continue;
        const DecStore ds{(int64_t)(start - rs), lo - start, hi - start, idx[i].size, u};
        if (r.prim[u].xlo == r.prim[u].xhi) {
            r.prim[u] = ds;
        } else {
            r.copies.push_back(ds);
            r.longest_copy = std::max(r.longest_copy, ds.xhi - ds.xlo);
        }
    }
    // pieces for the 12-byte header: the data of an encrypted kind is 32 bytes shorter and may leave the first one empty
    const auto data_len = [&](uint64_t u) {
        return r.ub[u].length > PBSGPU_BLOB_HEADER_SIZE ? r.ub[u].length - PBSGPU_BLOB_HEADER_SIZE : 0;
    };
    for (uint32_t u = 0; u < r.nu(); ++u) r.sha.add(data_len(u));
    if (!piece_table(r.nu(), data_len, r.pieces)) return false;
    if (!zstd) return true;
    const uint32_t nu = r.nu();
    r.zmax.assign(nu, 0);
    for (uint64_t i = 0; i < nidx; ++i) r.zmax[r.ents[i].u] = std::max(r.zmax[r.ents[i].u], r.ents[i].size);
    r.lit_groups = (uint32_t)std::min<uint64_t>(nu, lit_groups_max);
    r.scratch_bytes = (uint64_t)r.lit_groups * pbsk::zstd::kLitBytes;
    r.in_scratch.assign(nu, 0);
    r.jobs.assign(nu, RestoreJob{0, 0, 0});
    const auto add_copy = [&](const DecStore &c) {
        r.zcopies.push_back(RestoreCopy{r.jobs[c.u].place + c.xlo, (uint64_t)c.dofs + c.xlo, (uint32_t)(c.xhi - c.xlo), c.size, c.u, 0});
        r.longest_zcopy = std::max(r.longest_zcopy, (uint32_t)(c.xhi - c.xlo));
    };
    for (uint32_t u = 0; u < nu; ++u) {
        const DecStore &ps = r.prim[u];
        const bool direct = ps.xlo < ps.xhi && ps.xlo == 0 && ps.xhi == ps.size && ps.size == r.zmax[u];
        r.jobs[u].room = r.zmax[u];
        r.zsha.add(r.zmax[u]);
        if (direct) {
            r.jobs[u].place = (uint64_t)ps.dofs;
            continue;
        }
        r.in_scratch[u] = 1;
        r.jobs[u].place = r.scratch_bytes;
        r.scratch_bytes += ((uint64_t)r.zmax[u] + 15) & ~15ull;
        if (ps.xlo < ps.xhi) add_copy(ps);
    }
    for (const DecStore &c : r.copies) add_copy(c);
    return true;
}

}  // namespace pbsp
