// AES-256-GCM on the device (pbsgpu_aes_key_*, pbsgpu_aes_gcm_many_device, the AES leg of pbsgpu_blob_decode3_device;
// include/pbsgpu.h).
//
// The cipher and all of GHASH's arithmetic live in aes_gcm.h, once, for these kernels and for the CPU build that runs under
// sanitizers. This file adds the cooperation between lanes and the launches:
//   k_aes_head    per message, one lane: J0 from the IV (two plain multiplies for 16 bytes) and E_K(J0).
//   k_aes_pieces  per piece of 64 KiB, one workgroup of 256: pbsa::piece_lane on every lane (CTR over interleaved blocks,
//                 Horner with H^256 through the table), then the xor over the lanes: the piece's partial hash. The AES table,
//                 the multiplier table of H^256 and the reduction table are copied from the key to LDS per workgroup
//                 (6 KiB + the four words per wave of the reduction).
//   k_aes_fold    per message, one wave: lane l folds pieces l, l + 64, ... (partial times H^(blocks behind + 1)), the xor
//                 over the lanes, the length block, E_K(J0); the tag is written (encrypt) or compared without an early exit.
//   k_aes_zero    per message whose tag was bad: its output is zeroed. It looks at the statuses the fold left on the device;
//                 with all tags good every workgroup reads one byte per message and ends.
// and for the restore, where only the device knows which blobs are encrypted:
//   k_aesr_select per distinct blob: an encrypted blob with a good CRC becomes a message (IV and tag where the blob has them)
//   k_aesr_frames per distinct blob, behind the verdicts: the plaintext of an encrypted-compressed blob becomes a frame for
//                 k_zstd_frames (zstd.hip); every other blob's result is final
//   k_aesr_merge  per distinct blob, behind the frames: one result word for the host and one for the copy pass; with an id
//                 key (pbsgpu_blob_decode4_device) also the range of plaintext that the keyed SHA-256 pass hashes
//   k_aesr_status per entry of a blob the leg handled: tag, frame, size, and with an id key the keyed digest
// Memory instructions: global_* and ds_* only, no scratch (tests/test_aes_surface.py). Every pointer a kernel dereferences
// comes from its arguments.
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "aes_gcm.h"
#include "zstd_frames.h"

using namespace pbse;

struct pbsgpu_aes_key {
    pbsgpu_engine *eng = nullptr;
    DevBuf tables;  // one pbsa::KeyTables: the only copy of the key material once create has returned
};

namespace pbsk {
namespace aes {

using pbsa::Blk;
using pbsa::KeyTables;

enum : uint32_t { M_ACTIVE = 1, M_STORE = 2, M_FRAME = 4 };  // Msg::mode
constexpr uint8_t kIdle = 0xff;                              // the status of a message that is not M_ACTIVE

struct Msg {  // one message of a call
    uint64_t src_off, dst_off;  // the ciphertext (plaintext when encrypting) in src, the output in dst
    uint64_t iv_off, tag_off;   // in the call's IV and tag bytes
    uint32_t len;
    uint32_t first;  // its first piece in the call's piece space
    uint32_t mode, pad;
};
struct PieceRef {
    uint32_t msg, piece;
};
struct Batch {  // what the four kernels share
    const KeyTables *kt;
    const uint8_t *src, *ivs;
    uint8_t *dst, *tags;  // tags: read when decrypting, written when encrypting
    const Msg *msgs;
    const PieceRef *refs;
    Blk *heads, *partials;
    uint8_t *status;  // per message
    uint32_t nmsg, npieces, iv_len, encrypt;
};

__device__ __forceinline__ Blk wave_xor(Blk v) {
    for (int d = 32; d; d >>= 1)
        for (int k = 0; k < 4; ++k) v.w[k] ^= (uint32_t)__shfl_xor((int)v.w[k], d, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_aes_head(const KeyTables *kt, const uint8_t *ivs, const Msg *msgs, uint32_t iv_len, uint32_t n,
                                                  Blk *heads) {
    __shared__ uint32_t te0[256];
    te0[threadIdx.x] = kt->te0[threadIdx.x];
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t mode = msgs[i].mode;
    if (!(mode & M_ACTIVE)) return;
    const Blk j0 = pbsa::j0_of(kt->h, ivs + msgs[i].iv_off, iv_len);
    heads[2 * i] = j0;
    heads[2 * i + 1] = pbsa::encrypt_block(kt->rk, te0, j0);
}

__global__ __launch_bounds__(256) void k_aes_pieces(const KeyTables *kt, const uint8_t *src, uint8_t *dst, const Msg *msgs,
                                                    const PieceRef *refs, uint32_t npieces, const Blk *heads, Blk *partials,
                                                    uint32_t encrypt) {
    static_assert(pbsa::kStride == 256, "one lane of the piece per thread");
    __shared__ uint32_t te0[256];
    __shared__ uint32_t red[256];
    __shared__ Blk stride[256];
    __shared__ Blk box[4];
    te0[threadIdx.x] = kt->te0[threadIdx.x];
    red[threadIdx.x] = kt->red[threadIdx.x];
    stride[threadIdx.x] = kt->stride[threadIdx.x];
    __syncthreads();
    for (uint32_t p = blockIdx.x; p < npieces; p += gridDim.x) {
        const PieceRef ref = refs[p];
        const Msg m = msgs[ref.msg];
        if (!(m.mode & M_ACTIVE)) continue;  // (the workgroup's: one piece, one message)
        const uint64_t at = (uint64_t)ref.piece * pbsa::kPiece;
        Blk y = pbsa::piece_lane(kt->rk, te0, stride, red, kt->low, heads[2 * ref.msg], ref.piece, src + m.src_off + at,
                                 dst + m.dst_off + at, pbsa::piece_len(m.len, ref.piece), encrypt != 0, threadIdx.x,
                                 (m.mode & M_STORE) != 0);
        y = wave_xor(y);
        if ((threadIdx.x & 63u) == 0) box[threadIdx.x >> 6] = y;
        __syncthreads();
        if (threadIdx.x == 0) partials[p] = pbsa::bxor(pbsa::bxor(box[0], box[1]), pbsa::bxor(box[2], box[3]));
        __syncthreads();  // the box goes to the next piece
    }
}

__global__ __launch_bounds__(64) void k_aes_fold(const KeyTables *kt, const Msg *msgs, uint32_t nmsg, const Blk *heads,
                                                 const Blk *partials, uint8_t *tags, uint8_t *status, uint32_t encrypt) {
    for (uint32_t i = blockIdx.x; i < nmsg; i += gridDim.x) {
        const Msg m = msgs[i];
        if (!(m.mode & M_ACTIVE)) {
            if (threadIdx.x == 0) status[i] = kIdle;
            continue;
        }
        const uint32_t np = pbsa::pieces_of(m.len);
        Blk terms{{0, 0, 0, 0}};
        for (uint32_t p = threadIdx.x; p < np; p += 64) terms = pbsa::bxor(terms, pbsa::fold_piece(partials[m.first + p], m.len, p, kt->pow2));
        terms = wave_xor(terms);
        if (threadIdx.x == 0) {
            const Blk t = pbsa::tag_of(terms, m.len, kt->h, heads[2 * i + 1]);
            if (encrypt) {
                pbsa::store_be(tags + m.tag_off, t);
                status[i] = pbsa::OK;
            } else {
                status[i] = (uint8_t)pbsa::tag_verdict(t, pbsa::load_be(tags + m.tag_off));
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_aes_zero(const Msg *msgs, uint32_t nmsg, const uint8_t *status, uint8_t *dst) {
    for (uint32_t i = blockIdx.y; i < nmsg; i += gridDim.y) {
        if (status[i] != pbsa::BAD_TAG) continue;  // (the workgroup's: one message, one verdict)
        const Msg m = msgs[i];
        if (!(m.mode & M_STORE)) continue;
        uint8_t *o = dst + m.dst_off;
        for (uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x; b < m.len; b += (uint64_t)gridDim.x * 256u) o[b] = 0;
    }
}

// head, pieces, fold and, when decrypting, zero: enqueued, nothing synchronised
static int enqueue_batch(const Batch &b, uint32_t longest, int num_cus, hipStream_t st) {
    hipLaunchKernelGGL(k_aes_head, dim3((b.nmsg + 255) / 256), dim3(256), 0, st, b.kt, b.ivs, b.msgs, b.iv_len, b.nmsg, b.heads);
    HIPCHK(hipGetLastError());
    if (b.npieces) {
        const uint32_t grid = (uint32_t)std::min<uint64_t>(b.npieces, (uint64_t)num_cus * 8);
        hipLaunchKernelGGL(k_aes_pieces, dim3(grid), dim3(256), 0, st, b.kt, b.src, b.dst, b.msgs, b.refs, b.npieces, b.heads,
                           b.partials, b.encrypt);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_aes_fold, dim3(std::min<uint32_t>(b.nmsg, (uint32_t)num_cus * 16)), dim3(64), 0, st, b.kt, b.msgs, b.nmsg,
                       b.heads, b.partials, b.tags, b.status, b.encrypt);
    HIPCHK(hipGetLastError());
    if (!b.encrypt && longest) {
        const uint32_t gx = std::max<uint32_t>(1, std::min<uint32_t>((longest + 65535) / 65536, 64));
        hipLaunchKernelGGL(k_aes_zero, dim3(gx, std::min<uint32_t>(b.nmsg, 1024)), dim3(256), 0, st, b.msgs, b.nmsg, b.status, b.dst);
        HIPCHK(hipGetLastError());
    }
    return PBSGPU_OK;
}

// ---- the AES leg of the restore (pbsgpu_blob_decode3_device; planned and enqueued by blob.hip) ---------------------------
// Result words, status << 32 | bytes. res (for the host and k_aesr_status): kNotDecoded = the leg left the blob alone,
// R_BAD_TAG, else a PBSGPU_ZSTD_* status, with R_FRAME set when the plaintext was a frame that went to the decoder. fin (for
// launch_restore_copy, which copies when fin == the entry's size): OK << 32 | bytes, or kNotDecoded << 32.
enum : uint32_t { R_BAD_TAG = 0xfe, R_FRAME = 0x80 };
static_assert(R_BAD_TAG == kResBadTag && R_FRAME == kResFrame, "what blob.hip reads the leg's results with");
constexpr uint32_t kEncHdr = PBSGPU_BLOB_ENCRYPTED_HEADER_SIZE;

struct Leg {
    pbsk::zstd::RestorePlan zp;  // src, blobs, info, crcs, jobs, ents, status, dst
    const uint64_t *aplace;      // nu: where an encrypted-compressed blob's plaintext goes, an offset from dst (into scratch)
    const uint32_t *pfirst;      // nu: the blob's first piece
    Msg *msgs;                   // nu
    const uint8_t *verdict;      // nu: the fold's statuses
    pbsk::zstd::Desc *desc;      // nu
    uint64_t *zres;              // nu: the frames' results
    uint64_t *res, *fin;         // nu each
    pbsgpu_segment *ksha;        // nu, with an id key: what the keyed SHA-256 pass hashes, relative to dst
    const uint8_t *kdigs;        // nu * 32: SHA-256(plaintext || id_key); nullptr: no id key, the digest is not checked
    uint32_t zstd;
};

__global__ __launch_bounds__(256) void k_aesr_select(Leg lg) {
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    if (u >= lg.zp.nu) return;
    const uint32_t hk = lg.zp.info[2 * (uint64_t)u], stored = lg.zp.info[2 * (uint64_t)u + 1];
    const uint32_t kind = hk >> 8;
    const bool enc = (hk & 255u) == kEncHdr && lg.zp.crcs[u] == stored &&
                     (kind == PBSGPU_BLOB_ENCRYPTED || (kind == PBSGPU_BLOB_ENCRYPTED_COMPRESSED && lg.zstd));
    const pbsgpu_segment b = lg.zp.blobs[u];
    const pbsk::zstd::RestoreJob job = lg.zp.jobs[u];
    Msg m{};
    m.first = lg.pfirst[u];
    if (enc) {
        m.src_off = b.offset + kEncHdr;
        m.iv_off = b.offset + PBSGPU_BLOB_HEADER_SIZE;
        m.tag_off = b.offset + PBSGPU_BLOB_HEADER_SIZE + 16;
        m.len = (uint32_t)(b.length - kEncHdr);
        if (kind == PBSGPU_BLOB_ENCRYPTED_COMPRESSED) {
            m.dst_off = lg.aplace[u];
            m.mode = M_ACTIVE | M_STORE | M_FRAME;
        } else {  // to its place in the stream if it fits the largest entry that names it; its tag is checked either way
            m.dst_off = job.place;
            m.mode = m.len <= job.room ? (M_ACTIVE | M_STORE) : M_ACTIVE;
        }
    }
    lg.msgs[u] = m;
}

__global__ __launch_bounds__(256) void k_aesr_frames(Leg lg) {
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    if (u >= lg.zp.nu) return;
    const Msg m = lg.msgs[u];
    const bool frame = (m.mode & M_FRAME) && lg.verdict[u] == pbsa::OK;
    const pbsk::zstd::RestoreJob job = lg.zp.jobs[u];
    // (both places are offsets from dst: the frames' launch takes dst for its source as well)
    lg.desc[u] = pbsk::zstd::Desc{m.dst_off, frame ? (uint64_t)m.len : pbsk::zstd::kSkip, job.place, job.room};
}

__global__ __launch_bounds__(256) void k_aesr_merge(Leg lg) {
    const uint32_t u = blockIdx.x * 256 + threadIdx.x;
    if (u >= lg.zp.nu) return;
    const Msg m = lg.msgs[u];
    const uint64_t idle = (uint64_t)pbsk::zstd::kNotDecoded << 32;
    uint64_t res = idle, fin = idle;
    if (m.mode & M_ACTIVE) {
        if (lg.verdict[u] != pbsa::OK) {
            res = (uint64_t)R_BAD_TAG << 32;
        } else if (m.mode & M_FRAME) {
            const uint64_t z = lg.zres[u];
            res = z | (uint64_t)R_FRAME << 32;
            if ((z >> 32) == PBSGPU_ZSTD_OK) fin = z;
        } else if (m.mode & M_STORE) {
            res = fin = (uint64_t)PBSGPU_ZSTD_OK << 32 | m.len;
        } else {
            res = (uint64_t)PBSGPU_ZSTD_BAD_SIZE << 32;
        }
    }
    lg.res[u] = res;
    lg.fin[u] = fin;
    // with an id key: the plaintext of a blob the leg restored lies at its job's place, whichever way it got there (decrypted
    // in place, or decoded from its frame). That and the result's length is what the keyed SHA-256 pass hashes, as
    // k_zr_ranges has it for the zstd leg; an empty range for every other blob
    if (lg.ksha) lg.ksha[u] = pbsgpu_segment{lg.zp.jobs[u].place, (fin >> 32) == PBSGPU_ZSTD_OK ? (uint32_t)fin : 0u};
}

typedef const __attribute__((address_space(1))) uint32_t *aword_ptr;

__global__ __launch_bounds__(256) void k_aesr_status(Leg lg) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= lg.zp.nidx) return;
    const uint32_t u = lg.zp.ents[2 * (uint64_t)i], size = lg.zp.ents[2 * (uint64_t)i + 1];
    const uint64_t res = lg.res[u];
    const uint32_t code = (uint32_t)(res >> 32);
    if (code == pbsk::zstd::kNotDecoded) return;  // blob.hip's status stands, or the zstd leg's
    const uint32_t zs = code & ~(uint32_t)R_FRAME;
    uint8_t r;
    if (code == R_BAD_TAG) {
        r = PBSGPU_BLOB_BAD_TAG;
    } else if (zs == PBSGPU_ZSTD_BAD_FRAME || zs == PBSGPU_ZSTD_UNSUPPORTED) {
        r = PBSGPU_BLOB_BAD_DATA;
    } else if (zs != PBSGPU_ZSTD_OK || (uint32_t)res != size) {
        r = PBSGPU_BLOB_BAD_SIZE;
    } else {
        r = PBSGPU_BLOB_OK;  // (no digest: an encrypted chunk's index digest is keyed, and the tag has vouched for the content)
        if (lg.kdigs) {      // ... unless the call has the id key: the keyed digest of the plaintext against the record's
            const aword_ptr want = (aword_ptr)(lg.zp.recs + 48ull * i + 8), got = (aword_ptr)(lg.kdigs + 32ull * u);
            uint32_t diff = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) diff |= want[j] ^ got[j];
            if (diff) r = PBSGPU_BLOB_BAD_DIGEST;
        }
    }
    lg.zp.status[i] = r;
}

int enqueue_restore(pbsgpu_engine *e, Slot *s, const pbsgpu_aes_key *key, const pbsk::zstd::RestorePlan &zp,
                    const pbsgpu_segment *ub, bool zstd, uint32_t longest_copy, uint64_t *res, const uint32_t *idkey,
                    const pbsp::ShaWork *sha) {
    const uint32_t nu = zp.nu;
    const bool keyed = idkey && zp.recs && sha;
    // what the host can know: every distinct blob might be encrypted, so each gets its pieces and, with zstd, room for a
    // plaintext frame in scratch
    std::vector<uint32_t> pfirst(nu);
    std::vector<uint64_t> aplace(nu, 0);
    std::vector<PieceRef> refs;
    uint64_t scratch = 0;
    uint32_t longest = 0;
    for (uint32_t u = 0; u < nu; ++u) {
        const uint32_t len = ub[u].length > kEncHdr ? (uint32_t)(ub[u].length - kEncHdr) : 0;
        pfirst[u] = (uint32_t)refs.size();
        for (uint32_t p = 0; p < pbsa::pieces_of(len); ++p) refs.push_back(PieceRef{u, p});
        aplace[u] = scratch;
        if (zstd) scratch += ((uint64_t)len + 15) & ~15ull;
        longest = std::max(longest, len);
    }
    if (refs.size() >> 32) return PBSGPU_E_INVALID;
    uint8_t *plain = s->bulk((size_t)scratch + 16);
    CHK(s->taken());
    for (uint32_t u = 0; u < nu; ++u) aplace[u] += (uint64_t)((uintptr_t)plain - (uintptr_t)zp.dst);
    Leg lg{};
    lg.zp = zp;
    lg.zstd = zstd ? 1u : 0u;
    const PieceRef *drefs = nullptr;
    CHK(put_table(s, aplace.data(), nu, &lg.aplace));
    CHK(put_table(s, pfirst.data(), nu, &lg.pfirst));
    CHK(put_table(s, refs.data(), refs.size(), &drefs));
    lg.msgs = s->take<Msg>(nu);
    uint8_t *verdict = s->take<uint8_t>(nu);
    lg.desc = s->take<pbsk::zstd::Desc>(nu);
    lg.zres = s->take<uint64_t>(nu);
    lg.fin = s->take<uint64_t>(nu);
    Blk *heads = s->take<Blk>((size_t)nu * 2);
    Blk *partials = s->take<Blk>(refs.size() + 1);
    uint8_t *kdigs = keyed ? s->take<uint8_t>((size_t)nu * 32) : nullptr;
    uint32_t *kqueue = keyed ? s->take<uint32_t>(16) : nullptr;
    lg.ksha = keyed ? s->take<pbsgpu_segment>(nu) : nullptr;
    CHK(s->taken());
    lg.kdigs = kdigs;
    lg.verdict = verdict;
    lg.res = res;
    const dim3 per_blob((nu + 255) / 256);
    hipLaunchKernelGGL(k_aesr_select, per_blob, dim3(256), 0, s->stream, lg);
    HIPCHK(hipGetLastError());
    Batch b{};
    b.kt = key->tables.as<const KeyTables>();
    b.src = b.ivs = zp.src;
    b.tags = const_cast<uint8_t *>(zp.src);  // (decrypting: read only)
    b.dst = zp.dst;
    b.msgs = lg.msgs;
    b.refs = drefs;
    b.heads = heads;
    b.partials = partials;
    b.status = verdict;
    b.nmsg = nu;
    b.npieces = (uint32_t)refs.size();
    b.iv_len = 16;
    b.encrypt = 0;
    CHK(enqueue_batch(b, longest, e->num_cus, s->stream));
    hipLaunchKernelGGL(k_aesr_frames, per_blob, dim3(256), 0, s->stream, lg);
    HIPCHK(hipGetLastError());
    if (zstd) {
        pbsk::zstd::Plan fp{};
        fp.src = zp.dst;
        fp.desc = lg.desc;
        fp.dst = zp.dst;
        fp.lit = zp.lit;
        fp.res = lg.zres;
        fp.nframe = nu;
        fp.stride = zp.stride;
        HIPCHK(pbsk::zstd::launch_frames(fp, s->stream));
    }
    hipLaunchKernelGGL(k_aesr_merge, per_blob, dim3(256), 0, s->stream, lg);
    HIPCHK(hipGetLastError());
    if (zp.ncopy) {
        pbsk::zstd::RestorePlan cp = zp;
        cp.res = lg.fin;
        HIPCHK(pbsk::zstd::launch_restore_copy(cp, longest_copy, e->num_cus, s->stream));
    }
    if (keyed) {  // once per distinct blob, over the plaintext where the leg left it; the copies above only read it
        HIPCHK(hipMemsetAsync(kqueue, 0, 64, s->stream));
        CHK(enqueue_sha256(e, s->stream, zp.dst, lg.ksha, nu, kdigs, kqueue, *sha, idkey));
    }
    hipLaunchKernelGGL(k_aesr_status, dim3((zp.nidx + 255) / 256), dim3(256), 0, s->stream, lg);
    HIPCHK(hipGetLastError());
    return PBSGPU_OK;
}

pbsgpu_engine *key_engine(const pbsgpu_aes_key *k) { return k->eng; }
const void *key_tables(const pbsgpu_aes_key *k) { return k->tables.p; }

}  // namespace aes
}  // namespace pbsk

namespace {

void wipe(void *p, size_t n) {  // a memset the optimiser may not drop
    volatile uint8_t *v = static_cast<volatile uint8_t *>(p);
    for (size_t i = 0; i < n; ++i) v[i] = 0;
}

}  // namespace

extern "C" {

int pbsgpu_aes_key_create(pbsgpu_engine *e, const uint8_t *key, pbsgpu_aes_key **out) {
    if (!e || !key || !out) return PBSGPU_E_INVALID;
    *out = nullptr;
    CHK(set_device(e));
    pbsgpu_aes_key *k = new (std::nothrow) pbsgpu_aes_key();
    pbsa::KeyTables *kt = new (std::nothrow) pbsa::KeyTables();
    int st = k && kt ? k->tables.ensure(sizeof(pbsa::KeyTables)) : PBSGPU_E_NOMEM;
    if (st == PBSGPU_OK) {
        pbsa::make_key(key, *kt);
        // straight from this block, not through a slot's pinned staging: no second copy of the key outlives the call
        if (hipMemcpy(k->tables.p, kt, sizeof(*kt), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            st = PBSGPU_E_HIP;
        }
    }
    if (kt) wipe(kt, sizeof(*kt));
    delete kt;
    if (st != PBSGPU_OK) {
        if (k) k->tables.release();
        delete k;
        return st;
    }
    engine_ref(e);
    k->eng = e;
    *out = k;
    return PBSGPU_OK;
}

void pbsgpu_aes_key_destroy(pbsgpu_aes_key *k) {
    if (!k) return;
    pbsgpu_engine *e = k->eng;
    if (e) (void)set_device(e);
    if (k->tables.p) {
        AuxLease lease(e);  // (calls that use the key hold a lease until they have synchronised: none is running on it now)
        if (hipMemsetAsync(k->tables.p, 0, sizeof(pbsa::KeyTables), lease.s->stream) != hipSuccess ||
            hipStreamSynchronize(lease.s->stream) != hipSuccess)
            (void)hipGetLastError();
    }
    k->tables.release();
    delete k;
    if (e) engine_unref(e);
}

int pbsgpu_aes_gcm_many_device(pbsgpu_aes_key *k, const void *src, uint64_t nbytes, const pbsgpu_segment *msgs, uint32_t nmsg,
                               const uint8_t *ivs, uint32_t iv_len, uint8_t *tags, const pbsgpu_segment *out, void *dst,
                               uint64_t dst_cap, uint8_t *status, uint32_t flags) {
    using namespace pbsk::aes;
    if (!k || (flags & ~(uint32_t)PBSGPU_AES_F_ENCRYPT) || (iv_len != 12 && iv_len != 16)) return PBSGPU_E_INVALID;
    if (nmsg == 0) return PBSGPU_OK;
    if (!msgs || !ivs || !tags || !out || !status || (!src && nbytes) || (!dst && dst_cap)) return PBSGPU_E_INVALID;
    uint64_t lo = ~0ull, hi = 0, npieces = 0;  // lo, hi: the part of dst the call may write
    for (uint32_t i = 0; i < nmsg; ++i) {
        if ((msgs[i].length | out[i].length) >> 32) return PBSGPU_E_INVALID;
        if (msgs[i].length > nbytes || msgs[i].offset > nbytes - msgs[i].length) return PBSGPU_E_INVALID;
        if (out[i].length > dst_cap || out[i].offset > dst_cap - out[i].length) return PBSGPU_E_INVALID;
        if (out[i].length < msgs[i].length) return PBSGPU_E_INVALID;  // the output is as long as the input: no room, no call
        if (out[i].length) {
            lo = std::min(lo, out[i].offset);
            hi = std::max(hi, out[i].offset + out[i].length);
        }
        npieces += pbsa::pieces_of((uint32_t)msgs[i].length);
    }
    if (npieces >> 32) return PBSGPU_E_INVALID;
    std::vector<uint32_t> order;
    for (uint32_t i = 0; i < nmsg; ++i)
        if (out[i].length) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return out[a].offset < out[b].offset; });
    for (size_t j = 1; j < order.size(); ++j)
        if (out[order[j - 1]].offset + out[order[j - 1]].length > out[order[j]].offset) return PBSGPU_E_INVALID;
    if (hi > lo && pbsp::overlaps(static_cast<const uint8_t *>(dst) + lo, hi - lo, src, nbytes)) return PBSGPU_E_INVALID;
    pbsgpu_engine *e = k->eng;
    CHK(set_device(e));
    if ((nbytes && !is_device_pointer(src)) || (hi > lo && !is_device_pointer(dst))) return PBSGPU_E_INVALID;
    const bool encrypt = (flags & PBSGPU_AES_F_ENCRYPT) != 0;
    AuxLease lease(e);
    Slot *s = lease.s;
    std::vector<Msg> hm(nmsg);
    std::vector<PieceRef> hr;
    hr.reserve((size_t)npieces);
    uint32_t longest = 0;
    for (uint32_t i = 0; i < nmsg; ++i) {
        hm[i] = Msg{msgs[i].offset, out[i].offset, (uint64_t)i * iv_len, 16ull * i, (uint32_t)msgs[i].length, (uint32_t)hr.size(),
                    M_ACTIVE | M_STORE, 0};
        for (uint32_t p = 0; p < pbsa::pieces_of(hm[i].len); ++p) hr.push_back(PieceRef{i, p});
        longest = std::max(longest, hm[i].len);
    }
    Batch b{};
    CHK(put_table(s, hm.data(), nmsg, &b.msgs));
    CHK(put_table(s, hr.data(), hr.size(), &b.refs));
    CHK(put_table(s, ivs, (size_t)nmsg * iv_len, &b.ivs));
    b.heads = s->take<Blk>((size_t)nmsg * 2);
    b.partials = s->take<Blk>(hr.size() + 1);
    uint8_t *res = s->take<uint8_t>((size_t)nmsg * 17);  // the tags, then the statuses: what goes back
    CHK(s->taken());
    if (!encrypt) CHK(staged_h2d(*s, res, tags, (size_t)nmsg * 16, s->stream));
    b.kt = k->tables.as<const KeyTables>();
    b.src = static_cast<const uint8_t *>(src);
    b.dst = static_cast<uint8_t *>(dst);
    b.tags = res;
    b.status = res + (size_t)nmsg * 16;
    b.nmsg = nmsg;
    b.npieces = (uint32_t)hr.size();
    b.iv_len = iv_len;
    b.encrypt = encrypt ? 1u : 0u;
    CHK(enqueue_batch(b, longest, e->num_cus, s->stream));
    std::vector<uint8_t> back((size_t)nmsg * 17);
    CHK(fetch_result(s, back.data(), res, back.size()));  // the call's one synchronisation
    if (encrypt) std::memcpy(tags, back.data(), (size_t)nmsg * 16);
    std::memcpy(status, back.data() + (size_t)nmsg * 16, nmsg);
    return PBSGPU_OK;
}

}  // extern "C"
