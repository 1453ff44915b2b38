// Internal declarations shared by the libpbsgpu translation units (not part of the C ABI).
//
// Concurrency model (cgo calls arrive on arbitrary OS threads, several goroutines may share one engine):
//   * pbsgpu_engine::mu guards only bookkeeping — which pool slot is free, the ticket table, the aux leases, the
//     child count. It is NEVER held across a HIP synchronisation, a memcpy or a kernel enqueue.
//   * a Slot (device work context: HIP stream, events, work buffers, pinned staging) is owned by exactly one
//     logical user at a time: a batch ticket (pool slots), one synchronous helper call (aux slots, leased; callers
//     WAIT for a lease instead of failing), or one stream / chunker handle (private slot, never shared).
//   * Slot::op serialises concurrent operations on the same ticket (wait / collect / timing from two threads).
//   * streaming writers (pbsgpu_stream_*) are clients of ONE engine-owned page ring (ring_internal.h; own mutex): pages,
//     cut rounds, the persistent SHA-256 service and record delivery are shared by all streams of the engine.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "blob_plan.h"
#include "kernels.h"
#include "zstd_plan.h"

namespace pbse {

extern std::atomic<int> g_last_hip_error;

#define HIPCHK(expr)                                   \
    do {                                               \
        hipError_t _e = (expr);                        \
        if (_e != hipSuccess) {                        \
            pbse::g_last_hip_error.store((int)_e);     \
            return PBSGPU_E_HIP;                       \
        }                                              \
    } while (0)

#define CHK(expr)                       \
    do {                                \
        int _s = (expr);                \
        if (_s != PBSGPU_OK) return _s; \
    } while (0)

// hipFree / hipHostFree wait for the WHOLE device — including a page ring's persistent SHA-256 service, which only ends
// on request: a free issued while a service runs would block until someone stops it (for ever, if the caller is the
// thread that would). Every release in this library therefore goes through dev_free / host_free: while a service runs ON
// THE DEVICE THE MEMORY BELONGS TO the pointer is parked in that device's graveyard and really freed when the device's last
// service has stopped (ring.cpp: quiesce / park / the service's own stop); a device without a running service frees at once
// (round 5: services and graveyard are tracked per device — a service on GPU 0 no longer parks the frees of GPU 1).
// Parked DEVICE bytes are bounded: beyond the cap (an eighth of the device's memory, PBSGPU_GRAVEYARD_MIB) the device's
// rings are asked to park their services (service_park_generation, honoured once per request by the next pump), the last one to end frees
// everything and the services start again with the next round.
void service_started(int device);     // a page-ring service is about to be launched (waits for a flush in progress)
void service_ended(int device);       // ... is known to have ended; frees the device's parked memory when it was the last
int services_running(int device);
uint32_t service_park_generation(int device);  // 0 = no request pending, else the number of the pending request
void dev_free(void *p);
void host_free(void *p);

// growable device buffer
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    int ensure(size_t bytes) {
        if (bytes <= cap) return PBSGPU_OK;
        if (p) {
            dev_free(p);  // device-wide wait: see PinnedBuf::ensure
            p = nullptr;
            bytes = std::max(bytes, std::min<size_t>(cap * 2, cap + (256u << 20)));
            cap = 0;
        }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            want = bytes;
            e = hipMalloc(&p, want);
        }
        if (e != hipSuccess) {
            g_last_hip_error.store((int)e);
            (void)hipGetLastError();
            p = nullptr;
            return PBSGPU_E_NOMEM;
        }
        cap = want;
        return PBSGPU_OK;
    }
    void release() {
        if (p) dev_free(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

struct PinnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    PinnedBuf(PinnedBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    // NOTE: hipHostFree / hipFree wait for the whole device to go idle — a regrow while another stream's 0.4 s SHA
    // launch is running stalls the caller that long (measured on the streaming writer). Hot paths therefore size their
    // buffers once for the largest case (ensure_once / presize) and growth doubles.
    int ensure(size_t bytes) {
        if (bytes <= cap) return PBSGPU_OK;
        if (p) {
            host_free(p);
            bytes = std::max(bytes, cap * 2);
        }
        p = nullptr;
        cap = 0;
        hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (e != hipSuccess) {
            g_last_hip_error.store((int)e);
            (void)hipGetLastError();
            p = nullptr;
            return PBSGPU_E_NOMEM;
        }
        cap = bytes;
        return PBSGPU_OK;
    }
    void release() {
        if (p) host_free(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T> T *as() const { return reinterpret_cast<T *>(p); }
};

// Device scratch of one synchronous helper call (an AuxLease): buffers handed out in call order, each take a DevBuf of its
// own, so a later take never moves an earlier one that an enqueued kernel still reads. Every buffer has 64 bytes of slack
// behind what was asked for (the kernels' 16-byte loads may touch them). The cursor goes back to 0 with the next lease; the
// buffers stay and grow by DevBuf::ensure's policy.
struct Scratch {
    std::vector<DevBuf> bufs;
    size_t next = 0;
    void *take(size_t bytes, int *status);  // nullptr and *status = PBSGPU_E_NOMEM when the device has no room
    void release();
};

// device scalars of one slot (uint32 each)
enum : int { SC_NCAND = 0, SC_NREC = 1, SC_MAXCNT = 2, SC_QUEUE = 3, SC_WGLIMIT = 4, SC_ZERO = 5 /* stays 0 */,
             SC_TILEQ = 6 /* u64 */, SC_PARFB = 8 /* parallel resolve handed the job back */, SC_PARHOPS = 9, SC_COUNT = 10 };

enum : int { EV_BEGIN = 0, EV_SCAN0, EV_SCAN1, EV_RESOLVE1, EV_SHA1, EV_COUNT };

constexpr size_t kStageBytes = 32u << 20;

struct Slot {
    hipStream_t stream = nullptr;
    bool own_stream = true;  // false: the stream belongs to a sibling context (a payload stream's second cut context)
    hipEvent_t ev[EV_COUNT] = {};
    DevBuf data;  // staged copy of host submits
    DevBuf tile_cnt, tile_off, tile_slots, dense, scan_tmp, scalars, segs, seg_cnt, seg_off, recs, order;
    DevBuf sugg, sugg_idx;  // suggested boundaries (optional)
    DevBuf par;             // scratch of the parallel single-stream resolve (doubling tables)
    // aux slots: what a helper call needs beyond the staged ranges. take() serves tables and result blocks, bulk() the few
    // large byte buffers (the encoder's block output and work area, the decoders' literal and scratch area), which so
    // only ever share positions with each other. A failed take is remembered: CHK(taken()) behind a call's takes.
    Scratch tables, large;
    int scratch_status = PBSGPU_OK;
    template <typename T> T *take(size_t count) { return static_cast<T *>(tables.take(count * sizeof(T), &scratch_status)); }
    uint8_t *bulk(size_t bytes) { return static_cast<uint8_t *>(large.take(bytes, &scratch_status)); }
    int taken() const { return scratch_status; }
    PinnedBuf h_scalars;    // readback of SC_*
    PinnedBuf h_segs;       // pinned copy of the segment table
    PinnedBuf h_sugg;       // pinned copy of suggested offsets + index
    PinnedBuf h_recs;       // mapped pinned copy of the finished records (published by kernel, not by the copy engine)
    bool recs_published = false;
    PinnedBuf stage[2];     // host -> device staging of this slot (lazily allocated)
    hipEvent_t stage_ev[2] = {};
    // Control tables (segment table, suggested boundaries) are either copied to the device (batch tickets: thousands
    // of segments read by many waves) or, for the streaming writers, READ BY THE KERNELS STRAIGHT FROM the mapped pinned
    // copies: a small H2D copy would queue behind the megabytes of payload pieces in the shared SDMA queues.
    bool mapped_ctrl = false;
    const pbsgpu_segment *segs_dev() const {
        return mapped_ctrl ? h_segs.as<pbsgpu_segment>() : segs.as<pbsgpu_segment>();
    }
    std::mutex op;          // serialises operations on the ticket that owns this slot
    // in-flight state (owner only)
    bool busy = false;      // under engine mu
    bool ready = false;     // ticket published (under engine mu)
    bool synced = false;
    uint64_t ticket = 0;
    const uint8_t *dptr = nullptr;
    uint64_t nbytes = 0;
    uint32_t nseg = 0;
    uint32_t cap = 0;
    uint64_t rec_cap = 0;
    uint64_t nsugg = 0;     // suggested offsets staged for this batch (0 = none)
    uint64_t sugg_origin = 0;
    bool sugg_open_end = false;
    bool host_submit = false;
    uint32_t retries = 0;
    const uint32_t *id_key = nullptr;  // a keyed ticket (pbsgpu_submit_*_keyed): the key's eight words on the device, fixed at
                                       // submit time for every run of the batch; nullptr = plain digests
    bool dense_mode = false;  // scanned at the capacity limit: the resolve walks re-scan overflowed tiles on demand (DenseTiles)
    uint64_t nrec = 0, ncand = 0;

    int init(hipStream_t borrowed = nullptr);  // stream (unless borrowed) + events
    void destroy();  // frees everything (device must be current)
};

}  // namespace pbse

struct pbsgpu_stream;
struct pbsgpu_ring;
struct pbsgpu_known;
struct pbsgpu_engine {
    int device = 0;
    int num_cus = 256;
    // SHA workgroup budget slack (k_order): 25 % keeps one batch's makespan at its longest chunk; with more
    // than 4 batches in flight the chip is oversubscribed anyway and 0 % (fewest CUs per batch) carries more
    uint32_t sha_slack_pct = 25;
    pbsgpu_engine_options opt{};  // as given to pbsgpu_engine_create_opt, defaults resolved (engine.cpp: resolve_engine_options)
    pbsgpu_config cfg{};
    uint32_t bits = 0;     // mask == 2^bits - 1
    uint32_t thr = 0;      // break_min << (32 - bits)
    uint32_t effmin = 0;   // max(min, 65)
    // reader buffer size the suggested-boundary rule emulates (pbsgpu_engine_set_suggested_feed): 1 = byte-serial
    std::atomic<uint64_t> sugg_feed{1};
    std::atomic<uint32_t> sugg_feed_abs{0};
    uint32_t *d_table_rot = nullptr;
    std::vector<std::unique_ptr<pbse::Slot>> slots;  // batch-ticket pool
    std::vector<std::unique_ptr<pbse::Slot>> aux;    // leased to synchronous helper calls
    std::vector<char> aux_busy;
    uint64_t next_ticket = 1;
    std::atomic<int> tickets_out{0};  // pool slots in use (read without the lock as a scheduling hint)
    std::atomic<uint32_t> cap_hint{0};       // per-tile slot capacity that a density retry settled on
    std::atomic<uint32_t> cap_hint_tile{0};  // ... for this tile size
    std::mutex mu;
    std::condition_variable cv;  // an aux lease was returned
    // Host -> device payload copies of ALL streams go through these few engine-wide HIP streams (a page's copies stay on
    // one of them). Measured: one HIP copy stream per payload stream maps 8 streams unevenly onto the SDMA engines
    // (17 GiB/s aggregate, some streams 4x slower than others); two always-busy copy queues carry ~50 GiB/s whatever
    // the number of producers. Only ready copies are ever enqueued here (nothing that waits for a kernel).
    std::vector<hipStream_t> copy_streams;
    std::atomic<uint32_t> copy_rr{0};
    // ... and the per-file XXH3 tees of all streams through these (short kernels behind a page's copy; a stream keeps
    // to one of them so that its pieces run in order). Few engine-wide HIP streams instead of one per payload stream keep a
    // process under the ~20 hardware queues beyond which every kernel pays 19 %.
    std::vector<hipStream_t> tee_streams;
    std::atomic<uint32_t> tee_rr{0};
    // The engine's page ring: every payload stream of the engine is a client of it (stream.cpp). Created by the first
    // pbsgpu_stream_create, destroyed with the engine (or by pbsgpu_engine_trim when no stream is alive).
    std::mutex sring_mu;             // creation / destruction only; the ring has its own lock for use
    pbsgpu_ring *sring = nullptr;
    int sring_users = 0;             // live payload streams (under sring_mu)
    // whole stream contexts (pinned staging, tee buffers, events) of closed streams, re-used by the engine's next stream:
    // allocating 100 MB of pinned memory per archive costs tens of milliseconds, freeing it would wait for the device
    std::mutex pool_mu;
    std::vector<pbsgpu_stream *> stream_pool;
    int refs = 1;                // owner + live streams / chunkers (under mu); freed when it drops to 0
    bool destroyed = false;      // pbsgpu_engine_destroy was called (children may still be alive)
};
// the id key of keyed chunk digests, SHA-256(content || id_key) (engine.cpp): 32 bytes of device memory, the only copy the
// library keeps
struct pbsgpu_id_key {
    pbsgpu_engine *eng = nullptr;
    pbse::DevBuf words;
    const uint32_t *dev() const { return words.as<const uint32_t>(); }
};

namespace pbse {

uint32_t default_cap(const pbsgpu_engine *e, uint64_t nbytes);
// largest per-tile slot capacity a scan is given: one candidate per 128 bytes (or twice the chunker's nominal provisioning,
// whichever is larger). Tiles beyond it are resolved by on-demand re-scans (DenseTiles, kernels.h), never by more memory.
uint32_t cap_limit(const pbsgpu_engine *e, uint32_t tile_bytes);
int set_device(const pbsgpu_engine *e);
bool is_device_pointer(const void *p);

// leases one of the engine's aux slots for the duration of a synchronous helper call (waits for a free one); the slot's
// scratch starts over
struct AuxLease {
    pbsgpu_engine *e;
    Slot *s = nullptr;
    int idx = -1;
    explicit AuxLease(pbsgpu_engine *eng);
    ~AuxLease();
    AuxLease(const AuxLease &) = delete;
    AuxLease &operator=(const AuxLease &) = delete;
};

void engine_ref(pbsgpu_engine *e);
void engine_unref(pbsgpu_engine *e);  // frees the engine when the last reference goes

struct SuggestedHost {  // caller's suggested boundaries: offsets[index[s] .. index[s+1]) ascending, relative to segment s
    const uint64_t *offsets = nullptr;
    const uint32_t *index = nullptr;
    uint64_t origin = 0;  // stream offset of the (single) segment's first byte: only the absolute feed grid needs it
    bool open_end = false;  // the segment ends where the bytes seen so far end, not where the stream ends
};

int enqueue_candidates(pbsgpu_engine *e, Slot &s, const uint8_t *dptr, uint64_t nbytes, uint32_t cap,
                       uint64_t nseg_hint = 0);
int staged_h2d(Slot &s, void *dst, const void *src, uint64_t nbytes, hipStream_t st);
// a host table onto a take of the aux slot's scratch, enqueued on its stream
template <typename T>
int put_table(Slot *s, const T *host, size_t count, const T **dev) {
    T *p = s->take<T>(count);
    CHK(s->taken());
    if (count) CHK(staged_h2d(*s, p, host, count * sizeof(T), s->stream));
    *dev = p;
    return PBSGPU_OK;
}
int stage_segments(pbsgpu_engine *e, Slot &s, const pbsgpu_segment *segs, uint32_t nseg, uint64_t nbytes,
                   const SuggestedHost *sg);
// front half of the whole-range batches (sha256_many, xxh3_many, crc32_many, the blob calls): the segment table (and, with
// `host`, the bytes through the slot's pinned staging) onto the slot; *d = the device bytes; SC_* scalars zeroed
int stage_ranges(pbsgpu_engine *e, Slot *s, const void *ptr, bool host, uint64_t nbytes, const pbsgpu_segment *segs,
                 uint32_t nseg, const uint8_t **d);
// results of a synchronous helper: device -> mapped pinned memory by kernel, stream synchronised, then a host memcpy to dst
int fetch_result(Slot *s, void *dst, const void *src_dev, size_t nbytes);
// SHA-256 of n device ranges of `base` into digs (32 bytes each), with the dense-form policy of pbsgpu_sha256_many_device
// applied to `work`, the sums over the lengths the host knows; queue: a zeroed counter. Enqueued, nothing synchronised.
int enqueue_sha256(pbsgpu_engine *e, hipStream_t st, const uint8_t *base, const pbsgpu_segment *ranges_dev, uint32_t n,
                   uint8_t *digs, uint32_t *queue, const pbsp::ShaWork &work, const uint32_t *key = nullptr);
// (`key`: the device words of a pbsgpu_id_key: keyed digests. `work` counts plain blocks either way: a budget, not a result)
// synchronous helper for the upstream-style chunker (the caller owns the slot)
int candidates_sync(pbsgpu_engine *e, Slot &s, const uint8_t *dptr, uint64_t nbytes, uint64_t *count);
// Caller bytes -> pinned staging. One thread copies ~12 GB/s, the H2D engine moves 57 GB/s: a single writer (the
// reference drives ONE goroutine per archive, internal/tapeio/converter.go:672-680) was memcpy-bound at 24-28 GiB/s.
// Large copies are therefore split over a few helper threads of a process-wide pool (started at the first large
// write; PBSGPU_COPY_THREADS, default 4 incl. the caller, 1 = off). Small writes stay on the caller's thread.
void parallel_memcpy(void *dst, const void *src, size_t n);

}  // namespace pbse
// zstd.hip: the zstd leg of pbsgpu_blob_decode2_device. blob.hip plans it on the host and enqueues these three behind its
// own restore kernels, on the same stream. Every place is an offset from `dst` (64-bit, wrapping: scratch lies elsewhere).
namespace pbsk {
namespace zstd {
// (RestoreJob, RestoreCopy, kNotDecoded, kLitBytes and kDescBytes: blob_plan.h)
struct RestorePlan {
    const uint8_t *src;
    const pbsgpu_segment *blobs;  // nu
    const uint32_t *info, *crcs;  // blob.hip's DecInfo (two words each) and the computed CRCs
    const RestoreJob *jobs;       // nu
    const RestoreCopy *copies;    // ncopy
    const uint32_t *ents;         // nidx: blob, size
    const uint8_t *recs;          // nidx records (nullptr: digests not checked)
    const uint8_t *digs;          // nu * 32: SHA-256 of the decoded bytes
    uint64_t *res;                // nu: zstd status << 32 | bytes decoded; kNotDecoded << 32 for every other blob
    pbsgpu_segment *sha;          // nu: what launch_sha256_segments hashes, relative to dst
    uint8_t *status;              // nidx: blob.hip's statuses, rewritten for the decoded blobs
    uint8_t *dst, *lit;
    uint32_t nu, ncopy, nidx, stride;
};
hipError_t launch_restore_frames(const RestorePlan &pl, void *desc /* nu * kDescBytes */, hipStream_t st);  // pl.stride workgroups
hipError_t launch_restore_copy(const RestorePlan &pl, uint32_t longest, int num_cus, hipStream_t st);
hipError_t launch_restore_status(const RestorePlan &pl, hipStream_t st);
}  // namespace zstd
}  // namespace pbsk
// aes_gcm.hip: the AES leg of pbsgpu_blob_decode3_device, behind the restore's own kernels and the zstd leg on the same
// stream. zp is the zstd leg's plan (src, blobs, info, crcs, jobs, copies, ents, status, dst, lit, stride: the rooms and
// the copies are the same whatever transforms a blob). An encrypted blob with a good CRC is decrypted, a plain one to its
// room, a compressed one to scratch and from there through the frame decoder (with zstd); its entries' statuses are
// rewritten. ub: the distinct blobs (host). res (device, nu): per blob kNotDecoded << 32 when the leg left it alone, else
// status << 32 | bytes with 0xfe = bad tag and bit 0x80 = its plaintext was a frame.
struct pbsgpu_aes_key;
namespace pbsk {
namespace aes {
// idkey (pbsgpu_blob_decode4_device, with zp.recs set): the device words of the id key. Every blob the leg restored is then
// hashed once, keyed, where its plaintext lies (job.place, the length of its result), and an entry that passed tag, frame and
// size is compared with its record's digest on the device: PBSGPU_BLOB_BAD_DIGEST. sha: the budget over the rooms.
int enqueue_restore(pbsgpu_engine *e, pbse::Slot *s, const pbsgpu_aes_key *key, const pbsk::zstd::RestorePlan &zp,
                    const pbsgpu_segment *ub, bool zstd, uint32_t longest_copy, uint64_t *res, const uint32_t *idkey = nullptr,
                    const pbsp::ShaWork *sha = nullptr);
pbsgpu_engine *key_engine(const pbsgpu_aes_key *k);
const void *key_tables(const pbsgpu_aes_key *k);  // the key's pbsa::KeyTables in device memory
constexpr uint32_t kResBadTag = 0xfe, kResFrame = 0x80;
}  // namespace aes
// aes_encode.hip: the AES leg of pbsgpu_blob_encode3_device, on the slot's stream between the encoder's rounds and blob.hip's
// CRC pair. Blob i's message is the frame at dst + doff[i] + 44 when res says it won (res[i] >> 56 == PBSGPU_BLOB_COMPRESSED,
// length in the low bits: encrypted where it lies), else the chunk segs[i] of src (res == nullptr: every chunk). The IV goes
// to bytes 12-27 of the blob, the ciphertext behind byte 44, the tag to bytes 28-43. The pieces are blob.hip's table for
// the slots' capacities (pbase, pseg: device); ivs is the host's array, 16 bytes per blob. Enqueued, nothing synchronised.
namespace aese {
struct Job {
    const uint8_t *src;
    uint8_t *dst;
    const pbsgpu_segment *segs;  // nseg (device)
    const uint64_t *doff;        // nseg + 1 (device)
    const uint64_t *res;         // nseg (device), or nullptr
    const uint64_t *pbase;       // nseg + 1 (device)
    const uint32_t *pseg;        // npieces (device)
    uint32_t nseg, npieces;
};
int enqueue(pbsgpu_engine *e, pbse::Slot *s, const pbsgpu_aes_key *key, const Job &job, const uint8_t *ivs);
}  // namespace aese
}  // namespace pbsk
// zstd_encode.hip: the frames of many chunks, enqueued on a slot's stream (pbsgpu_zstd_encode_device, and the zstd leg of
// pbsgpu_blob_encode2_device, which blob.hip follows with its CRC and header kernels on the same stream).
namespace pbsk {
namespace zenc {
struct Job {  // one chunk: its bytes at src + src_off, its frame's room at dst + dst_off
    uint64_t src_off, src1_off;  // the first `a` bytes, and the rest (a ring chunk in two pages; a == len: one part)
    uint64_t dst_off, room;
    uint32_t len, first;  // first: its first block in the call's block index space (zstd_plan.h)
    uint32_t a;
    uint32_t out;         // its entry of res; kNoJob: not to be encoded, its blocks are left at once
};
constexpr uint32_t kNoJob = 0xffffffffu;
// res_dev[i] = frame length | status << 56. blob = false: PBSGPU_ZSTD_OK or _BAD_SIZE (nothing written, length 0).
// blob = true: room is the chunk's length; PBSGPU_BLOB_COMPRESSED when the frame is strictly shorter than the chunk and
// was written, PBSGPU_BLOB_UNCOMPRESSED (nothing written) otherwise. Takes its arrays from the slot's
// scratch. jobs: src_off, dst_off, room and len from the caller, one part each; the rest is filled in here.
// sums (device, n, may be nullptr): XXH64 of each chunk's content, made on the same stream before; every frame then
// carries the content checksum (4 bytes more; pbsgpu_zstd_encode2_device).
int enqueue(pbsgpu_engine *e, pbse::Slot *s, const uint8_t *src, uint8_t *dst, std::vector<Job> &jobs, bool blob,
            uint64_t **res_dev, const uint64_t *sums = nullptr);
// The same in three steps for a caller that has a kernel of its own fill in what only the device knows of a job (blob.hip's
// fused upload): prepare() plans the blocks from the jobs' `len` and says how much room each array needs;
// carve() takes that room from the slot's scratch and copies the jobs and the block table to it; launch() enqueues the
// rounds.
struct Room {  // device arrays
    Job *jobs;         // n
    uint32_t *bchunk;  // every block of the call: its chunk
    uint64_t *res;     // n
    uint8_t *blkout;   // the largest round's blocks, 128 KiB each
    uint64_t *bplace;  // the largest round's blocks: place in the frame (8 bytes each), then type and size (4 each); then a
                       // block counter per round
    uint8_t *work;     // per workgroup: literals, sequences and, with sources in two parts, the block that holds the seam;
                       // with the long-range match finder its table instead (64 KiB)
};
struct Prep {
    pbsz::enc::BlockPlan bp;
    uint32_t grid = 0;  // workgroups of the block kernel
    bool two_parts = false;
    uint32_t window_log = 0;  // pbsgpu_engine_options::zstd_window_log: the match finder's table is part of `work`
    size_t jobs_bytes = 0, bchunk_bytes = 0, res_bytes = 0, blkout_bytes = 0, bplace_bytes = 0, work_bytes = 0;  // of Room's arrays
};
int prepare(pbsgpu_engine *e, std::vector<Job> &jobs, bool two_parts, Prep &p);  // PBSGPU_E_INVALID: 2^32 blocks or more
int carve(pbse::Slot *s, const Prep &p, const std::vector<Job> &jobs, Room &room);
int launch(pbsgpu_engine *e, hipStream_t st, const Prep &p, const Room &room, const uint8_t *src, uint8_t *dst, bool blob,
           const uint64_t *sums = nullptr);
}  // namespace zenc
}  // namespace pbsk
namespace pbse {

// stream contexts parked in pbsgpu_engine::stream_pool (stream.cpp): really free them (engine teardown, trim)
void stream_pool_release(pbsgpu_engine *e);

// the engine's page ring (stream.cpp): destroyed at engine teardown / trim
void engine_ring_release(pbsgpu_engine *e);

// known.hip: one classify pass of a known-chunk set in pieces, enqueued on a stream the caller owns (the lease of
// known_common, or the fused upload of blob.hip, which builds its encode plan between the marking and the insert).
// The arrays are the caller's: it decides where they live and for how long.
struct KnownPass {
    const uint8_t *recs = nullptr;  // device: n records or .didx entries (`stride` 48 or 40), the digest at offset 8
    uint32_t stride = 0;
    uint64_t n = 0;
    uint32_t *keys = nullptr;       // 2 n: sort keys and their double buffer
    uint32_t *idx = nullptr;        // 2 n: record indices and their double buffer
    uint8_t *before = nullptr;      // n: the digest was in the set before the call
    uint8_t *known = nullptr;       // n: the result
    uint64_t *stats = nullptr;      // 4: records, new, total bytes, new bytes
    void *tmp = nullptr;            // the sort's temporary storage (known_sort_bytes)
    size_t tmp_bytes = 0;
};
int known_sort_bytes(uint64_t n, hipStream_t st, size_t *bytes);
// lookup (k = NULL: nothing is known before the call) / sort / mark: p.known and p.stats are final behind it
int known_enqueue_mark(const pbsgpu_known *k, const KnownPass &p, hipStream_t st);
// true when n more digests could pass the table's load limit: the caller reads p.stats[1] back and calls known_reserve
bool known_may_grow(const pbsgpu_known *k, uint64_t n);
// room for nnew more digests (synchronises `st` when it grows); PBSGPU_E_CAPACITY at the limit of the set's size
int known_reserve(pbsgpu_known *k, uint64_t nnew, hipStream_t st);
// the digests of the records with skip[i] == 0 into the table (they are new: pairwise distinct and absent)
int known_enqueue_insert(pbsgpu_known *k, const KnownPass &p, const uint8_t *skip, hipStream_t st);
void known_inserted(pbsgpu_known *k, uint64_t nnew);  // the insert has completed: the set's count
pbsgpu_engine *known_engine(const pbsgpu_known *k);

}  // namespace pbse
