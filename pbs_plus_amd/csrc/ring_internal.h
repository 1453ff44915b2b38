// The page ring's host-side state (ring.cpp), shared with the payload-stream writer (stream.cpp), which is a CLIENT of an
// engine-owned ring: pbsgpu_stream_* = staging + H2D into reserved pages + the bookkeeping of sections, tees and entries;
// cutting, hashing, page release and record delivery are the ring's. Not part of the C ABI.
#pragma once

#include <deque>
#include <mutex>
#include <vector>

#include "engine_internal.h"
#include "hold.h"
#include "ring_plan.h"

namespace pbse {

constexpr uint32_t kRingInputs = 16;            // rounds whose host-written tables may be in flight
constexpr uint32_t kPagesPerStreamRound = 256;  // < kRingPT - 2 (open chunk). It was 48 until a lone 64 GiB file turned out to
                                                // go through 83 small rounds, none of them large enough for the cut-ahead at
                                                // full chip width (pbsp::defer_decision): a whole default round per stream now

struct PageReq {                          // a committed page waiting for its round
    uint32_t phys = 0;
    uint64_t k = 0;                       // logical page index in its stream
    uint32_t valid = 0;
    bool final = false;
    bool do_fill = false;
    uint64_t seed = 0, fill_off = 0;
    uint32_t kind = 0;
    const pbsk::FillPiece *tab = nullptr;  // kind 5: the stream's piece table
    uint32_t ntab = 0;
    hipEvent_t dep = nullptr;             // the page's bytes are there once this event has completed (host-fed pages: the
                                          // H2D copy, or the XXH3 tee behind it); from the ring's event pool, returned at enqueue
};

struct CellRef {
    uint32_t cell;
    uint32_t round_idx;                   // RoundInfo::seq of the round that produced it
};

struct StreamSlot {
    bool open = false;
    bool fresh = true;                    // no round has carried this stream yet (device state starts from zero)
    uint64_t next_k = 0;                  // next logical page
    uint64_t bytes_committed = 0;
    uint64_t bytes_enqueued = 0;          // stream length after the rounds enqueued so far
    bool final_committed = false, final_enqueued = false, final_done = false;
    bool zero_final = false;              // final commit of 0 bytes still to be carried by a round
    int64_t reserved = -1;                // physical page handed out by reserve
    int64_t last_phys = -1;               // physical page of the last page that went into a round (the next page's head pad source)
    std::deque<PageReq> ready;
    std::deque<CellRef> cells;            // record cells in stream order (round results reaped)
    uint64_t records_out = 0;
    uint64_t polled_end = 0;              // `end` of the last record handed out (what release / the ring-sourced encode may refer to)
    bool reported = false;                // poll_any has announced the end of this stream
    uint64_t origin = 0;                  // payload position of the stream's byte 0 (absolute reader grid of suggested boundaries)
    std::deque<uint64_t> sugg;            // suggested boundaries still of interest (stream offsets, ascending)
    void *owner = nullptr;                // the stream writer's section that feeds this slot (stream.cpp)
    bool holding = true;                  // on a PBSGPU_RING_F_HOLD_PAGES ring: its pages wait for a release (ring_open_hold)
};

struct RoundInfo {
    uint32_t seq = 0;                     // round number + 1
    uint32_t input = 0;
    uint64_t cell_base = 0;               // monotonic
    uint32_t cell_cap = 0;
    uint32_t live_cells = 0;              // cells handed to streams and not yet polled
    bool reaped = false;
    std::vector<uint32_t> finals;         // slots whose stream ended with this round
    uint64_t new_bytes = 0;               // stream bytes this round added
};

enum class SvcState { Stopped, Running, Stopping };

}  // namespace pbse

struct pbsgpu_ring : pbsp::RingShape {  // (geometry, CU split, round and queue sizes: decided by pbsp::shape_ring at creation)
    pbsgpu_engine *eng = nullptr;
    bool holds_engine_ref = true;         // false for the engine's own ring (the engine owns it, not the reverse)
    std::mutex mu;                        // taken by the stream writer around every use (the C ABI's ring calls are
                                          // single-threaded by contract and do not lock)
    // what the backlog gate (RingShape::backlog_limit) weighs
    uint64_t ready_bytes = 0, inflight_bytes = 0;
    uint32_t tail_seen = 0;               // queue tail after the last reaped round
    uint64_t pub_positions = 0, pub_bytes = 0;  // queue positions / stream bytes of all reaped rounds (average chunk size)
    // device
    pbse::DevBuf arena, ctl, streams, pending, desc, ldesc, sdesc, probe;
    unsigned long long probe_seen[6] = {};  // the probe counters as the newest reaped round reported them (pbsgpu_ring_get_probe)
    bool probe_seen_valid = false;
    unsigned long long ctl_phase_ticks[2][5] = {};  // k_ring_control's phase times summed over the reaped rounds (small / large rounds)
    unsigned long long ctl_phase_rounds[2] = {};
    pbse::DevBuf scalars, tile_cnt, tile_off, tile_slots, scan_tmp, dense, segs, seg_cnt, seg_off, recs, seg_newc, seg_open;
    pbse::DevBuf tile_cnt2, tile_slots2, tileq;  // second set of the scan side (rounds alternate) + the two tile-queue counters
    pbse::DevBuf seg_ecand_in, seg_ecand;
    pbse::DevBuf inputs_dev;  // device mirror of `inputs` (the round tables are staged once per round: k_ring_stage)
    bool stage_inputs = true;
    // mapped pinned
    pbse::PinnedBuf cells, free_fifo, inputs, heartbeat;
    std::vector<pbse::PinnedBuf> piece_tab;      // per stream slot: the piece table of a synthetic edited stream (fill_pieces)
    std::vector<uint32_t> piece_n;
    pbse::PinnedBuf sugg_in[pbse::kRingInputs];  // suggested offsets of the round built in input i (grown on demand)
    size_t input_stride = 0, in_pages_off = 0, in_segs_off = 0, in_recbase_off = 0, in_suggidx_off = 0, in_status_off = 0;
    hipStream_t cs = nullptr, ss = nullptr, fs = nullptr;  // cut rounds, SHA service, synthetic producer
    hipStream_t ls = nullptr;             // the LANES service when lanes_cus > 0
    hipStream_t xs = nullptr;             // the EXPRESS service (two lanes per chunk, long chunks only) when xp_cus > 0
    hipStream_t ps = nullptr;             // scan side of the cut rounds (head pads + scan): round n + 1 is scanned while round n's
                                          // control kernel runs on cs (PBSGPU_RING_OVERLAP=0: everything on cs)
    hipEvent_t ev_scan[pbse::kRingInputs] = {};  // scan of the round built in input i done
    hipEvent_t ev_ctl[2] = {};            // control kernel of the last round that used scan set 0 / 1 done
    bool ctl_used[2] = {false, false};
    uint32_t scan_set = 0;                // scan set of the next round
    int bulk_prio = 0;                    // HIP priority of the refill and scan streams (lowest: the control side goes first)
    double obs_bytes = 0, obs_long_bytes = 0;  // published bytes / those in long chunks since the last split decision (ring_adapt_split)
    hipEvent_t ev_reset = nullptr, ev_svc0 = nullptr, ev_svc1 = nullptr, ev_xsvc1 = nullptr, ev_lsvc1 = nullptr;
    hipEvent_t ev_fill[pbse::kRingInputs] = {};
    std::vector<hipEvent_t> ev_pool;      // page dependency events (ring_event_get / ring_event_put)
    pbse::SvcState svc = pbse::SvcState::Stopped;
    uint32_t rounds_enq = 0;              // mirrored into the heartbeat block for the service's self-stop handshake
    double autopark_ms = 0;               // > 0: stop the service when the ring has been idle this long (engine ring of the stream writer)
    double idle_since_ms = 0;
    uint32_t park_gen_seen = 0;           // last graveyard park request this ring honoured (engine_internal.h: dev_free)
    uint32_t park_grace_gen = 0;          // the park request this ring has already waited its grace period for (ring_start_service)
    double park_wait_t0 = 0;              // since when a start has been waiting for the other rings of the device to let go (ring_start_service)
    bool parked_for_flush = false;        // ... and its service was parked for it: the next start waits for that service's END
    bool hold = false;                    // PBSGPU_RING_F_HOLD_PAGES: handed-back pages wait in `held` for pbsgpu_ring_release
    pbse::HeldPages held;
    uint32_t opt_long_lo = 0, opt_long_spill = 0, opt_poll_every = 0;  // pbsgpu_ring_options (0 = the default rule)
    uint32_t opt_fill_cus = 0;            // pbsgpu_ring_options::fill_cus (0 = the rule in pbsp::cut_partition)
    uint32_t rounds_since_fill = 1000;    // rounds enqueued since the last one with pages for the synthetic refill
    double defer_t0 = 0;                  // when the current deferral began (0 = none)
    uint64_t deferred_bytes = 0;          // bytes cut while no service was running (they are the next launch's work)
    double idle_timeout_s = 0;            // > 0: the service's own idle stop (pbsgpu_ring_options::idle_timeout_s; default 20 s)
    // host bookkeeping
    std::vector<uint32_t> free_pages;
    uint32_t free_read = 0;               // entries of the free FIFO consumed
    std::vector<pbse::StreamSlot> slots;
    std::deque<pbse::RoundInfo> rounds;   // enqueued, oldest first; popped when reaped AND all their cells were polled
    bool input_busy[pbse::kRingInputs] = {};
    uint32_t next_seq = 1;
    uint64_t cell_cursor = 0;
    int error = PBSGPU_OK;
    pbsgpu_ring_stats st{};
    double svc_t0 = 0;
    uint64_t svc_bytes0 = 0;

    uint8_t *in(uint32_t i) const { return inputs.as<uint8_t>() + (size_t)i * input_stride; }
    uint8_t *in_dev(uint32_t i) const { return inputs_dev.as<uint8_t>() + (size_t)i * input_stride; }
    pbsk::RingPage *in_pages(uint32_t i) const { return reinterpret_cast<pbsk::RingPage *>(in(i) + in_pages_off); }
    pbsk::RingSeg *in_segs(uint32_t i) const { return reinterpret_cast<pbsk::RingSeg *>(in(i) + in_segs_off); }
    uint32_t *in_recbase(uint32_t i) const { return reinterpret_cast<uint32_t *>(in(i) + in_recbase_off); }
    uint32_t *in_suggidx(uint32_t i) const { return reinterpret_cast<uint32_t *>(in(i) + in_suggidx_off); }
    pbsk::RingRoundStatus *in_status(uint32_t i) const {
        return reinterpret_cast<pbsk::RingRoundStatus *>(in(i) + in_status_off);
    }
    pbsk::RingSource source() const;
};

namespace pbse {

// ring.cpp internals the stream writer uses (caller holds ring->mu)
// (long_bytes_hint: from which chunk size a chunk takes the express service; 0 = the default 13/16 of the maximum)
int ring_create_internal(pbsgpu_engine *e, const pbsgpu_ring_options *opt, bool hold_engine_ref, pbsgpu_ring **out,
                         uint32_t long_bytes_hint = 0);
// an event from the ring's pool; record it behind the page's last copy / tee and hand it to ring_commit_dep
int ring_event_get(pbsgpu_ring *r, hipEvent_t *ev);
void ring_event_put(pbsgpu_ring *r, hipEvent_t ev);
// pbsgpu_ring_commit with a dependency: the page's bytes are there once `dep` has completed (nullptr = they are now)
int ring_commit_dep(pbsgpu_ring *r, uint32_t stream, uint64_t nbytes, int final, hipEvent_t dep);
// records of one stream that are ready, in order, appended to out[*n ..) (segment = slot)
void ring_pop_records(pbsgpu_ring *r, uint32_t slot, pbsgpu_record *out, uint64_t cap, uint64_t *n);
// stop the service behind everything enqueued so far WITHOUT waiting for it; the next round starts it again
int ring_park(pbsgpu_ring *r);
bool ring_idle(const pbsgpu_ring *r);

// blob.hip: sources in up to two parts (a ring chunk in one or two pages). Offsets from `base`; a part of length 0 is none.
struct SrcPart {
    uint64_t src;
    uint32_t len;
};
// blob i = header + src[i][0] + src[i][1] at dst + doff[i]; crcs (nblob, may be NULL). On a leased aux stream, synchronised.
int blob_encode_parts(pbsgpu_engine *e, const uint8_t *base, const SrcPart (*src)[2], uint32_t nblob, uint8_t *dst,
                      const uint64_t *doff, uint32_t *crcs);
// the parts' bytes back to back at dst
int copy_parts(pbsgpu_engine *e, const uint8_t *base, const SrcPart *src, uint32_t nparts, uint8_t *dst);

// blob.hip: classify against a known-chunk set and frame the new chunks with a plan built on the device
// (pbsgpu_ring_upload_new_device / pbsgpu_known_upload_new_device). The callers have checked everything
// that can be refused on the host.
constexpr uint32_t kBlobPieceLog = 16;  // blob.hip cuts every part into pieces of 64 KiB (its kPieceLog)
struct PageTab {     // one per stream slot of the ring
    uint64_t k0;     // first logical page of the table
    uint32_t off;    // its index in the page array that follows the PageTabs
    uint32_t n;      // pages
};
struct UploadSrc {
    const uint8_t *base = nullptr;           // the ring's arena, or the contiguous source
    const pbsgpu_segment *chunks = nullptr;  // host, n: the contiguous form (then no tables)
    const uint64_t *tabs = nullptr;          // host image: nslots PageTabs, then the offset of every listed page's body from base
    size_t tab_words = 0;
    uint32_t nslots = 0;
    uint32_t stream = 0;                     // or PBSGPU_RING_ANY_STREAM
    uint64_t page_bytes = 0;
    uint64_t pieces_max = 0;                 // upper bound of the 64 KiB pieces of all n chunks, < 2^32
};
// flags: PBSGPU_ENCODE_F_ZSTD or 0; lens, kinds, crcs and enc may be NULL (pbsgpu_*_upload_new2_device)
int upload_new(pbsgpu_known *k, const UploadSrc &src, const pbsgpu_record *recs, uint64_t n, bool insert, uint32_t flags,
               uint8_t *dst, uint64_t dst_cap, uint8_t *known_out, uint64_t *blob_off, uint32_t *lens, uint8_t *kinds,
               uint32_t *crcs, uint64_t *used, pbsgpu_dedup_stats *stats, pbsgpu_encode_stats *enc);

// ---- the engine's ring holds pages for the payload streams that ask for it (pbsgpu_stream_hold) ----
// pbsgpu_ring_open with the choice: a stream opened with hold = false on a PBSGPU_RING_F_HOLD_PAGES ring gets no page
// assignments — its pages are nobody's and go to the free list the moment the services hand them back
int ring_open_hold(pbsgpu_ring *r, uint32_t *stream, bool hold);
// no page is free and none can become free without a release (hold.h: frees_without_release): waiting would never end
bool ring_page_needs_release(pbsgpu_ring *r);
// The host's part of pbsgpu_ring_upload_new2_device / pbsgpu_ring_copy_device: the range checks and the page lookup. The
// caller holds ring->mu for THIS and runs the device work without it (only its own release could free those pages).
struct UploadPlan {
    UploadSrc us;
    std::vector<uint64_t> tabs;
};
int ring_upload_plan(pbsgpu_ring *r, uint32_t stream, const pbsgpu_record *recs, uint64_t n, UploadPlan *plan);
int ring_copy_plan(pbsgpu_ring *r, uint32_t stream, uint64_t offset, uint64_t length, std::vector<SrcPart> *parts);

}  // namespace pbse
