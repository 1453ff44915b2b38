// The page ring's host-side decisions (ring.cpp): how a ring is sized and how its CUs are split when it is created, how
// the pair / express split follows the data, and what every round decides before it is launched — whether to go, how many
// pages it takes, how many record cells, whether the service start is deferred, how refill and scan share the cut side —
// plus the queue policy numbers the services read. Every input is a parameter: no ring, no clock, no environment, no
// device. Plain C++, no HIP: tests/native/test_ring_plan.cpp runs it under sanitizers.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "../../include/pbsgpu.h"

namespace pbsp {

inline uint32_t pow2_at_least(uint64_t v) {
    uint32_t p = 1;
    while (p < v && p < (1u << 31)) p <<= 1;
    return p;
}

// the chunker as the ring sees it (pbsgpu_config and the engine's effective minimum, max(min, window + 1))
struct ChunkerView {
    uint32_t min, effmin, avg, max, mask;
    uint32_t minsz() const { return std::min(effmin, min); }  // no chunk but a stream's last is shorter
};

// ---- record cells of a round ------------------------------------------------------------------------------------------
// One formula in two forms: a segment (one stream's pages in a round) of `take` pages can end at most this many chunks ...
inline uint64_t seg_cell_bound(uint32_t take, uint64_t page_bytes, uint32_t maxsz, uint32_t minsz) {
    return ((uint64_t)take * page_bytes + maxsz) / minsz + 2;
}
// ... and a full round of round_pages pages in up to max_streams segments never more than this (the sum of the segments'
// bounds is never larger: test_ring_plan.cpp checks it over splits of a round)
inline uint64_t round_rec_cap(uint32_t round_pages, uint64_t page_bytes, uint32_t max_streams, uint32_t maxsz, uint32_t minsz) {
    return ((uint64_t)round_pages * page_bytes + (uint64_t)max_streams * maxsz) / minsz + 4ull * max_streams + 64;
}

// the automatic backlog gate: ~30 ms of the service's throughput (4.3 GiB/s per CU measured) is plenty to ride out the gaps
// between rounds (the gate is sized by the CUs that serve the main and the short queue)
inline uint64_t backlog_auto_bytes(uint32_t sha_cus, uint32_t lanes_cus) { return (uint64_t)(sha_cus + lanes_cus) << 27; }

// ---- the shape of a ring: everything pbsgpu_ring_create decides before its first allocation ---------------------------
// (pbsgpu_ring is one: a ring carries its shape. Only sha_cus, xp_cus and an automatic backlog_limit move afterwards, when
// the split follows the data.)
struct RingShape {
    // geometry
    uint64_t page_bytes = 0, stride = 0;
    uint32_t tile_bytes = 0, tpp = 0, npages = 0, max_streams = 0;
    // the services' CUs: pair (sha), express (xp), lanes
    uint32_t sha_cus = 0, xp_cus = 0;
    uint32_t lanes_cus = 0, short_bytes = 0;  // the LANES service and its short-chunk queue (kernels.h: RingSource::sdesc)
    uint32_t svc_cus = 0;                 // CUs of the services together (constant)
    // The split between the two services follows the DATA (round 5): the share of the published bytes that sits in long
    // chunks (>= long_bytes) is observed as rounds are reaped, and every service START — the ring was idle, nothing is in
    // flight, the change is free — picks the express share that balances the two services' CU-time for that share
    // (adapt_xp_cus). Only when neither the options nor the environment fixed the counts.
    bool split_auto = false;
    uint32_t round_pages = 0, min_round_pages = 0, max_inflight = 3;
    // backlog gate: no page is handed out while more than this many bytes wait in front of the service — committed pages
    // not yet in a round, rounds in flight, published chunks no lane has claimed. A full arena of unhashed chunks feeds
    // the service no faster than a short queue does; it only adds its length to every latency (and to the final drain).
    uint64_t backlog_limit = 0;
    bool backlog_auto = true;             // backlog_limit derived from sha_cus (follows the split)
    double lone_defer_ms = 25.0;          // a lone bulk stream's rounds are cut ahead of the service start for at most this long (0 = off)
    bool defer_service = false;           // PBSGPU_RING_F_DEFER_SERVICE (profiling): rounds only enqueue; quiesce runs the service ALONE
    bool fill_serial = false;             // PBSGPU_RING_F_FILL_SERIAL
    bool dense_service = false;           // PBSGPU_RING_F_DENSE_SERVICE
    bool dense_lanes = false;             // PBSGPU_RING_F_DENSE_LANES
    bool tier_tag = false;                // PBSGPU_RING_F_TIER_TAG
    // sizes of what a round and the arena can hold
    uint32_t cap = 0;                     // candidate slots per scan tile
    uint64_t ntiles = 0, dense_cap = 0, rec_cap = 0;
    uint32_t qslots = 0, ncells = 0, nfree = 0;
    uint32_t long_bytes = 0, lslots = 0, sslots = 0;
    bool long_lo_auto = false;            // RingSource::long_lo from the chunker's maximum (bulk rings)
};

// `o`: the options after the environment's overrides. free_bytes: what hipMemGetInfo reports, read only when
// o.arena_bytes == 0. long_bytes_hint: from which chunk size a chunk takes the express service (0 = 13/16 of the maximum).
// ring_inputs: rounds whose tables may be in flight (kRingInputs). PBSGPU_OK or PBSGPU_E_INVALID.
inline int shape_ring(const pbsgpu_ring_options &o, const ChunkerView &c, int num_cus, uint64_t free_bytes,
                      uint32_t long_bytes_hint, uint32_t ring_inputs, RingShape *out) {
    RingShape s;
    // page geometry: a whole number of scan tiles, >= the largest chunk (so a chunk touches at most two pages)
    const uint32_t big = 64u * 34u * 128u, small = 64u * 4u * 128u;
    uint64_t page = o.page_bytes;
    if (page == 0) {
        const uint32_t tile = c.max >= (1u << 20) ? big : small;
        page = ((uint64_t)c.max + tile - 1) / tile * tile;
        if (page < 2ull * tile && tile == small) page = 2ull * tile;
    }
    if (page % big == 0) s.tile_bytes = big;
    else if (page % small == 0) s.tile_bytes = small;
    else return PBSGPU_E_INVALID;
    if (page < c.max || page >= (1ull << 31)) return PBSGPU_E_INVALID;
    s.page_bytes = page;
    s.tpp = (uint32_t)(page / s.tile_bytes);
    s.stride = page + 256;
    uint64_t arena_bytes = o.arena_bytes;
    if (arena_bytes == 0) arena_bytes = free_bytes > (12ull << 30) ? free_bytes - (8ull << 30) : free_bytes / 2;
    s.npages = (uint32_t)std::min<uint64_t>(arena_bytes / s.stride, 65534);  // 16-bit page ids in the queue descriptors
    {   // the chunk FIFO and the record cells are sized for every chunk the arena can hold (arena / min chunk size):
        // with small average chunk sizes that bound, not HBM, limits the arena (4 M resident chunks = 128 MB of
        // descriptors + 1 GB of pinned record cells)
        const uint64_t lim = (4ull << 20) * c.minsz() / s.page_bytes;
        if (s.npages > lim) s.npages = (uint32_t)std::max<uint64_t>(lim, 4);
    }
    if (s.npages < 4) return PBSGPU_E_INVALID;
    s.max_streams = o.max_streams ? o.max_streams : 64;
    if (s.max_streams > 4096) return PBSGPU_E_INVALID;
    // 3/4 of the chip hashes, 1/4 cuts: per GiB the cut rounds cost ~70 CU-ms (scan 52 + refill 18), the service
    // ~233 CU-ms (128 chains per CU at 1.66-1.75 us per 64-byte block) — measured optimum 192 of 256 CUs
    // (profiles/r03_ring_sweep_*.log: 184 -> 580, 192 -> 597, 200 -> 528, 208 -> 504 GiB/s)
    int sha = o.sha_cus ? (int)o.sha_cus : std::max(1, num_cus - num_cus / 4);
    // EXPRESS service: that many CUs run k_sha256_xpair — two lanes per chunk: the chain of a chunk 1.37x faster (1.28
    // vs 1.75 us per block, profiles/r04_chain_time_pair_vs_express.log) at 0.65 of the throughput per CU — on the
    // chunks of at least long_bytes. Bulk rings (default service share): 16 CUs for chunks >= 13/16 of the maximum
    // (1.3 % of random data's chunks, 5 % of its bytes): the driver's line is unchanged within noise (the drain gets
    // 0.08 s shorter, the feed phase 4 % slower: profiles/r04_ab_express_service.log), one file alone is 15 % sooner.
    // The CUs come out of the pair service's share unless that was given explicitly.
    int xp = o.express_cus == PBSGPU_RING_OFF ? 0 : (int)o.express_cus;
    if (o.express_cus == 0 && !o.sha_cus && num_cus >= 128) xp = 16;
    xp = std::min(xp, std::max(0, num_cus / 2));
    if (xp && !o.sha_cus) sha = std::max(1, sha - xp);
    // The cut side needs its share: with 13/16 of the chip (208 of 256 CUs) in service workgroups the driver's line falls
    // to 525-545 GiB/s, with 216 the cut kernels barely find a CU (a warm-up of 5 files took 120 s:
    // profiles/r04_ab_cu_split.log). Whatever was asked for, the services together get at most 3/4 of the chip + 8.
    const int svc_max = std::max(2, num_cus - num_cus / 4 + (num_cus >= 64 ? 8 : 0));
    if (sha + xp > svc_max) sha = std::max(1, svc_max - xp);
    s.xp_cus = (uint32_t)xp;
    s.sha_cus = (uint32_t)std::min(std::max(sha, 1), std::max(1, num_cus - 1 - xp));
    // LANES service: out of the pair service's share (at most 3/4 of it)
    s.lanes_cus = std::min<uint32_t>(o.lanes_cus, s.sha_cus * 3u / 4u);
    s.sha_cus -= s.lanes_cus;
    s.short_bytes = o.short_bytes ? (uint32_t)std::min<uint64_t>(o.short_bytes, c.max) : (uint32_t)((uint64_t)c.avg * 3 / 2);
    s.svc_cus = s.sha_cus + s.xp_cus + s.lanes_cus;  // (summed BEFORE xp_cus is zeroed for a ring without a long queue, below)
    s.split_auto = xp > 0 && !o.sha_cus && !o.express_cus && s.svc_cus >= 96 && !(o.flags & PBSGPU_RING_F_NO_SPLIT_AUTO);
    s.round_pages = o.round_pages ? o.round_pages : 256;
    s.round_pages = std::min(s.round_pages, s.npages);
    s.min_round_pages = o.min_round_pages ? std::max(1u, std::min(o.min_round_pages, std::max(1u, s.round_pages / 4)))
                                          : std::max(1u, s.round_pages / 4);
    s.backlog_limit = o.backlog_mib < 0   ? 0
                      : o.backlog_mib > 0 ? (uint64_t)(o.backlog_mib * 1048576.0)
                                          : backlog_auto_bytes(s.sha_cus, s.lanes_cus);
    s.backlog_auto = o.backlog_mib == 0;
    if (o.max_inflight) s.max_inflight = std::min<uint32_t>(std::max(1u, o.max_inflight), ring_inputs);
    s.defer_service = (o.flags & PBSGPU_RING_F_DEFER_SERVICE) != 0;
    s.fill_serial = (o.flags & PBSGPU_RING_F_FILL_SERIAL) != 0;
    s.dense_service = (o.flags & PBSGPU_RING_F_DENSE_SERVICE) != 0;
    s.dense_lanes = (o.flags & PBSGPU_RING_F_DENSE_LANES) != 0;
    s.tier_tag = (o.flags & PBSGPU_RING_F_TIER_TAG) != 0;
    s.lone_defer_ms = o.lone_defer_ms < 0 ? 0.0 : o.lone_defer_ms > 0 ? o.lone_defer_ms : 25.0;
    // Candidate slots per scan tile. The batch path starts small and RE-RUNS a batch whose tile overflowed; a ring round
    // cannot be re-run (later rounds continue from it), so the ring provisions for periodic data up front: one
    // candidate per 128 bytes (a repeating block of >= 128 bytes whose every period holds a candidate — BASELINE
    // configs[2]'s repeating 4 KiB files have one per 4 KiB). 12 bytes per slot: ~400 MB at the default round size.
    // A tile beyond that (a crafted short period) keeps what fits and is re-scanned on demand by the resolve walk
    // (DenseTiles, kernels.h): slower for that stretch, exact all the same.
    const double lambda = 3.0 * s.tile_bytes / ((double)c.mask + 1.0);
    uint32_t capv = 8;
    while (capv < 4.0 * lambda + 16.0) capv <<= 1;
    s.cap = std::min<uint32_t>(std::max<uint32_t>(capv * 2, s.tile_bytes / 128), s.tile_bytes);
    s.ntiles = (uint64_t)s.round_pages * s.tpp;
    if (s.ntiles * s.cap >= (1ull << 32)) return PBSGPU_E_INVALID;  // (round_pages far beyond anything an arena holds)
    const uint32_t minsz = c.minsz();
    s.dense_cap = s.ntiles * s.cap;
    s.rec_cap = round_rec_cap(s.round_pages, s.page_bytes, s.max_streams, c.max, minsz);
    const uint64_t resident_chunks = (uint64_t)s.npages * s.page_bytes / minsz + 2ull * s.npages + s.rec_cap;
    s.qslots = pow2_at_least(2 * resident_chunks + 4096);
    s.ncells = pow2_at_least(4 * resident_chunks + 4 * s.rec_cap);
    s.nfree = pow2_at_least(4ull * s.npages + 64);
    // optional long-chunk queue (PBSGPU_RING_LONG_BYTES, e.g. half the maximum chunk size = 8 % of the chunks, 30 % of the
    // bytes of random data): idle lanes look at it first
    // (OFF by default: measured +0.8 % on the bench line for +40 ms of single-file latency — the drain is not made of
    // late-starting long chunks; kept as a switch)
    s.long_bytes = s.xp_cus ? (long_bytes_hint ? long_bytes_hint : (uint32_t)((uint64_t)c.max * 13 / 16)) : 0;
    s.long_lo_auto = long_bytes_hint == 0;  // (a ring with its own threshold — the stream writer's — keeps it)
    if (o.long_bytes) s.long_bytes = o.long_bytes == PBSGPU_RING_OFF ? 0u : o.long_bytes;
    if (s.xp_cus && s.long_bytes == 0) s.xp_cus = 0;  // (no long queue: nothing the express service could take)
    s.lslots = pow2_at_least(2 * ((uint64_t)s.npages * s.page_bytes / std::max<uint32_t>(s.long_bytes, minsz) + s.rec_cap) + 1024);
    s.sslots = s.lanes_cus ? s.qslots : 2;
    *out = s;
    return PBSGPU_OK;
}

// ---- the pair / express split follows the data ------------------------------------------------------------------------
// The express form hashes a chunk 1.37x sooner at 0.70 of the pair form's throughput per CU (2.99 vs 4.28 GiB/s per CU,
// DESIGN.md 5.6). For a share s of the bytes in long chunks both services are equally busy when the express service holds
//   (s / 2.99) / (s / 2.99 + (1 - s) / 4.28)   of the services' CUs:
// 7 % = 16 CUs for random data (s = 0.05: the default), 59 % = 112 CUs for a corpus with half its bytes in zero runs or
// periodic files (BASELINE configs[2]: measured 429 GiB/s with 16 express CUs, 441 / 475 / 490 with 48 / 80 / 112 — every
// page of such a file is held for the chain of a 16 MiB chunk, 0.49 s on a pair lane, 0.34 s on an express pair, and the
// arena binds). Returns the express service's new CU count, or xp_cus itself under the hysteresis.
inline uint32_t adapt_xp_cus(double long_share, uint32_t svc_cus, uint32_t xp_cus) {
    const double s = std::min(1.0, long_share);
    const double fx = (s / 2.99) / (s / 2.99 + (1.0 - s) / 4.28);
    // (x 0.9: the pair lanes help out with long chunks whenever every express pair is busy, the express pairs never take a
    // short chunk — too few express CUs cost little, too many leave the pair service short: configs[2] measured 490 GiB/s at
    // 112 express CUs, 469 at 120, 445 at 128)
    int xp = (int)(0.9 * fx * (double)svc_cus / 8.0 + 0.5) * 8;  // whole XCD rows: other counts leave the XCDs unevenly loaded
    xp = std::max(16, std::min(xp, (int)svc_cus - 32));
    if (std::abs(xp - (int)xp_cus) < 16) return xp_cus;  // hysteresis
    return (uint32_t)xp;
}

// ---- a round: go or wait ----------------------------------------------------------------------------------------------
// A round costs a few dependent launches whatever it holds: while earlier rounds keep the device busy, wait until
// a quarter of a full round has gathered (pages come back from the SHA service one by one). A stream's end and an
// idle device go at once.
inline bool round_gate(size_t inflight, bool any_final, size_t ready, uint32_t min_round_pages, uint32_t max_inflight) {
    if (inflight > 0 && !any_final && ready < min_round_pages) return false;
    // ... and never queue rounds deep: a page that waits behind several queued rounds is resident without being
    // worked on (measured: 16 rounds deep = ~80 ms of extra residency per page, a quarter of the whole)
    return inflight < max_inflight;
}

// record cells: a round takes a contiguous (modulo the ring) range; wait while older rounds still own what the
// largest possible round would overwrite (only a caller that never polls gets here). `oldest`: the cell base of the
// oldest round still kept, or the cursor itself when there is none.
inline bool cells_have_room(uint64_t cell_cursor, uint64_t oldest, uint64_t rec_cap, uint32_t ncells) {
    return cell_cursor + rec_cap - oldest <= ncells;
}

// While the services run the cut side has a quarter of the chip, and there a FULL round costs it 1.5x more per byte than a
// half one (the refill of round n + 1 then runs beside the scan of round n on the same CUs, and nothing of a 4.3 GB round
// is still in the last-level cache when the scan comes to it): measured with 184 + 8 service CUs, where every round was
// full, 680 GiB/s of feed phase at 256 pages per round, 763 at 128, 780 at 32 (profiles/r06_round_size_bistability.log).
// A ring that falls behind once grows its rounds, which makes it fall behind further: round 5's "unexplained" 184 + 8
// cliff and its few-large-rounds regime. So a round takes at most HALF the configured pages while a service runs; the
// whole-chip cut-ahead of an idle ring (no service yet: 64 GiB in ~20 ms) keeps full rounds.
// (Since the refill takes turns with the scan while a service runs — cut_partition — the cap no longer dodges their sharing;
// it stays because it was not measured again without it: profiles/ring_cut_partition.log.)
// (one stream alone is cut-bound on the cut side's quarter of the chip once its service has started, with most lanes
// idle: there the full round is the faster one — one file alone 407 vs 395 ms — and nothing can pile up behind it)
inline uint32_t round_cap(bool service_stopped, uint32_t streams_waiting, uint32_t round_pages, uint32_t min_round_pages) {
    if (service_stopped || streams_waiting < 2) return round_pages;
    return std::max(std::min(round_pages, min_round_pages), round_pages / 2);
}

// ---- a round: start the service with it, or cut ahead of the service --------------------------------------------------
// the bytes that keep every lane of the pair service busy with a chunk of average size
inline uint64_t lanes_worth(uint32_t sha_cus, bool dense_service, uint32_t avg) {
    return (uint64_t)sha_cus * (dense_service ? 256u : 128u) * (uint64_t)avg;
}

struct DeferDecision {
    bool defer;  // this round does not start the service
    bool timed;  // the deferral's clock counts (the caller starts it with this round if it is not running yet)
};
// Start the service with this round — unless it is worth cutting AHEAD of it: a LONE stream that delivers pages in bulk
// (bytes already in device memory) cannot keep the service's lanes busy anyway (a 64 GiB file is 17 k chunks for 24 k
// lanes: it is bound by the chain of its longest chunk), but its scan can use the WHOLE chip while no service holds
// three quarters of it: 64 GiB are cut in ~20 ms at full width instead of ~75 ms on the cut side's quarter. The
// service starts when the stream's bytes are all in, when another stream shows up, or after lone_defer_ms — and
// finds every chunk queued (the queue was reset when the previous service ended, not now).
// The same holds for the first rounds of SEVERAL bulk streams on an idle ring: until the service's lanes could all be
// busy (lanes x average chunk size: ~96 GiB at avg 4 MiB) it only holds CUs the cut side could use — 96 GiB are cut in
// ~26 ms on the whole chip, ~105 ms on a quarter of it with lanes waiting all the while. A trickle of pages (host-fed
// streams: a few pages per pump) never defers: np is small there.
// cut_ahead_bytes: what was cut since the last service ended, this round included. since_ms: how long the deferral has
// lasted (0 when it begins with this round).
inline DeferDecision defer_decision(bool defer_flag, bool service_stopped, double lone_defer_ms, bool any_final, uint32_t np,
                                    uint32_t round_pages, uint32_t sha_cus, bool dense_service, uint32_t avg,
                                    uint64_t cut_ahead_bytes, double since_ms) {
    if (defer_flag) return {true, false};
    if (!service_stopped || !(lone_defer_ms > 0) || any_final || np < std::max<uint32_t>(1, round_pages / 2)) return {false, false};
    return {since_ms < lone_defer_ms && cut_ahead_bytes < lanes_worth(sha_cus, dense_service, avg), true};
}

// ---- a round: how the synthetic refill and the scan share the cut side ------------------------------------------------
struct CutPartition {
    uint32_t scan_blocks, fill_blocks;
    bool fill_shared;  // the refill's workgroups are not one per CU of their own: they share the scan's CUs
    bool fill_serial;  // the refill runs in stream order in front of the scan, not on its own stream
};
// No service (the whole-chip cut-ahead of an idle ring, a lone file): both at full width, the refill on its own stream.
// A service runs: the cut side is shared IN TIME. The refill of round n + 1 goes in stream order behind the scan of round n,
// and each has every cut CU but the one left to the control kernel, which runs beside them on its own stream. Measured
// (profiles/ring_cut_partition.log): whenever the two run at the same time both get dearer per byte, on shared CUs
// (scan 82, refill 28 CU-ms per GiB) and on disjoint ones alike (58 and 22), against 42 and 16 in turn on small rounds: the refill
// is bound by what the memory system takes in beside the services' reads, not by its CUs, and the scan waits on the same
// memory. A ring that had fallen behind once then stayed behind (the large-round regime of round 6).
// fill_cus > 0 (experiments, tests): the partition IN SPACE instead — that many whole-CU refill workgroups on their own
// stream beside the scan, which gets the rest; a ring whose recent rounds had nothing to refill gives them to the scan.
// overlap: the scan side has its own stream, so the control kernel runs beside it.
inline CutPartition cut_partition(bool service_stopped, int num_cus, uint32_t svc_cus, bool overlap, uint32_t fill_cus,
                                  bool fill_serial_flag, uint32_t rounds_since_fill) {
    if (service_stopped) {
        const uint32_t scan = (uint32_t)std::max(1, num_cus);
        return {scan, 2u * scan, true, fill_serial_flag};  // (two 1024-thread workgroups fill a CU's wave slots)
    }
    constexpr uint32_t kFillRecent = 8;  // rounds
    const int cut = std::max(1, num_cus - (int)svc_cus);
    const int rest = cut - ((overlap && cut > 8) ? 1 : 0);  // (one CU stays free for the control kernel)
    if (fill_cus && !fill_serial_flag && rest >= 2) {
        const int F = rounds_since_fill < kFillRecent ? (int)std::min<uint32_t>(fill_cus, (uint32_t)rest - 1u) : 0;
        return {(uint32_t)(rest - F), (uint32_t)std::max(1, F), false, false};
    }
    const uint32_t scan = (uint32_t)std::max(1, rest);
    return {scan, 2u * scan, true, true};
}

// ---- the queue policy the services read (RingSource, kernels.h) -------------------------------------------------------
struct QueueView {
    uint32_t lanes_cus, xp_cus;
    bool dense_lanes, long_lo_auto;
    uint32_t long_bytes;                              // the long queue's threshold (0 = none)
    uint32_t opt_long_lo, opt_long_spill, opt_poll_every;  // pbsgpu_ring_options (0 = the default rule)
    double idle_timeout_s;                            // pbsgpu_ring_options (0 = the default)
    uint32_t cfg_max, minsz;                          // the chunker's maximum and its smallest chunk
};
struct QueuePolicy {
    uint32_t short_room, xp_pairs, long_spill, long_lo, poll_mask;
    unsigned long long idle_ticks;
};
inline QueuePolicy queue_policy(const QueueView &v) {
    QueuePolicy q{};
    // entries that may wait for the lanes service: its lanes take ~2 chunks per CU and round (256 lanes x 1.2 ms / ~0.15 s per
    // chunk); 32 per CU rides out a dozen rounds and fills an idle service within ten
    q.short_room = v.lanes_cus * (v.dense_lanes ? 64u : 32u);
    // the pair lanes take a long chunk only while EVERY express pair is busy (RingCtl::xp_busy): random data keeps the express
    // service just busy (2.6 long chunks per ms against the 2.8 it can take), a corpus whose files are mostly zero runs or
    // periodic (configs[2]: half the bytes in 16 MiB chunks) swamps 16 CUs at once — and a long chunk that WAITS for an express
    // pair (0.36 s + 0.36 s) finishes later than on a pair lane that is free now (0.49 s), holding its page all the while
    // (measured with a queue-length rule instead: ring_manyfiles 441 -> 418 GiB/s, drain 0.50 -> 0.58 s)
    q.long_spill = 0u;
    q.xp_pairs = v.xp_cus * 64u;
    // ... unless the express service is LARGE (the split has followed a corpus of long chunks, adapt_xp_cus): with
    // thousands of express pairs one comes free every few dozen microseconds (6 656 pairs x 0.34 s per 16 MiB chunk: one per
    // 50 us), so a long chunk near the head of the queue is on an express pair — and done 0.15 s sooner than on a pair lane —
    // almost at once. The pair lanes then only see what is queued beyond xp_pairs / 16 (<= 21 ms of waiting).
    if (v.xp_cus >= 32) q.long_spill = q.xp_pairs / 16u;
    // light load (fewer than 3/4 of the express pairs taken): chunks from 11/16 of the maximum on go express too — bulk rings
    // only (the stream writer's ring already sends every chunk >= half the maximum express). One 64 GiB file alone: ~400 chunks
    // >= 11 MiB for 1 024 pairs; its last record then waits for the express chain of a 16 MiB chunk (0.34 s), not for the pair
    // chain of a 12.9 MiB one (0.37 s).
    q.long_lo = (v.xp_cus && v.long_lo_auto) ? (uint32_t)((uint64_t)v.cfg_max * 11 / 16) : 0u;
    if (v.opt_long_lo) q.long_lo = (v.xp_cus && v.opt_long_lo != PBSGPU_RING_OFF) ? v.opt_long_lo : 0u;
    if (q.long_lo >= v.long_bytes) q.long_lo = 0u;
    if (v.opt_long_spill) q.long_spill = v.opt_long_spill;
    const double idle_s = v.idle_timeout_s > 0 ? std::max(0.05, v.idle_timeout_s) : 20.0;
    q.idle_ticks = (unsigned long long)(idle_s * 100e6);  // wall_clock64 runs at 100 MHz
    {   // poll period of waves that carry work (power of two; 1 = every step, the behaviour before round 4)
        // A free lane waits up to `every` block steps (1.75 us each) for its next look at the queue: kept below 0.4 % of the
        // chain of a MINIMUM-size chunk — 8 for small chunkers (tests), 64 at the production average of 4 MiB (min 1 MiB =
        // 16 384 steps). Measured on the driver's command: every 8th step 610.5 / 609.7, every 32nd 617.0 GiB/s, drain
        // 0.430 -> 0.409 s (profiles/r05_ab_long_spill_and_poll.log; round 4: 1 -> 8: 606 -> 615).
        const uint64_t min_steps = v.minsz / 64u;
        int every = (int)std::min<uint64_t>(64, std::max<uint64_t>(8, pow2_at_least(min_steps / 256u + 1u) / 2u));
        if (v.opt_poll_every) every = (int)v.opt_poll_every;
        q.poll_mask = pow2_at_least((uint64_t)every) - 1u;
    }
    return q;
}

}  // namespace pbsp
