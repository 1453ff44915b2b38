// The page ring's host-side decisions (pbs_plus_amd/csrc/ring_plan.h) on their own, under ASan + UBSan:
//   (a) the values the project's documents and comments state, each with its source;
//   (b) invariants over a seeded sweep of options, chunker configurations and CU counts;
//   (c) the shapes the parent commit's build reported on the device (argv[1]: tests/golden/ring_shape_v1.txt).
// Every case checks itself; "ring-plan-ok" at the end.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../pbs_plus_amd/csrc/ring_plan.h"

#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);          \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

using namespace pbsp;

constexpr uint32_t kInputs = 16;  // ring_internal.h: kRingInputs

// buzhash.NewConfig(avg): min = avg / 4, max = 4 * avg, mask = 2 * avg - 1; the engine's effmin = max(min, window + 1)
static ChunkerView chunker(uint32_t avg) { return {avg / 4, std::max(avg / 4, 65u), avg, avg * 4, 2 * avg - 1}; }

static bool is_pow2(uint32_t v) { return v && !(v & (v - 1)); }

// ---- (a) stated values ------------------------------------------------------------------------------------------------

static void shape_cases() {
    const ChunkerView c = chunker(4u << 20);
    pbsgpu_ring_options o{};
    RingShape s;
    // NEXT.md, "State": "pair service 176 CUs + express 16"; ring_plan.h: the backlog gate is 128 MiB per CU of the main queue
    REQUIRE(shape_ring(o, c, 256, 280ull << 30, 0, kInputs, &s) == PBSGPU_OK);
    REQUIRE(s.sha_cus == 176 && s.xp_cus == 16 && s.lanes_cus == 0 && s.svc_cus == 192 && s.split_auto);
    REQUIRE(s.backlog_auto && s.backlog_limit == 176ull << 27);
    // include/pbsgpu.h: "16.2 MiB at avg 4 MiB", "0 = what is free minus 8 GiB", round_pages "0 = 256", max_inflight "0 = 3",
    // min_round_pages "0 = round_pages / 4", long_bytes "0 = 13/16 of the maximum", short_bytes "0 = 3/2 of the average"
    REQUIRE(s.page_bytes == 61ull * 64 * 34 * 128 && s.tile_bytes == 64u * 34 * 128 && s.tpp == 61 && s.stride == s.page_bytes + 256);
    REQUIRE(s.npages == (272ull << 30) / s.stride && s.max_streams == 64);
    REQUIRE(s.round_pages == 256 && s.min_round_pages == 64 && s.max_inflight == 3 && s.lone_defer_ms == 25.0);
    REQUIRE(s.long_bytes == (16u << 20) / 16 * 13 && s.long_lo_auto && s.short_bytes == 6u << 20);
    // shape_ring: "Whatever was asked for, the services together get at most 3/4 of the chip + 8" = 200 of 256
    o.sha_cus = 250;
    REQUIRE(shape_ring(o, c, 256, 280ull << 30, 0, kInputs, &s) == PBSGPU_OK);
    REQUIRE(s.sha_cus + s.xp_cus == 200 && s.xp_cus == 0 && !s.split_auto);
    o.express_cus = 16;
    REQUIRE(shape_ring(o, c, 256, 280ull << 30, 0, kInputs, &s) == PBSGPU_OK);
    REQUIRE(s.sha_cus + s.xp_cus == 200 && s.xp_cus == 16);
    // the limits: 16-bit page ids, 4 Mi resident chunks, at least 4 pages, at most 4096 streams, pages of whole tiles >= max
    o = pbsgpu_ring_options{};
    REQUIRE(shape_ring(o, c, 256, 4096ull << 30, 0, kInputs, &s) == PBSGPU_OK && s.npages == 65534);
    const ChunkerView tiny = chunker(256);
    REQUIRE(shape_ring(o, tiny, 256, 280ull << 30, 0, kInputs, &s) == PBSGPU_OK);
    REQUIRE(s.page_bytes == 65536 && s.npages == (4ull << 20) * 64 / 65536);
    o.arena_bytes = 3 * (16990208ull + 256);
    REQUIRE(shape_ring(o, c, 256, 0, 0, kInputs, &s) == PBSGPU_E_INVALID);
    o.arena_bytes = 4 * (16990208ull + 256);
    REQUIRE(shape_ring(o, c, 256, 0, 0, kInputs, &s) == PBSGPU_OK && s.npages == 4 && s.round_pages == 4);
    o.max_streams = 4097;
    REQUIRE(shape_ring(o, c, 256, 0, 0, kInputs, &s) == PBSGPU_E_INVALID);
    o.max_streams = 4096;
    REQUIRE(shape_ring(o, c, 256, 0, 0, kInputs, &s) == PBSGPU_OK);
    o.page_bytes = (16u << 20) + 4096;  // not a whole number of tiles of either size
    REQUIRE(shape_ring(o, c, 256, 0, 0, kInputs, &s) == PBSGPU_E_INVALID);
    o.page_bytes = 60ull * 64 * 34 * 128;  // whole tiles, below the largest chunk
    REQUIRE(shape_ring(o, c, 256, 0, 0, kInputs, &s) == PBSGPU_E_INVALID);
    // the quirk that stays: svc_cus is summed before xp_cus is zeroed for a ring without a long queue
    o = pbsgpu_ring_options{};
    o.long_bytes = PBSGPU_RING_OFF;
    REQUIRE(shape_ring(o, c, 256, 280ull << 30, 0, kInputs, &s) == PBSGPU_OK);
    REQUIRE(s.xp_cus == 0 && s.long_bytes == 0 && s.sha_cus == 176 && s.svc_cus == 192);
}

static void adapt_cases() {
    // adapt_xp_cus: "7 % = 16 CUs for random data (s = 0.05: the default)"
    REQUIRE(adapt_xp_cus(0.05, 192, 64) == 16);
    // s = 0.5: fx = (0.5 / 2.99) / (0.5 / 2.99 + 0.5 / 4.28) = 0.16722 / 0.28405 = 0.58871 (the comment's "59 % = 112 CUs":
    // 0.58871 * 192 = 113.0 -> 112 in rows of 8). With the x 0.9: 0.9 * 0.58871 * 192 / 8 = 12.716, + 0.5 -> 13 rows = 104.
    REQUIRE(adapt_xp_cus(0.5, 192, 16) == 104);
    // hysteresis: less than 16 CUs apart = unchanged
    REQUIRE(adapt_xp_cus(0.5, 192, 96) == 96 && adapt_xp_cus(0.5, 192, 112) == 112 && adapt_xp_cus(0.5, 192, 119) == 119);
    REQUIRE(adapt_xp_cus(0.5, 192, 88) == 104 && adapt_xp_cus(0.5, 192, 120) == 104);
    REQUIRE(adapt_xp_cus(0.05, 192, 31) == 31 && adapt_xp_cus(0.05, 192, 32) == 16);
    // never below 16, never more than svc_cus - 32; a share beyond 1 is 1
    REQUIRE(adapt_xp_cus(0.0, 192, 64) == 16 && adapt_xp_cus(1.0, 192, 16) == 160 && adapt_xp_cus(7.0, 192, 16) == 160);
}

static void round_cases() {
    // round_cap: "a round takes at most HALF the configured pages while a service runs", full rounds for an idle ring and
    // for one stream alone
    REQUIRE(round_cap(true, 5, 256, 64) == 256);
    REQUIRE(round_cap(false, 1, 256, 64) == 256 && round_cap(false, 0, 256, 64) == 256);
    REQUIRE(round_cap(false, 2, 256, 64) == 128);
    REQUIRE(round_cap(false, 2, 2, 1) == 1);
    REQUIRE(round_cap(false, 2, 1, 1) == 1);
    // round_gate: "A stream's end and an idle device go at once", "never queue rounds deep"
    REQUIRE(round_gate(0, false, 1, 64, 3));
    REQUIRE(!round_gate(1, false, 63, 64, 3) && round_gate(1, false, 64, 64, 3) && round_gate(1, true, 1, 64, 3));
    REQUIRE(round_gate(2, true, 1, 64, 3) && !round_gate(3, true, 1000, 64, 3));
    // cells: the largest possible round must fit beside what the oldest kept round still owns
    REQUIRE(cells_have_room(1000, 1000, 500, 512) && !cells_have_room(1000, 1000, 513, 512));
    REQUIRE(cells_have_room(1012, 1000, 500, 512) && !cells_have_room(1013, 1000, 500, 512));
}

static void defer_cases() {
    const uint64_t worth = lanes_worth(176, false, 4u << 20);  // 128 lanes per CU, 256 with the dense service
    REQUIRE(worth == 176ull * 128 * (4u << 20) && lanes_worth(176, true, 4u << 20) == 2 * worth);
    auto d = [&](bool flag, bool stopped, double lone, bool fin, uint32_t np, uint64_t bytes, double since) {
        return defer_decision(flag, stopped, lone, fin, np, 256, 176, false, 4u << 20, bytes, since);
    };
    REQUIRE(d(true, false, 25, true, 1, 0, 0).defer && !d(true, false, 25, true, 1, 0, 0).timed);  // the profiling flag: always
    REQUIRE(d(false, true, 25, false, 128, 1, 0).defer && d(false, true, 25, false, 128, 1, 0).timed);
    REQUIRE(!d(false, false, 25, false, 256, 1, 0).defer);   // a service runs
    REQUIRE(!d(false, true, 0, false, 256, 1, 0).defer);     // lone_defer_ms off
    REQUIRE(!d(false, true, 25, true, 256, 1, 0).defer);     // a stream's end
    REQUIRE(!d(false, true, 25, false, 127, 1, 0).defer && !d(false, true, 25, false, 127, 1, 0).timed);  // a trickle of pages
    REQUIRE(!d(false, true, 25, false, 256, 1, 25.0).defer && d(false, true, 25, false, 256, 1, 25.0).timed);  // long enough
    REQUIRE(d(false, true, 25, false, 256, worth - 1, 24.9).defer && !d(false, true, 25, false, 256, worth, 0).defer);
    REQUIRE(defer_decision(false, true, 25, false, 1, 1, 1, false, 4096, 1, 0).defer);  // round_pages 1: half a round is 1 page
}

static void partition_cases() {
    auto same = [](CutPartition p, uint32_t scan, uint32_t fill, bool shared, bool serial) {
        return p.scan_blocks == scan && p.fill_blocks == fill && p.fill_shared == shared && p.fill_serial == serial;
    };
    // cut_partition: "No service: both at full width, the refill on its own stream"
    REQUIRE(same(cut_partition(true, 256, 192, true, 0, false, 0), 256, 512, true, false));
    REQUIRE(same(cut_partition(true, 256, 192, true, 8, true, 0), 256, 512, true, true));
    // "A service runs: the cut side is shared IN TIME ... every cut CU but the one left to the control kernel"
    REQUIRE(same(cut_partition(false, 256, 192, true, 0, false, 0), 63, 126, true, true));
    // "fill_cus > 0: the partition IN SPACE ... a ring whose recent rounds had nothing to refill gives them to the scan"
    REQUIRE(same(cut_partition(false, 256, 192, true, 8, false, 0), 55, 8, false, false));
    REQUIRE(same(cut_partition(false, 256, 192, true, 8, false, 7), 55, 8, false, false));
    REQUIRE(same(cut_partition(false, 256, 192, true, 64, false, 0), 1, 62, false, false));
    REQUIRE(same(cut_partition(false, 256, 192, true, 8, false, 8), 63, 1, false, false));
    REQUIRE(same(cut_partition(false, 256, 192, true, 8, false, 1000), 63, 1, false, false));
    REQUIRE(same(cut_partition(false, 256, 192, true, 8, true, 0), 63, 126, true, true));  // PBSGPU_RING_F_FILL_SERIAL wins
    // no CU is set aside for the control kernel on a cut side of 8 CUs or fewer, or without the scan's own stream
    REQUIRE(same(cut_partition(false, 64, 56, true, 0, false, 0), 8, 16, true, true));
    REQUIRE(same(cut_partition(false, 64, 55, true, 0, false, 0), 8, 16, true, true));
    REQUIRE(same(cut_partition(false, 256, 192, false, 0, false, 0), 64, 128, true, true));
    // fewer than two CUs left: nothing to partition
    REQUIRE(same(cut_partition(false, 2, 1, true, 8, false, 0), 1, 2, true, true));
    REQUIRE(same(cut_partition(false, 8, 8, true, 8, false, 0), 1, 2, true, true));
    REQUIRE(same(cut_partition(false, 8, 6, true, 8, false, 0), 1, 1, false, false));
    const int cus[] = {1, 2, 8, 64, 128, 256, 304};
    for (int stopped = 0; stopped < 2; ++stopped)
        for (int n : cus)
            for (uint32_t svc = 0; svc <= (uint32_t)n + 9; ++svc)
                for (int overlap = 0; overlap < 2; ++overlap)
                    for (uint32_t fill : {0u, 1u, 8u, 64u, 1000u, 0xffffffffu})
                        for (int flag = 0; flag < 2; ++flag)
                            for (uint32_t since : {0u, 7u, 8u, 1000u}) {
                                const CutPartition p = cut_partition(stopped, n, svc, overlap, fill, flag, since);
                                REQUIRE(p.scan_blocks >= 1 && p.fill_blocks >= 1);
                            }
}

static void policy_cases() {
    const ChunkerView c = chunker(4u << 20);
    QueueView v{0, 16, false, true, c.max / 16 * 13, 0, 0, 0, 0.0, c.max, c.minsz()};
    QueuePolicy q = queue_policy(v);
    // queue_policy: xp_pairs = CUs x 64; the pair lanes help "only while EVERY express pair is busy" (long_spill 0) up to a
    // LARGE express service (>= 32 CUs: xp_pairs / 16); long_lo "11/16 of the maximum" on bulk rings; "64 at the production
    // average of 4 MiB"; idle stop after 20 s of 100 MHz ticks
    REQUIRE(q.short_room == 0 && q.xp_pairs == 1024 && q.long_spill == 0 && q.long_lo == c.max / 16 * 11 && q.poll_mask == 63);
    REQUIRE(q.idle_ticks == 2000000000ull);
    v.xp_cus = 104;
    REQUIRE(queue_policy(v).long_spill == 104 * 64 / 16 && queue_policy(v).xp_pairs == 6656);  // "6 656 pairs"
    v.opt_long_spill = 5;
    REQUIRE(queue_policy(v).long_spill == 5);
    v.long_lo_auto = false;  // the stream writer's ring keeps its own threshold
    REQUIRE(queue_policy(v).long_lo == 0);
    v.opt_long_lo = 1000;
    REQUIRE(queue_policy(v).long_lo == 1000);
    v.opt_long_lo = v.long_bytes;  // at or beyond long_bytes it means nothing
    REQUIRE(queue_policy(v).long_lo == 0);
    v.opt_long_lo = PBSGPU_RING_OFF;
    v.long_lo_auto = true;
    REQUIRE(queue_policy(v).long_lo == 0);
    v.opt_long_lo = 1000;
    v.xp_cus = 0;
    REQUIRE(queue_policy(v).long_lo == 0 && queue_policy(v).xp_pairs == 0);
    v.lanes_cus = 32;  // "32 per CU", 64 with the dense lanes service
    REQUIRE(queue_policy(v).short_room == 1024);
    v.dense_lanes = true;
    REQUIRE(queue_policy(v).short_room == 2048);
    v.minsz = chunker(64u << 10).minsz();  // "8 for small chunkers (tests)"
    REQUIRE(queue_policy(v).poll_mask == 7);
    v.opt_poll_every = 5;  // rounded up to a power of two
    REQUIRE(queue_policy(v).poll_mask == 7);
    v.opt_poll_every = 1;
    REQUIRE(queue_policy(v).poll_mask == 0);
    v.idle_timeout_s = 0.001;  // at least 50 ms
    REQUIRE(queue_policy(v).idle_ticks == 5000000ull);
    v.idle_timeout_s = 5.0;
    REQUIRE(queue_policy(v).idle_ticks == 500000000ull);
    REQUIRE(pow2_at_least(0) == 1 && pow2_at_least(1) == 1 && pow2_at_least(3) == 4 && pow2_at_least(4) == 4);
    REQUIRE(pow2_at_least(1ull << 40) == 1u << 31);
}

// ---- (b) invariants over a seeded sweep -------------------------------------------------------------------------------

template <class T>
static T pick(std::mt19937_64 &g, std::initializer_list<T> l) {
    return l.begin()[g() % l.size()];
}

static pbsgpu_ring_options random_options(std::mt19937_64 &g, const ChunkerView &c, int num_cus) {
    pbsgpu_ring_options o{};
    const uint64_t tile = c.max >= (1u << 20) ? 64u * 34u * 128u : 64u * 4u * 128u;
    const uint64_t page = std::max<uint64_t>(2, (c.max + tile - 1) / tile) * tile;
    o.page_bytes = pick<uint64_t>(g, {0, 0, page, 2 * page, page + tile});
    o.arena_bytes = pick<uint64_t>(g, {0, 0, 4 * (2 * page + 256), 10 * (2 * page + 256), 1ull << 30, 64ull << 30, 1ull << 42});
    o.max_streams = pick<uint32_t>(g, {0, 1, 4, 64, 1000, 4096});
    o.sha_cus = pick<uint32_t>(g, {0, 0, 1, (uint32_t)(g() % (2 * num_cus + 1)), 1000});
    o.express_cus = pick<uint32_t>(g, {0, 0, PBSGPU_RING_OFF, 1, (uint32_t)(g() % (num_cus + 1)), 1000});
    o.lanes_cus = pick<uint32_t>(g, {0, 0, 1, (uint32_t)(g() % (num_cus + 1)), 1000});
    o.round_pages = pick<uint32_t>(g, {0, 0, 1, 2, 7, 256, 1000, 70000});
    o.min_round_pages = pick<uint32_t>(g, {0, 0, 1, 3, 64, 100000});
    o.max_inflight = pick<uint32_t>(g, {0, 1, 3, 16, 100});
    o.long_bytes = pick<uint32_t>(g, {0, 0, PBSGPU_RING_OFF, c.max / 2, 1});
    o.short_bytes = pick<uint64_t>(g, {0, 1, c.avg, 1ull << 40});
    o.backlog_mib = pick<double>(g, {0.0, 0.0, -1.0, 0.5, 4096.0});
    o.lone_defer_ms = pick<double>(g, {0.0, -1.0, 3.0});
    o.flags = (uint32_t)(g() & 0x3ff);
    return o;
}

static void sweep() {
    std::mt19937_64 g(20240607);
    const int cus[] = {1, 8, 64, 128, 256, 304};
    uint64_t ok = 0, refused = 0;
    for (uint32_t k = 8; k <= 28; ++k) {  // every average NewConfig accepts (tests/config_inputs.py: AVGS)
        const ChunkerView c = chunker(1u << k);
        for (int n : cus)
            for (int trial = 0; trial < 48; ++trial) {
                const pbsgpu_ring_options o = random_options(g, c, n);
                const uint64_t free_bytes = pick<uint64_t>(g, {1ull << 30, 20ull << 30, 280ull << 30});
                const uint32_t hint = pick<uint32_t>(g, {0, 0, c.max / 2});
                RingShape s;
                const int st = shape_ring(o, c, n, free_bytes, hint, kInputs, &s);
                REQUIRE(st == PBSGPU_OK || st == PBSGPU_E_INVALID);
                if (st != PBSGPU_OK) {
                    ++refused;
                    continue;
                }
                ++ok;
                REQUIRE(s.sha_cus >= 1);
                if (n > 1) REQUIRE(s.sha_cus + s.xp_cus + s.lanes_cus <= (uint32_t)n - 1);
                REQUIRE(s.page_bytes >= c.max && s.page_bytes % s.tile_bytes == 0 && s.tpp * (uint64_t)s.tile_bytes == s.page_bytes);
                REQUIRE(s.npages >= 4 && s.npages <= 65534);
                REQUIRE(is_pow2(s.qslots) && is_pow2(s.ncells) && is_pow2(s.nfree) && is_pow2(s.lslots));
                REQUIRE(s.min_round_pages >= 1 && s.min_round_pages <= s.round_pages && s.round_pages <= s.npages);
                REQUIRE(s.max_inflight >= 1 && s.max_inflight <= kInputs);
                REQUIRE(s.xp_cus == 0 || s.long_bytes > 0);
                REQUIRE(s.rec_cap == round_rec_cap(s.round_pages, s.page_bytes, s.max_streams, c.max, c.minsz()));
                // ring.cpp, round_gather: "the bound above is never larger" — the segments' cell bounds of any round
                for (int split = 0; split < 6; ++split) {
                    const uint32_t nseg = split == 0 ? s.max_streams : 1 + (uint32_t)(g() % s.max_streams);
                    uint32_t left = s.round_pages;
                    uint64_t cells = 0;
                    for (uint32_t i = 0; i < nseg; ++i) {
                        // the first split gives every page to the last segment, the second one page each, the others at random
                        uint32_t take = split == 0 ? (i + 1 == nseg ? left : 0) : split == 1 ? std::min(left, 1u) : (uint32_t)(g() % (left + 1));
                        if (split > 1 && i + 1 == nseg) take = left;
                        left -= take;
                        cells += seg_cell_bound(take, s.page_bytes, c.max, c.minsz());
                    }
                    REQUIRE(cells <= s.rec_cap);
                }
            }
    }
    REQUIRE(ok > 2000 && refused > 100);  // (both outcomes are exercised)
}

// ---- (c) the parent's own answers -------------------------------------------------------------------------------------

static void fixture(const char *path) {
    std::FILE *f = std::fopen(path, "r");
    REQUIRE(f != nullptr);
    char line[1024];
    int cases = 0;
    while (std::fgets(line, sizeof line, f)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        long long v[26];
        int n = 0;
        for (char *p = line, *e = nullptr; n < 26; ++n, p = e) {
            v[n] = std::strtoll(p, &e, 10);
            if (e == p) break;
        }
        REQUIRE(n == 26);
        // num_cus avg min max mask | arena_bytes page_bytes max_streams sha_cus round_pages express_cus min_round_pages
        // max_inflight long_bytes flags lanes_cus backlog_mib short_bytes | page_bytes pages_total sha_cus express_cus
        // long_bytes backlog_limit lanes_cus short_bytes
        const ChunkerView c{(uint32_t)v[2], std::max((uint32_t)v[2], 65u), (uint32_t)v[1], (uint32_t)v[3], (uint32_t)v[4]};
        pbsgpu_ring_options o{};
        o.arena_bytes = (uint64_t)v[5];
        o.page_bytes = (uint64_t)v[6];
        o.max_streams = (uint32_t)v[7];
        o.sha_cus = (uint32_t)v[8];
        o.round_pages = (uint32_t)v[9];
        o.express_cus = (uint32_t)v[10];
        o.min_round_pages = (uint32_t)v[11];
        o.max_inflight = (uint32_t)v[12];
        o.long_bytes = (uint32_t)v[13];
        o.flags = (uint32_t)v[14];
        o.lanes_cus = (uint32_t)v[15];
        o.backlog_mib = (double)v[16];
        o.short_bytes = (uint64_t)v[17];
        RingShape s;
        REQUIRE(shape_ring(o, c, (int)v[0], 0, 0, kInputs, &s) == PBSGPU_OK);
        REQUIRE(s.page_bytes == (uint64_t)v[18] && s.npages == (uint32_t)v[19] && s.sha_cus == (uint32_t)v[20]);
        REQUIRE(s.xp_cus == (uint32_t)v[21] && (s.xp_cus ? s.long_bytes : 0u) == (uint32_t)v[22]);  // (pbsgpu_ring_express)
        REQUIRE(s.backlog_limit == (uint64_t)v[23] && s.lanes_cus == (uint32_t)v[24] && s.short_bytes == (uint32_t)v[25]);
        ++cases;
    }
    std::fclose(f);
    REQUIRE(cases >= 12);
}

int main(int argc, char **argv) {
    REQUIRE(argc == 2);
    shape_cases();
    adapt_cases();
    round_cases();
    defer_cases();
    partition_cases();
    policy_cases();
    sweep();
    fixture(argv[1]);
    std::puts("ring-plan-ok");
    return 0;
}
