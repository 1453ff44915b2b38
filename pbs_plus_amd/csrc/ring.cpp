// libpbsgpu host side, part 3: the PAGE RING — many payload streams through one device arena with page-granular
// memory release and a persistent cross-stream SHA-256 service. Since round 4 it is THE engine behind every streaming
// entry point: pbsgpu_ring_* drives it directly (bytes already in device memory), pbsgpu_stream_* (stream.cpp) is a client
// that feeds host bytes into reserved pages.
//
// Why it exists. SHA-256 is serial inside a chunk (a 16 MiB chunk = 262 144 dependent compressions ~ 0.43 s on one
// lane), so a batch submitted with pbsgpu_submit_device keeps ALL its bytes resident until its longest chunk is done:
// throughput <= resident bytes / 0.45 s whatever the chip could hash. The ring removes the batch as the unit of
// residency. It stands where the chunk loop behind WriteEntryReader runs for every archive of a multi-archive ingest
// (internal/pxarmount/commit_reuse.go:457, internal/tapeio/converter.go:836):
//   * device memory is an arena of fixed PAGES (>= max chunk, a whole number of scan tiles). A stream is a sequence
//     of pages in logical order; physically they lie wherever a page was free;
//   * newly filled pages of all streams are cut in ROUNDS (ring_kernels.hip): scan of the new pages only, multi-stream
//     resolve continuing from each stream's open chunk (device-resident state: no host round trip between rounds);
//   * every cut chunk goes into ONE device-resident FIFO that the SHA-256 SERVICE — a persistent kernel on a fixed set
//     of CUs — drains: a lane takes the next chunk the moment it finishes one, across rounds and streams;
//   * each page counts the chunks that still have to be read from it (plus a hold while the stream's open chunk
//     reaches into it). The lane that loads a chunk's last block drops the reference; a page that reaches zero is
//     reported to the host through mapped pinned memory and can take new bytes at once — residency per page is the
//     hash time of the longest chunk that touches THAT page, not of the longest chunk of a 64 GiB batch;
//   * digests and record fields land in host-visible record cells; pbsgpu_ring_poll hands them out per stream, in order.
// One thread drives a ring (like one goroutine owns a writer, internal/tapeio/converter.go:672-680).
//
// No byte content fails a stream: a scan tile that finds more candidates than it has slots (periodic / crafted data) is
// resolved exactly by an on-demand re-scan inside the control kernel (DenseTiles, kernels.h) — like the reference's writer,
// which has no content-dependent error (internal/pxarmount/commit_reuse.go:457, internal/tapeio/converter.go:836).
// A host that stops calling for longer than the idle timeout finds the service gone and the ring healthy — the next round
// starts it again.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "ring_internal.h"

using namespace pbse;

namespace {

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

volatile uint32_t *hb_words(const pbsgpu_ring *r) { return r->heartbeat.as<volatile uint32_t>(); }

// the service launched last is known to have ended: statistics, the service count, parked frees
void ring_service_ended(pbsgpu_ring *r) {
    if (r->svc == SvcState::Stopped) return;
    r->svc = SvcState::Stopped;
    float ms = 0;
    if (hipEventElapsedTime(&ms, r->ev_svc0, r->ev_svc1) == hipSuccess) {
        r->st.service_ms_last = ms;
        r->st.service_ms_total += ms;
    } else {
        (void)hipGetLastError();
    }
    r->st.service_bytes_last = r->st.bytes_enqueued - r->svc_bytes0;
    volatile uint32_t *hb = hb_words(r);
    hb[pbsk::kHbIntent] = 0;
    hb[pbsk::kHbCommitted] = 0;
    // head := tail, stop := 0 — NOW, while nothing is published behind the service's back: its lanes may have left holding
    // claims beyond the tail, and rounds enqueued from here on (even before the next service starts: a lone stream's rounds
    // are cut ahead at full chip width, pbsp::defer_decision) must find the queue ready to be served from exactly this point
    if (r->cs) {
        (void)pbsk::launch_ring_reset(r->ctl.as<pbsk::RingCtl>(), r->cs);
        (void)hipEventRecord(r->ev_reset, r->cs);
    }
    r->parked_for_flush = false;
    service_ended(r->eng->device);  // (the device's last service: memory parked by dev_free / host_free is freed now)
}

// Did the service stop on its own (idle timeout, kernels.hip)? Then wait the few microseconds until the kernel is gone.
// With `gate` (a round is about to be enqueued) also settle an ANNOUNCED stop: the caller has bumped heartbeat and round
// count before coming here, so the service either withdraws or commits within a PCIe round trip.
int ring_service_check(pbsgpu_ring *r, bool gate) {
    if (r->svc != SvcState::Running) return PBSGPU_OK;
    volatile uint32_t *hb = hb_words(r);
    if (gate && hb[pbsk::kHbIntent] != 0 && hb[pbsk::kHbCommitted] == 0) {
        const double t0 = now_ms();
        while (hb[pbsk::kHbIntent] != 0 && hb[pbsk::kHbCommitted] == 0) {
            if (now_ms() - t0 > 5000.0) return r->error = PBSGPU_E_STATE;  // neither withdrawn nor committed: the device is gone
            std::this_thread::yield();
        }
    }
    if (hb[pbsk::kHbCommitted] != 0) {
        std::atomic_thread_fence(std::memory_order_acquire);
        HIPCHK(hipStreamSynchronize(r->ss));
        ring_service_ended(r);
    }
    return PBSGPU_OK;
}

// every ring call: tell the service the host is alive
void ring_heartbeat(pbsgpu_ring *r) {
    volatile uint32_t *hb = hb_words(r);
    hb[pbsk::kHbBeat] = hb[pbsk::kHbBeat] + 1u;
}

// pages the service has handed back since the last call
void ring_reap_free(pbsgpu_ring *r) {
    volatile unsigned long long *f = r->free_fifo.as<volatile unsigned long long>();
    for (;;) {
        const unsigned long long e = f[r->free_read & (r->nfree - 1)];
        if ((uint32_t)(e >> 32) != r->free_read + 1u) break;
        if (r->hold) r->held.handed_back((uint32_t)e, r->free_pages);  // (free only once its stream has released it)
        else r->free_pages.push_back((uint32_t)e);
        r->free_read++;
        r->st.pages_recycled++;
    }
}

// round results in order: record cells to their streams, finished streams, input tables reusable
void ring_reap_rounds(pbsgpu_ring *r) {
    for (auto &ri : r->rounds) {
        if (ri.reaped) continue;
        volatile pbsk::RingRoundStatus *hs = r->in_status(ri.input);
        if (hs->seq != ri.seq) break;  // rounds complete in order
        std::atomic_thread_fence(std::memory_order_acquire);
        if (hs->error) {
            r->error = PBSGPU_E_STATE;  // record / cell capacity of a round exceeded: the ring's own bound was wrong
        } else {
            const uint32_t n = hs->nrec;
            const uint8_t *cells = r->cells.as<uint8_t>();
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t c = (uint32_t)((ri.cell_base + i) & (r->ncells - 1));
                const uint32_t *cw = reinterpret_cast<const uint32_t *>(cells + (size_t)c * pbsk::kCellBytes);
                if (cw[pbsk::kCellSize] == 0) continue;  // the round's open chunk: no record
                const uint32_t slot = cw[pbsk::kCellSegment];
                if (slot >= r->slots.size()) continue;
                r->slots[slot].cells.push_back(CellRef{c, ri.seq});
                ri.live_cells++;
                r->st.chunks++;
                const uint32_t size = cw[pbsk::kCellSize];
                r->obs_bytes += (double)size;
                if (r->long_bytes && size >= r->long_bytes) r->obs_long_bytes += (double)size;
            }
            r->st.candidates += hs->ncand;
            r->pub_positions += (uint32_t)(hs->tail - r->tail_seen);
            r->pub_bytes += ri.new_bytes;
            r->tail_seen = hs->tail;
            for (int i = 0; i < 6; ++i) r->probe_seen[i] = hs->probe[i];
            r->probe_seen_valid = true;
            {   // the control kernel's phase times, summed per round size class (pbsgpu_ring_debug): small (< 100 pages) / large rounds
                const int cls = ri.new_bytes < 100ull * r->page_bytes ? 0 : 1;
                for (int i = 0; i < 5; ++i) r->ctl_phase_ticks[cls][i] += hs->phase_ticks[i];
                r->ctl_phase_rounds[cls]++;
            }
        }
        for (uint32_t s : ri.finals) r->slots[s].final_done = true;
        r->inflight_bytes -= ri.new_bytes;
        ri.reaped = true;
        r->input_busy[ri.input] = false;
        r->st.rounds_done++;
    }
    while (!r->rounds.empty() && r->rounds.front().reaped && r->rounds.front().live_cells == 0) r->rounds.pop_front();
}

// the pair service on `ss` and, when the ring has one, the express service on `xs`; ev_svc1 = BOTH have ended
int ring_launch_services(pbsgpu_ring *r) {
    HIPCHK(hipStreamWaitEvent(r->ss, r->ev_reset, 0));  // (never recorded before the first launch: no wait)
    HIPCHK(hipEventRecord(r->ev_svc0, r->ss));
    HIPCHK(pbsk::launch_ring_service(r->source(), r->sha_cus, r->ss, r->dense_service));
    if (r->xp_cus) {
        HIPCHK(hipStreamWaitEvent(r->xs, r->ev_reset, 0));
        HIPCHK(pbsk::launch_ring_service_xp(r->source(), r->xp_cus, r->xs));
        HIPCHK(hipEventRecord(r->ev_xsvc1, r->xs));
        HIPCHK(hipStreamWaitEvent(r->ss, r->ev_xsvc1, 0));
    }
    if (r->lanes_cus) {
        HIPCHK(hipStreamWaitEvent(r->ls, r->ev_reset, 0));
        HIPCHK(pbsk::launch_ring_service_lanes(r->source(), r->lanes_cus, r->ls, r->dense_lanes));
        HIPCHK(hipEventRecord(r->ev_lsvc1, r->ls));
        HIPCHK(hipStreamWaitEvent(r->ss, r->ev_lsvc1, 0));
    }
    HIPCHK(hipEventRecord(r->ev_svc1, r->ss));
    return PBSGPU_OK;
}

// The pair / express split follows the data (pbsp::adapt_xp_cus). Called when a service starts: the observation window is
// what was published since the last decision (at least 8 GiB), halved afterwards so that the split follows the data with
// some memory.
void ring_adapt_split(pbsgpu_ring *r) {
    if (!r->split_auto || r->xs == nullptr || r->long_bytes == 0 || r->obs_bytes < 8.0 * 1073741824.0) return;
    const uint32_t xp = pbsp::adapt_xp_cus(r->obs_long_bytes / r->obs_bytes, r->svc_cus, r->xp_cus);
    r->obs_bytes *= 0.5;
    r->obs_long_bytes *= 0.5;
    if (xp == r->xp_cus) return;
    r->xp_cus = xp;
    r->sha_cus = r->svc_cus - r->xp_cus - r->lanes_cus;
    r->st.sha_cus = r->sha_cus;
    if (r->backlog_auto) r->backlog_limit = pbsp::backlog_auto_bytes(r->sha_cus, r->lanes_cus);
}

// (`force`: quiesce / destroy — the caller is about to wait for the queue to drain, a service must run now)
int ring_start_service(pbsgpu_ring *r, bool force = false) {
    if (r->svc == SvcState::Running) return PBSGPU_OK;
    if (r->svc == SvcState::Stopping && r->parked_for_flush) {
        // parked because memory waits in the device's graveyard for the services to END: a new launch queued right behind
        // the old one would keep the device's service count above zero for ever — wait for the old one (at most the chain
        // of the chunks its lanes hold, ~0.5 s; a rare memory-pressure event), let the frees happen, then start afresh
        HIPCHK(hipStreamSynchronize(r->ss));
        ring_service_ended(r);
    }
    const uint32_t park_gen = service_park_generation(r->eng->device);
    if (r->svc == SvcState::Stopped && !force && park_gen != 0 && park_gen != r->park_grace_gen) {
        // The park request is STILL pending: other rings of the device (the stream writer's engine ring beside a bulk ring,
        // two engines) have not let go of their services yet. Starting ours now would put the device's service count back
        // before theirs has dropped — with several busy rings the count then never reaches zero, nothing is ever freed and
        // every ring pays its restart stall for nothing (round 5's cap only worked with ONE ring per device). Stay stopped:
        // rounds are still cut (like the cut-ahead of a lone stream), the next pump asks again, and the last ring to end
        // flushes. Bounded, ONCE per request: a ring that is never called again (its service stops by its idle timeout, but
        // nobody observes the end — an engine a host leaked) keeps the request pending for good, and must cost every other
        // ring one grace period, not one per service start (a stream writer's ring restarts its service after every idle
        // 2 ms: the first version of this wait made a whole test suite crawl behind one leaked engine).
        const double t = now_ms();
        if (r->park_wait_t0 == 0) r->park_wait_t0 = t;
        if (t - r->park_wait_t0 < 250.0) return PBSGPU_OK;
        r->park_grace_gen = park_gen;
    }
    r->park_wait_t0 = 0;
    if (r->svc == SvcState::Stopping) {
        // parked, its end not yet observed: the new service goes behind the old one's END and a reset (its lanes may hold
        // claims beyond the tail that the reset hands out again) — all on the device, nobody waits here
        HIPCHK(hipStreamWaitEvent(r->cs, r->ev_svc1, 0));
        HIPCHK(pbsk::launch_ring_reset(r->ctl.as<pbsk::RingCtl>(), r->cs));
        HIPCHK(hipEventRecord(r->ev_reset, r->cs));
    } else {
        service_started(r->eng->device);  // (Stopped: the queue was reset when the last service ended)
    }
    r->svc = SvcState::Running;  // (from here on an error leaves a service count behind that quiesce / destroy settle)
    ring_adapt_split(r);
    r->defer_t0 = 0;
    hb_words(r)[pbsk::kHbClaim] = r->tail_seen;
    CHK(ring_launch_services(r));
    r->svc_t0 = now_ms();
    r->svc_bytes0 = r->st.bytes_enqueued - r->deferred_bytes;  // (bytes cut ahead of this launch are its work too)
    r->deferred_bytes = 0;
    r->st.service_launches++;
    return PBSGPU_OK;
}

// ---- one round, step by step (ring_enqueue_round; what each step DECIDES is in ring_plan.h) ----

struct RoundBuild {                  // a round between the gate and the launch
    uint32_t in = 0;                 // the set of input tables it is built in
    bool any_final = false;          // a stream's end is waiting
    uint32_t np = 0, ns = 0, fill_pages = 0;
    uint64_t cells_needed = 0, new_bytes = 0;
    uint64_t feed = 0;               // the engine's suggested-boundary feed when the round was gathered
    const uint64_t *sugg_dev = nullptr;
    uint32_t set = 0;                // scan set
    RoundInfo ri;
    std::vector<hipEvent_t> deps;
    std::vector<uint64_t> sugg;
};

// step 1, the gate: is there anything to cut, is it worth a round now, and is there an input table set and cell room for it?
bool round_gate(pbsgpu_ring *r, RoundBuild &b) {
    bool any = false;
    size_t ready = 0, inflight = 0;
    for (auto &s : r->slots) {
        if (!s.open) continue;
        any |= !s.ready.empty() || s.zero_final;
        b.any_final |= s.zero_final || (!s.ready.empty() && s.ready.back().final);
        ready += s.ready.size();
    }
    if (!any) return false;
    for (auto &ri : r->rounds) inflight += ri.reaped ? 0 : 1;
    if (!pbsp::round_gate(inflight, b.any_final, ready, r->min_round_pages, r->max_inflight)) return false;
    int in = -1;
    for (uint32_t i = 0; i < kRingInputs; ++i)
        if (!r->input_busy[i]) { in = (int)i; break; }
    if (in < 0) return false;
    b.in = (uint32_t)in;
    const uint64_t oldest = r->rounds.empty() ? r->cell_cursor : r->rounds.front().cell_base;
    return pbsp::cells_have_room(r->cell_cursor, oldest, r->rec_cap, r->ncells);
}

// the ready page `q` of stream slot `si` as an entry of the round's page table, in segment `seg`
pbsk::RingPage round_page(const pbsgpu_ring *r, StreamSlot &s, uint32_t si, uint32_t seg, const PageReq &q) {
    pbsk::RingPage p{};
    p.phys = q.phys;
    p.phys_off = (uint64_t)q.phys * r->stride + 128u;
    p.logical = ((uint64_t)si << pbsk::kRingOffBits) | (q.k * r->page_bytes);
    p.valid = q.valid;
    p.slot = si;
    p.seg = seg;
    p.do_fill = q.do_fill ? 1u : 0u;
    p.fill_seed = q.seed;
    p.fill_off = q.fill_off;
    p.fill_kind = q.kind;
    p.fill_tab = q.tab;
    p.fill_ntab = q.ntab;
    p.prev_phys = (q.k > 0 && s.last_phys >= 0) ? (uint32_t)s.last_phys : 0xffffffffu;
    s.last_phys = (int64_t)q.phys;
    return p;
}

// step 2: the page, segment, record-base and suggested-boundary tables from the stream slots — the only step that takes
// pages and boundaries out of them. false: nothing was taken.
bool round_gather(pbsgpu_ring *r, RoundBuild &b) {
    pbsgpu_engine *e = r->eng;
    pbsk::RingPage *pg = r->in_pages(b.in);
    pbsk::RingSeg *sg = r->in_segs(b.in);
    uint32_t *recbase = r->in_recbase(b.in);
    uint32_t *suggidx = r->in_suggidx(b.in);
    const uint32_t minsz = std::min(e->effmin, e->cfg.min);
    b.feed = e->sugg_feed.load(std::memory_order_relaxed);
    const uint64_t look = b.feed > 1 ? (uint64_t)e->cfg.max : 0;  // reader-buffer rule: boundaries just beyond the bytes matter too
    uint32_t streams_waiting = 0;
    for (auto &s : r->slots) streams_waiting += (s.open && !s.ready.empty()) ? 1u : 0u;
    const uint32_t round_cap = pbsp::round_cap(r->svc == SvcState::Stopped, streams_waiting, r->round_pages, r->min_round_pages);
    for (uint32_t si = 0; si < r->slots.size() && b.np < round_cap; ++si) {
        StreamSlot &s = r->slots[si];
        if (!s.open || (s.ready.empty() && !s.zero_final)) continue;
        pbsk::RingSeg g{};
        g.slot = si;
        g.first_page = b.np;
        g.reset = s.fresh ? 1u : 0u;
        g.origin = s.origin;
        const uint64_t end_old = s.bytes_enqueued;
        uint64_t end = end_old;
        uint32_t take = 0;
        while (!s.ready.empty() && take < kPagesPerStreamRound && b.np < round_cap) {
            const PageReq &q = s.ready.front();
            const pbsk::RingPage p = round_page(r, s, si, b.ns, q);
            b.fill_pages += p.do_fill;
            pg[b.np++] = p;
            if (q.dep) b.deps.push_back(q.dep);
            end += q.valid;
            b.new_bytes += q.valid;
            if (q.final) g.final = 1;
            s.ready.pop_front();
            ++take;
        }
        if (s.zero_final && s.ready.empty()) {
            g.final = 1;
            s.zero_final = false;
        }
        g.npages = take;
        g.new_end = end;
        s.bytes_enqueued = end;
        s.fresh = false;
        if (g.final) {
            s.final_enqueued = true;
            b.ri.finals.push_back(si);
        }
        // suggested boundaries that can still matter: behind the open chunk's start (>= end_old - max, the chunk is
        // shorter than max), up to the new end (+ one max chunk under the reader-buffer rule)
        suggidx[b.ns] = (uint32_t)b.sugg.size();
        {
            const uint64_t lower = end_old > e->cfg.max ? end_old - e->cfg.max : 0;
            while (!s.sugg.empty() && s.sugg.front() < lower) s.sugg.pop_front();
            for (uint64_t x : s.sugg) {
                if (x > end + look) break;
                b.sugg.push_back(x);
            }
        }
        recbase[b.ns] = (uint32_t)b.cells_needed;
        b.cells_needed += pbsp::seg_cell_bound(take, r->page_bytes, e->cfg.max, minsz);
        sg[b.ns++] = g;
    }
    if (b.ns == 0) return false;
    suggidx[b.ns] = (uint32_t)b.sugg.size();
    if (b.cells_needed > r->rec_cap) b.cells_needed = r->rec_cap;  // (the bound above is never larger: pbsp::round_rec_cap)
    recbase[b.ns] = (uint32_t)b.cells_needed;
    return true;
}

// From round_gather on the popped pages and the streams' new lengths exist only in the round: any failure is the ring's (sticky).
int round_fail(pbsgpu_ring *r, RoundBuild &b, int st) {
    r->error = st;
    for (hipEvent_t ev : b.deps) ring_event_put(r, ev);
    return st;
}

// the round's suggested boundaries where the device reads them, its record cells (cleared), its number and status block
int round_claim(pbsgpu_ring *r, RoundBuild &b) {
    if (!b.sugg.empty()) {
        PinnedBuf &sb = r->sugg_in[b.in];
        if (sb.ensure(std::max<size_t>(b.sugg.size() * 8, 4096)) != PBSGPU_OK) return PBSGPU_E_NOMEM;
        std::memcpy(sb.p, b.sugg.data(), b.sugg.size() * 8);
        b.sugg_dev = sb.as<uint64_t>();
    }
    b.ri.cell_base = r->cell_cursor;
    b.ri.cell_cap = (uint32_t)b.cells_needed;
    r->cell_cursor += b.cells_needed;
    uint8_t *cells = r->cells.as<uint8_t>();
    for (uint64_t i = 0; i < b.cells_needed; ++i)
        std::memset(cells + (size_t)((b.ri.cell_base + i) & (r->ncells - 1)) * pbsk::kCellBytes, 0, pbsk::kCellBytes);
    b.ri.seq = r->next_seq++;
    b.ri.input = b.in;
    r->in_status(b.in)->seq = 0;
    return PBSGPU_OK;
}

// step 3: what the round's kernels are launched with
void round_params(pbsgpu_ring *r, RoundBuild &b, pbsk::RingRound &rr) {
    pbsgpu_engine *e = r->eng;
    rr.arena = r->arena.as<uint8_t>();
    rr.page_bytes = (uint32_t)r->page_bytes;
    rr.stride = (uint32_t)r->stride;
    rr.tile_bytes = r->tile_bytes;
    rr.tpp = r->tpp;
    rr.effmin = e->effmin;
    rr.cmin = e->cfg.min;
    rr.maxsz = e->cfg.max;
    rr.cap = r->cap;
    rr.thr = e->thr;
    rr.table_rot = e->d_table_rot;
    rr.pages = r->in_pages(b.in);
    rr.npages = b.np;
    rr.segs_in = r->in_segs(b.in);
    rr.nseg = b.ns;
    rr.seq = b.ri.seq;
    rr.cell_base = (uint32_t)(b.ri.cell_base & (r->ncells - 1));
    rr.cell_cap = b.ri.cell_cap;
    rr.cell_mask = r->ncells - 1;
    rr.status = r->in_status(b.in);
    rr.streams = r->streams.as<pbsk::RingStreamState>();
    rr.q = r->source();
    rr.desc_w = r->desc.as<uint4>();
    rr.ldesc_w = r->ldesc.as<uint4>();
    rr.sdesc_w = r->lanes_cus ? r->sdesc.as<uint4>() : nullptr;
    b.set = r->ps ? r->scan_set : 0u;
    rr.scalars = r->scalars.as<uint32_t>();
    rr.tile_queue = r->tileq.as<unsigned long long>() + b.set * 8u;
    rr.fill_queue = r->tileq.as<unsigned long long>() + 16u + b.in;
    rr.tile_cnt = b.set ? r->tile_cnt2.as<uint32_t>() : r->tile_cnt.as<uint32_t>();
    rr.tile_off = r->tile_off.as<uint32_t>();
    rr.tile_slots = b.set ? r->tile_slots2.as<uint32_t>() : r->tile_slots.as<uint32_t>();
    rr.scan_tmp = r->scan_tmp.as<uint32_t>();
    rr.dense = r->dense.as<uint64_t>();
    rr.dense_cap = r->dense_cap;
    rr.segs = r->segs.as<pbsgpu_segment>();
    rr.seg_cnt = r->seg_cnt.as<uint32_t>();
    rr.seg_off = r->seg_off.as<uint32_t>();
    rr.recs = r->recs.as<pbsgpu_record>();
    rr.rec_cap = r->rec_cap;
    rr.seg_newc = r->seg_newc.as<uint64_t>();
    rr.seg_open = r->seg_open.as<uint32_t>();
    rr.seg_ecand_in = r->seg_ecand_in.as<uint64_t>();
    rr.seg_ecand = r->seg_ecand.as<uint64_t>();
    rr.sugg = b.sugg_dev;
    rr.sugg_idx = b.sugg_dev ? r->in_suggidx(b.in) : nullptr;
    rr.sugg_feed = b.feed;
    rr.sugg_abs = e->sugg_feed_abs.load(std::memory_order_relaxed);
    rr.seg_rec_base = r->in_recbase(b.in);
}

// step 4, second half: start the service with this round, or cut ahead of it (pbsp::defer_decision)
int round_service(pbsgpu_ring *r, const RoundBuild &b, pbsk::RingRound &rr) {
    const double t = now_ms();
    const pbsp::DeferDecision d = pbsp::defer_decision(
        r->defer_service, r->svc == SvcState::Stopped, r->lone_defer_ms, b.any_final, b.np, r->round_pages, r->sha_cus,
        r->dense_service, r->eng->cfg.avg, r->deferred_bytes + b.new_bytes, r->defer_t0 == 0 ? 0.0 : t - r->defer_t0);
    if (d.timed && r->defer_t0 == 0) r->defer_t0 = t;
    if (!d.defer) {
        CHK(ring_start_service(r));
        // the start may have moved the pair / express split (ring_adapt_split): this round publishes against the split it
        // will be served by, not the one before it (xp_pairs, long_spill, long_lo: heuristics only, records do not depend on them)
        rr.q = r->source();
    }
    if (r->svc == SvcState::Stopped) r->deferred_bytes += b.new_bytes;  // cut ahead of the service (or the start waits for a graveyard flush)
    return PBSGPU_OK;
}

// step 5: the cut side's partition, the waits, the staging of the tables and the launch
int round_launch(pbsgpu_ring *r, RoundBuild &b, pbsk::RingRound &rr) {
    if (b.fill_pages) r->rounds_since_fill = 0;
    else if (r->rounds_since_fill < 1000u) r->rounds_since_fill++;
    const pbsp::CutPartition cp = pbsp::cut_partition(r->svc == SvcState::Stopped, r->eng->num_cus, r->svc_cus, r->ps != nullptr,
                                                      r->opt_fill_cus, r->fill_serial, r->rounds_since_fill);
    rr.scan_blocks = cp.scan_blocks;
    rr.fill_blocks = cp.fill_blocks;
    rr.fill_shared = cp.fill_shared ? 1u : 0u;
    hipStream_t scan_st = r->ps ? r->ps : r->cs;
    for (hipEvent_t ev : b.deps)  // host-fed pages: the cut waits for their copies (device-side wait; the copies never wait for a kernel)
        HIPCHK(hipStreamWaitEvent(scan_st, ev, 0));
    for (hipEvent_t ev : b.deps) ring_event_put(r, ev);
    b.deps.clear();
    if (r->ps && r->ctl_used[b.set])  // this scan set's previous user must have been resolved before the scan overwrites it
        HIPCHK(hipStreamWaitEvent(r->ps, r->ev_ctl[b.set], 0));
    pbsk::RingStage stg{};
    if (r->stage_inputs) {
        const uint8_t *hb = r->in(b.in);
        uint8_t *db = r->in_dev(b.in);
        stg.src = hb;
        stg.dst = db;
        stg.off[0] = (uint32_t)r->in_pages_off;   stg.len[0] = b.np * (uint32_t)sizeof(pbsk::RingPage);
        stg.off[1] = (uint32_t)r->in_segs_off;    stg.len[1] = b.ns * (uint32_t)sizeof(pbsk::RingSeg);
        stg.off[2] = (uint32_t)r->in_recbase_off; stg.len[2] = (b.ns + 1u) * 4u;
        stg.off[3] = (uint32_t)r->in_suggidx_off; stg.len[3] = rr.sugg_idx ? (b.ns + 1u) * 4u : 0u;
        stg.pages_host = rr.pages;
        auto mirror = [&](const void *hp) { return db + (reinterpret_cast<const uint8_t *>(hp) - hb); };
        rr.pages = reinterpret_cast<const pbsk::RingPage *>(mirror(rr.pages));
        rr.segs_in = reinterpret_cast<const pbsk::RingSeg *>(mirror(rr.segs_in));
        rr.seg_rec_base = reinterpret_cast<const uint32_t *>(mirror(rr.seg_rec_base));
        if (rr.sugg_idx) rr.sugg_idx = reinterpret_cast<const uint32_t *>(mirror(rr.sugg_idx));
    }
    HIPCHK(pbsk::launch_ring_round(rr, r->eng->num_cus, r->cs, cp.fill_serial ? nullptr : r->fs, r->ev_fill[b.in], r->ps,
                                   r->ps ? r->ev_scan[b.in] : nullptr, r->stage_inputs ? &stg : nullptr));
    if (r->ps) {
        HIPCHK(hipEventRecord(r->ev_ctl[b.set], r->cs));
        r->ctl_used[b.set] = true;
        r->scan_set ^= 1u;
    }
    return PBSGPU_OK;
}

// build + enqueue one round from the committed pages; *did = false when there is nothing to do or no room
int ring_enqueue_round(pbsgpu_ring *r, bool *did) {
    *did = false;
    if (r->error != PBSGPU_OK) return r->error;
    RoundBuild b;
    if (!round_gate(r, b) || !round_gather(r, b)) return PBSGPU_OK;
    int st = round_claim(r, b);
    if (st != PBSGPU_OK) return round_fail(r, b, st);
    // step 4, first half: the service's self-stop handshake (kernels.hip): count and heartbeat first, THEN look at its intent flag
    hb_words(r)[pbsk::kHbRoundsEnq] = ++r->rounds_enq;
    ring_heartbeat(r);
    std::atomic_thread_fence(std::memory_order_seq_cst);
    st = ring_service_check(r, true);
    if (st != PBSGPU_OK) return round_fail(r, b, st);
    pbsk::RingRound rr{};
    round_params(r, b, rr);
    std::atomic_thread_fence(std::memory_order_release);
    st = round_service(r, b, rr);
    if (st == PBSGPU_OK) st = round_launch(r, b, rr);
    if (st != PBSGPU_OK) return round_fail(r, b, st);
    // step 6: the bookkeeping
    r->input_busy[b.in] = true;
    b.ri.new_bytes = b.new_bytes;
    r->ready_bytes -= b.new_bytes;
    r->inflight_bytes += b.new_bytes;
    r->rounds.push_back(std::move(b.ri));
    r->st.rounds++;
    r->st.bytes_enqueued += b.new_bytes;
    r->st.pages_enqueued += b.np;
    *did = true;
    return PBSGPU_OK;
}

int ring_take_page(pbsgpu_ring *r, uint32_t *phys) {
    if (r->backlog_limit && r->svc == SvcState::Running) {
        // published and unclaimed: queue tail of the last reaped round minus the service's claim progress (a word of the
        // heartbeat block, written whenever the head crosses a multiple of 256 — hence the slack: idle lanes claim ahead
        // of the tail, so with nothing left to claim the difference always falls below 256)
        const int32_t behind = (int32_t)(r->tail_seen - hb_words(r)[pbsk::kHbClaim]) - 256;
        double wait = (double)r->ready_bytes + (double)r->inflight_bytes;
        if (behind > 0 && r->pub_positions) wait += (double)behind * ((double)r->pub_bytes / (double)r->pub_positions);
        if (wait > (double)r->backlog_limit) return PBSGPU_E_BUSY;
    }
    if (r->free_pages.empty()) ring_reap_free(r);
    if (r->free_pages.empty()) return PBSGPU_E_BUSY;
    *phys = r->free_pages.back();
    r->free_pages.pop_back();
    return PBSGPU_OK;
}

// DEBUG overrides of pbsgpu_ring_options by environment: the variable names of rounds 3-5, ONE table, one getenv. What a
// host passes in the options is what counts (two engines of one process may want different rings); these exist so that an
// unmodified binary can be A/B-tested (scripts/, the parity tests that force a code path).
void ring_env_overrides(pbsgpu_ring_options &o) {
    enum Kind { U32, U32_ZERO_OFF, U64, F64, F64_ZERO_NEG, FLAG_IF_ZERO, FLAG_IF_SET };
    struct Entry {
        const char *name;
        Kind kind;
        void *field;
        uint32_t flag;
    };
    const Entry table[] = {
        {"PBSGPU_RING_SHA_CUS", U32, &o.sha_cus, 0},
        {"PBSGPU_RING_XP_CUS", U32_ZERO_OFF, &o.express_cus, 0},
        {"PBSGPU_RING_LANES_CUS", U32, &o.lanes_cus, 0},
        {"PBSGPU_RING_SHORT_BYTES", U64, &o.short_bytes, 0},
        {"PBSGPU_RING_ROUND_PAGES", U32, &o.round_pages, 0},
        {"PBSGPU_RING_MIN_ROUND_PAGES", U32, &o.min_round_pages, 0},
        {"PBSGPU_RING_MAX_INFLIGHT", U32, &o.max_inflight, 0},
        {"PBSGPU_RING_FILL_CUS", U32, &o.fill_cus, 0},
        {"PBSGPU_RING_LONG_BYTES", U32_ZERO_OFF, &o.long_bytes, 0},
        {"PBSGPU_RING_LONG_LO_BYTES", U32_ZERO_OFF, &o.long_lo_bytes, 0},
        {"PBSGPU_RING_LONG_SPILL", U32, &o.long_spill, 0},
        {"PBSGPU_RING_POLL_EVERY", U32, &o.poll_every, 0},
        {"PBSGPU_RING_BACKLOG_MIB", F64_ZERO_NEG, &o.backlog_mib, 0},
        {"PBSGPU_RING_LONE_DEFER_MS", F64_ZERO_NEG, &o.lone_defer_ms, 0},
        {"PBSGPU_RING_IDLE_TIMEOUT_S", F64, &o.idle_timeout_s, 0},
        {"PBSGPU_RING_AUTOPARK_MS", F64, &o.autopark_ms, 0},
        {"PBSGPU_RING_OVERLAP", FLAG_IF_ZERO, &o.flags, PBSGPU_RING_F_NO_OVERLAP},
        {"PBSGPU_RING_STAGE_INPUTS", FLAG_IF_ZERO, &o.flags, PBSGPU_RING_F_NO_STAGE},
        {"PBSGPU_RING_CUT_PRIO", FLAG_IF_ZERO, &o.flags, PBSGPU_RING_F_NO_CUT_PRIO},
        {"PBSGPU_RING_SPLIT_AUTO", FLAG_IF_ZERO, &o.flags, PBSGPU_RING_F_NO_SPLIT_AUTO},
        {"PBSGPU_RING_DEFER_SERVICE", FLAG_IF_SET, &o.flags, PBSGPU_RING_F_DEFER_SERVICE},
        {"PBSGPU_RING_FILL_SERIAL", FLAG_IF_SET, &o.flags, PBSGPU_RING_F_FILL_SERIAL},
        {"PBSGPU_RING_DENSE_SERVICE", FLAG_IF_SET, &o.flags, PBSGPU_RING_F_DENSE_SERVICE},
        {"PBSGPU_RING_DENSE_LANES", FLAG_IF_SET, &o.flags, PBSGPU_RING_F_DENSE_LANES},
        {"PBSGPU_RING_TIER_TAG", FLAG_IF_SET, &o.flags, PBSGPU_RING_F_TIER_TAG},
    };
    for (const Entry &e : table) {
        const char *v = getenv(e.name);
        if (!v || !*v) continue;
        switch (e.kind) {
        case U32: *static_cast<uint32_t *>(e.field) = (uint32_t)std::max(0L, atol(v)); break;
        case U32_ZERO_OFF: *static_cast<uint32_t *>(e.field) = atol(v) <= 0 ? PBSGPU_RING_OFF : (uint32_t)atol(v); break;
        case U64: *static_cast<uint64_t *>(e.field) = strtoull(v, nullptr, 10); break;
        case F64: *static_cast<double *>(e.field) = std::max(0.0, atof(v)); break;
        case F64_ZERO_NEG: *static_cast<double *>(e.field) = atof(v) <= 0.0 ? -1.0 : atof(v); break;
        case FLAG_IF_ZERO: if (atoi(v) == 0) *static_cast<uint32_t *>(e.field) |= e.flag; break;
        case FLAG_IF_SET: if (atoi(v) != 0) *static_cast<uint32_t *>(e.field) |= e.flag; break;
        }
    }
}

}  // namespace

pbsk::RingSource pbsgpu_ring::source() const {
    pbsk::RingSource q{};
    q.desc = desc.as<uint4>();
    q.qmask = qslots - 1;
    q.probe = probe.as<unsigned long long>();
    q.ldesc = ldesc.as<uint4>();
    q.lmask = lslots - 1;
    q.long_bytes = long_bytes;
    q.sdesc = sdesc.as<uint4>();
    q.smask = sslots ? sslots - 1 : 0;
    q.short_bytes = lanes_cus ? short_bytes : 0u;
    q.xp = xp_cus ? 1u : 0u;
    const pbsp::QueuePolicy pol = pbsp::queue_policy({lanes_cus, xp_cus, dense_lanes, long_lo_auto, long_bytes, opt_long_lo,
                                                      opt_long_spill, opt_poll_every, idle_timeout_s, eng->cfg.max,
                                                      std::min(eng->effmin, eng->cfg.min)});
    q.short_room = pol.short_room;
    q.xp_pairs = pol.xp_pairs;
    q.long_spill = pol.long_spill;
    q.long_lo = pol.long_lo;
    q.idle_ticks = pol.idle_ticks;
    q.poll_mask = pol.poll_mask;
    q.ctl = ctl.as<pbsk::RingCtl>();
    q.cells = cells.as<uint8_t>();
    q.pending = pending.as<uint32_t>();
    q.free_fifo = free_fifo.as<unsigned long long>();
    q.free_mask = nfree - 1;
    q.heartbeat = heartbeat.as<uint32_t>();
    return q;
}

namespace pbse {

// records of one stream that are ready, in order, into out[*n ..)
void ring_pop_records(pbsgpu_ring *r, uint32_t slot, pbsgpu_record *out, uint64_t cap, uint64_t *n) {
    StreamSlot &s = r->slots[slot];
    const uint8_t *cells = r->cells.as<uint8_t>();
    while (*n < cap && !s.cells.empty()) {
        const CellRef cr = s.cells.front();
        const uint8_t *c = cells + (size_t)cr.cell * pbsk::kCellBytes;
        const volatile uint32_t *cw = reinterpret_cast<const volatile uint32_t *>(c);
        if (cw[pbsk::kCellFlag] != 1u) break;  // its chunk is still being hashed: records come out in stream order
        std::atomic_thread_fence(std::memory_order_acquire);
        pbsgpu_record rec;
        std::memcpy(&rec, c, sizeof(rec));
        rec.segment = slot;
        if (r->tier_tag) rec.segment |= (cw[pbsk::kCellTier] & 3u) << 28;  // PBSGPU_RING_F_TIER_TAG
        out[(*n)++] = rec;
        s.cells.pop_front();
        s.records_out++;
        s.polled_end = rec.end;
        for (auto &ri : r->rounds)
            if (ri.seq == cr.round_idx) {
                ri.live_cells--;
                break;
            }
    }
}

int ring_event_get(pbsgpu_ring *r, hipEvent_t *ev) {
    if (!r->ev_pool.empty()) {
        *ev = r->ev_pool.back();
        r->ev_pool.pop_back();
        return PBSGPU_OK;
    }
    HIPCHK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    return PBSGPU_OK;
}

void ring_event_put(pbsgpu_ring *r, hipEvent_t ev) {
    if (ev) r->ev_pool.push_back(ev);
}

bool ring_idle(const pbsgpu_ring *r) {
    if (!r->rounds.empty() || r->ready_bytes || r->inflight_bytes) return false;
    for (auto &s : r->slots)
        if (s.open && (!s.ready.empty() || s.zero_final || !s.cells.empty())) return false;
    return true;
}

// Stop the service behind everything enqueued so far without waiting for it: the kernel drains what is published and
// ends; the next round starts a new one (which first waits, on the device, for the old one's end).
int ring_park(pbsgpu_ring *r) {
    if (r->svc != SvcState::Running) return PBSGPU_OK;
    CHK(ring_service_check(r, false));
    if (r->svc != SvcState::Running) return PBSGPU_OK;
    HIPCHK(pbsk::launch_ring_stop(r->ctl.as<pbsk::RingCtl>(), r->cs));
    r->svc = SvcState::Stopping;
    return PBSGPU_OK;
}

int ring_commit_dep(pbsgpu_ring *r, uint32_t stream, uint64_t nbytes, int final, hipEvent_t dep) {
    if (!r || stream >= r->slots.size() || !r->slots[stream].open) return PBSGPU_E_INVALID;
    StreamSlot &s = r->slots[stream];
    if (s.final_committed) return PBSGPU_E_STATE;
    if (nbytes > r->page_bytes || (nbytes != r->page_bytes && !final)) return PBSGPU_E_INVALID;  // only a stream's last page is short
    if (s.bytes_committed + nbytes > pbsk::kRingMaxStream) return PBSGPU_E_INVALID;  // 4 PiB per stream (52-bit logical offsets)
    if (nbytes == 0) {
        if (s.reserved >= 0) {  // nothing written: the page goes back
            r->free_pages.push_back((uint32_t)s.reserved);
            s.reserved = -1;
        }
        s.zero_final = true;
        s.final_committed = true;
        return PBSGPU_OK;
    }
    if (s.reserved < 0) return PBSGPU_E_STATE;
    PageReq q;
    q.phys = (uint32_t)s.reserved;
    q.k = s.next_k++;
    q.valid = (uint32_t)nbytes;
    q.final = final != 0;
    q.dep = dep;
    if (r->hold) {
        if (s.holding) r->held.assign(stream, q.k, q.phys);
        else r->held.unowned(q.phys);  // (a section of a payload stream that does not hold: free at hand-back, as without the flag)
    }
    s.ready.push_back(q);
    r->ready_bytes += nbytes;
    s.reserved = -1;
    s.bytes_committed += nbytes;
    if (final) s.final_committed = true;
    return PBSGPU_OK;
}

int ring_open_hold(pbsgpu_ring *r, uint32_t *stream, bool hold) {
    CHK(pbsgpu_ring_open(r, stream));
    r->slots[*stream].holding = hold;
    return PBSGPU_OK;
}

bool ring_page_needs_release(pbsgpu_ring *r) {
    if (!r->hold) return false;
    ring_reap_free(r);
    return r->free_pages.empty() && !r->held.frees_without_release();
}

// creation step 1: the ring's shape (pbsp::shape_ring) and the options that are only carried along
static int ring_shape(pbsgpu_ring *r, const pbsgpu_ring_options &o, uint32_t long_bytes_hint) {
    pbsgpu_engine *e = r->eng;
    size_t fr = 0, tot = 0;
    if (o.arena_bytes == 0) HIPCHK(hipMemGetInfo(&fr, &tot));
    CHK(pbsp::shape_ring(o, {e->cfg.min, e->effmin, e->cfg.avg, e->cfg.max, e->cfg.mask}, e->num_cus, fr, long_bytes_hint,
                         kRingInputs, r));
    r->autopark_ms = std::max(0.0, o.autopark_ms);
    r->idle_timeout_s = o.idle_timeout_s;
    r->opt_long_lo = o.long_lo_bytes;
    r->opt_long_spill = o.long_spill;
    r->opt_poll_every = o.poll_every;
    r->opt_fill_cus = o.fill_cus;
    // PBSGPU_RING_F_NO_STAGE: the round's kernels read their tables from mapped host memory (rounds 3-4), for A/B runs
    r->stage_inputs = !(o.flags & PBSGPU_RING_F_NO_STAGE);
    return PBSGPU_OK;
}

// creation step 2: every buffer of the shape, and the layout of the round input tables
static int ring_allocate(pbsgpu_ring *r, bool overlap) {
    const uint64_t ntiles = r->ntiles;
    CHK(r->arena.ensure((size_t)r->npages * r->stride + 512));
    CHK(r->ctl.ensure(256));
    CHK(r->probe.ensure(128));
    CHK(r->streams.ensure((size_t)r->max_streams * sizeof(pbsk::RingStreamState)));
    CHK(r->pending.ensure((size_t)r->npages * 4 + 64));
    CHK(r->desc.ensure((size_t)r->qslots * 32));
    CHK(r->ldesc.ensure((size_t)r->lslots * 32));
    CHK(r->sdesc.ensure((size_t)r->sslots * 32));
    CHK(r->scalars.ensure(pbsk::kRsCount * 4 + 64));
    CHK(r->tile_cnt.ensure((size_t)ntiles * 4 + 16));
    CHK(r->tile_off.ensure((size_t)ntiles * 4 + 16));
    CHK(r->tile_slots.ensure((size_t)ntiles * r->cap * 4 + 16));
    CHK(r->tileq.ensure(128 + kRingInputs * 8));  // two tile counters (64 bytes apart), then one refill counter per round in flight
    if (overlap) {
        CHK(r->tile_cnt2.ensure((size_t)ntiles * 4 + 16));
        CHK(r->tile_slots2.ensure((size_t)ntiles * r->cap * 4 + 16));
    }
    CHK(r->dense.ensure((size_t)r->dense_cap * 8 + 16));
    CHK(r->scan_tmp.ensure(pbsk::scan_tmp_words(std::max<uint64_t>(ntiles, r->max_streams)) * 4 + 64));
    CHK(r->segs.ensure((size_t)r->max_streams * sizeof(pbsgpu_segment)));
    CHK(r->seg_cnt.ensure((size_t)r->max_streams * 4 + 16));
    CHK(r->seg_off.ensure((size_t)r->max_streams * 4 + 16));
    CHK(r->seg_newc.ensure((size_t)r->max_streams * 8 + 16));
    CHK(r->seg_open.ensure((size_t)r->max_streams * 4 + 16));
    CHK(r->seg_ecand_in.ensure((size_t)r->max_streams * 8 + 16));
    CHK(r->seg_ecand.ensure((size_t)r->max_streams * 8 + 16));
    CHK(r->recs.ensure((size_t)r->rec_cap * sizeof(pbsgpu_record) + 64));
    CHK(r->cells.ensure((size_t)r->ncells * pbsk::kCellBytes));
    CHK(r->heartbeat.ensure(256));
    std::memset(r->heartbeat.p, 0, 256);
    CHK(r->free_fifo.ensure((size_t)r->nfree * 8));
    std::memset(r->free_fifo.p, 0, (size_t)r->nfree * 8);
    auto al64 = [](size_t v) { return (v + 63) & ~(size_t)63; };
    r->in_pages_off = 0;
    r->in_segs_off = al64((size_t)r->round_pages * sizeof(pbsk::RingPage));
    r->in_recbase_off = al64(r->in_segs_off + (size_t)r->max_streams * sizeof(pbsk::RingSeg));
    r->in_suggidx_off = al64(r->in_recbase_off + ((size_t)r->max_streams + 1) * 4);
    r->in_status_off = al64(r->in_suggidx_off + ((size_t)r->max_streams + 1) * 4);
    r->input_stride = r->in_status_off + 128;
    CHK(r->inputs.ensure(r->input_stride * kRingInputs));
    if (r->stage_inputs) CHK(r->inputs_dev.ensure(r->input_stride * kRingInputs));
    std::memset(r->inputs.p, 0, r->input_stride * kRingInputs);
    return PBSGPU_OK;
}

// creation step 3: the ring's streams and events, and the device-side state cleared
static int ring_streams_and_events(pbsgpu_ring *r, bool overlap, bool cut_prio) {
    // Three priorities: the services highest (their own hardware-queue pool: nothing may queue behind a kernel that only
    // ends on request), the CONTROL side of the rounds normal, the producers of bulk work — synthetic refill, scan —
    // lowest: the one-workgroup control kernel and its prep launch find a CU as soon as one frees up instead of waiting
    // behind the next round's scan workgroups (kernel trace of the driver's command: k_ring_prep 1.2 ms and
    // k_ring_control 1.1 ms per launch for 10 us / 170 us of work; PBSGPU_RING_CUT_PRIO=0: all normal).
    int prio_lo = 0, prio_hi = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
    r->bulk_prio = cut_prio ? prio_lo : 0;
    HIPCHK(hipStreamCreateWithFlags(&r->cs, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithPriority(&r->fs, hipStreamNonBlocking, r->bulk_prio));
    // The device-side state starts from zero — cleared ON THE CONTROL STREAM and waited for. A plain hipMemset is
    // queued on the null stream and returns at once for device memory; the ring's streams are non-blocking, i.e. not
    // ordered against the null stream: when the null stream was held up (it waits for every blocking stream's earlier
    // work, e.g. the previous engine's last kernels) the clear arrived AFTER the first rounds had run and wiped queue
    // tail, stream states and page reference counts — pages never came back, lanes waited at positions the tail had
    // been reset below (the one-in-a-few-hundred hang of the small-ring tests).
    HIPCHK(hipMemsetAsync(r->ctl.p, 0, 256, r->cs));
    HIPCHK(hipMemsetAsync(r->probe.p, 0, 128, r->cs));
    HIPCHK(hipMemsetAsync(r->streams.p, 0, (size_t)r->max_streams * sizeof(pbsk::RingStreamState), r->cs));
    HIPCHK(hipMemsetAsync(r->pending.p, 0, (size_t)r->npages * 4 + 64, r->cs));
    HIPCHK(hipMemsetAsync(r->scalars.p, 0, pbsk::kRsCount * 4 + 64, r->cs));
    HIPCHK(hipMemsetAsync(r->tileq.p, 0, 128 + kRingInputs * 8, r->cs));
    HIPCHK(hipStreamSynchronize(r->cs));
    for (auto &ev : r->ev_fill) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    if (overlap) {
        HIPCHK(hipStreamCreateWithPriority(&r->ps, hipStreamNonBlocking, r->bulk_prio));
        for (auto &ev : r->ev_scan) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        for (auto &ev : r->ev_ctl) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    // the service must never share a hardware queue with a stream that enqueues behind it (packets of one queue
    // run in order: work queued behind a kernel that only ends on request would never start). HIP keeps one queue
    // pool per priority: the service gets the highest priority to itself.
    HIPCHK(hipStreamCreateWithPriority(&r->ss, hipStreamNonBlocking, prio_hi));
    if (r->xp_cus) {
        HIPCHK(hipStreamCreateWithPriority(&r->xs, hipStreamNonBlocking, prio_hi));
        HIPCHK(hipEventCreateWithFlags(&r->ev_xsvc1, hipEventDisableTiming));
    }
    if (r->lanes_cus) {
        HIPCHK(hipStreamCreateWithPriority(&r->ls, hipStreamNonBlocking, prio_hi));
        HIPCHK(hipEventCreateWithFlags(&r->ev_lsvc1, hipEventDisableTiming));
    }
    HIPCHK(hipEventCreateWithFlags(&r->ev_reset, hipEventDisableTiming));
    HIPCHK(hipEventCreate(&r->ev_svc0));
    HIPCHK(hipEventCreate(&r->ev_svc1));
    return PBSGPU_OK;
}

int ring_create_internal(pbsgpu_engine *e, const pbsgpu_ring_options *opt, bool hold_engine_ref, pbsgpu_ring **out,
                         uint32_t long_bytes_hint) {
    if (!e || !out) return PBSGPU_E_INVALID;
    *out = nullptr;
    CHK(set_device(e));
    pbsgpu_ring_options o{};
    if (opt) o = *opt;
    ring_env_overrides(o);
    pbsgpu_ring *r = new (std::nothrow) pbsgpu_ring();
    if (!r) return PBSGPU_E_NOMEM;
    r->holds_engine_ref = hold_engine_ref;
    if (hold_engine_ref) engine_ref(e);
    r->eng = e;
    const bool overlap = !(o.flags & PBSGPU_RING_F_NO_OVERLAP);
    int st = ring_shape(r, o, long_bytes_hint);
    if (st == PBSGPU_OK) st = ring_allocate(r, overlap);
    if (st == PBSGPU_OK) st = ring_streams_and_events(r, overlap, !(o.flags & PBSGPU_RING_F_NO_CUT_PRIO));
    if (st != PBSGPU_OK) {
        pbsgpu_ring_destroy(r);
        return st;
    }
    r->slots.resize(r->max_streams);
    r->piece_tab.resize(r->max_streams);
    r->piece_n.assign(r->max_streams, 0);
    r->free_pages.reserve(r->npages);
    for (uint32_t p = r->npages; p-- > 0;) r->free_pages.push_back(p);  // page 0 is handed out first
    r->hold = (o.flags & PBSGPU_RING_F_HOLD_PAGES) != 0;
    if (r->hold) r->held.init(r->npages, r->max_streams, r->page_bytes);
    r->st.pages_total = r->npages;
    r->st.page_bytes = r->page_bytes;
    r->st.sha_cus = r->sha_cus;
    *out = r;
    return PBSGPU_OK;
}

}  // namespace pbse

extern "C" {

int pbsgpu_ring_create(pbsgpu_engine *e, const pbsgpu_ring_options *opt, pbsgpu_ring **out) {
    return ring_create_internal(e, opt, true, out);
}

// Stop the SHA service behind everything enqueued so far and wait until the device holds no ring work: every chunk of
// every enqueued round is hashed, the persistent kernel has ended (hipDeviceSynchronize / hipFree can return again).
// The next pump starts the service again.
int pbsgpu_ring_quiesce(pbsgpu_ring *r) {
    if (!r) return PBSGPU_E_INVALID;
    CHK(set_device(r->eng));
    ring_heartbeat(r);
    if (r->defer_service && r->svc == SvcState::Stopped) {
        // Profiling mode (PBSGPU_RING_DEFER_SERVICE=1; scripts/r4_ring_pmc.py): the rounds have only filled the queue. Now
        // the service runs ALONE over everything published, `stop` already raised, and ends — one ordinary dispatch that
        // rocprofv3's counter passes (which serialise dispatches) can measure: k_sha256_pair<RingSource,false> with every
        // lane busy, reading chunks that cross pages, releasing pages. (The arena must hold what was fed: no page comes
        // back before this point.)
        HIPCHK(hipStreamSynchronize(r->cs));
        HIPCHK(pbsk::launch_ring_stop(r->ctl.as<pbsk::RingCtl>(), r->cs));
        HIPCHK(hipEventRecord(r->ev_reset, r->cs));
        CHK(ring_launch_services(r));
        service_started(r->eng->device);
        r->svc = SvcState::Running;
        r->st.service_launches++;
        HIPCHK(hipStreamSynchronize(r->ss));
        ring_service_ended(r);  // (head := tail, stop := 0 for the next batch of rounds)
        HIPCHK(hipStreamSynchronize(r->cs));
        r->svc_bytes0 = r->st.bytes_enqueued;
        ring_reap_free(r);
        ring_reap_rounds(r);
        return r->error;
    }
    if (r->svc == SvcState::Stopped && r->deferred_bytes > 0) {
        // rounds were cut AHEAD of the service (a lone bulk stream on an idle ring: pbsp::defer_decision): their chunks sit in
        // the queue with no service to hash them. "Everything enqueued is hashed" needs one: start it, then stop it behind
        // what is published, like a running one (round 5; before that fill -> pump -> quiesce -> poll saw no records)
        CHK(ring_start_service(r, true));
    }
    if (r->svc == SvcState::Running) {
        CHK(ring_service_check(r, false));  // (it may have stopped on its own in the meantime)
        if (r->svc == SvcState::Running) HIPCHK(pbsk::launch_ring_stop(r->ctl.as<pbsk::RingCtl>(), r->cs));
    }
    HIPCHK(hipStreamSynchronize(r->cs));
    if (r->svc != SvcState::Stopped) {
        HIPCHK(hipStreamSynchronize(r->ss));
        HIPCHK(hipStreamSynchronize(r->fs));
        ring_service_ended(r);
    }
    ring_reap_free(r);
    ring_reap_rounds(r);
    return r->error;
}

int pbsgpu_ring_park(pbsgpu_ring *r) {
    if (!r) return PBSGPU_E_INVALID;
    CHK(set_device(r->eng));
    ring_heartbeat(r);
    CHK(ring_park(r));
    return r->error;
}

void pbsgpu_ring_destroy(pbsgpu_ring *r) {
    if (!r) return;
    pbsgpu_engine *e = r->eng;
    if (e) {
        (void)hipSetDevice(e->device);
        if (r->cs && r->ss) (void)pbsgpu_ring_quiesce(r);
        if (r->svc != SvcState::Stopped) {  // quiesce failed half-way (HIP error): the count must not leak
            r->svc = SvcState::Stopped;
            service_ended(r->eng->device);
        }
        if (r->ss) (void)hipStreamDestroy(r->ss);
        if (r->xs) (void)hipStreamDestroy(r->xs);
        if (r->ev_xsvc1) (void)hipEventDestroy(r->ev_xsvc1);
        if (r->ls) (void)hipStreamDestroy(r->ls);
        if (r->ev_lsvc1) (void)hipEventDestroy(r->ev_lsvc1);
        if (r->cs) (void)hipStreamDestroy(r->cs);
        if (r->ps) (void)hipStreamDestroy(r->ps);
        if (r->fs) (void)hipStreamDestroy(r->fs);
        for (auto ev : r->ev_scan)
            if (ev) (void)hipEventDestroy(ev);
        for (auto ev : r->ev_ctl)
            if (ev) (void)hipEventDestroy(ev);
        for (auto ev : r->ev_fill)
            if (ev) (void)hipEventDestroy(ev);
        for (hipEvent_t ev : {r->ev_reset, r->ev_svc0, r->ev_svc1})
            if (ev) (void)hipEventDestroy(ev);
        for (auto &s : r->slots)
            for (auto &q : s.ready)
                if (q.dep) r->ev_pool.push_back(q.dep);
        for (auto ev : r->ev_pool) (void)hipEventDestroy(ev);
        for (DevBuf *b : {&r->arena, &r->ctl, &r->probe, &r->streams, &r->pending, &r->desc, &r->ldesc, &r->sdesc, &r->scalars, &r->tile_cnt, &r->tile_off,
                          &r->tile_slots, &r->tile_cnt2, &r->tile_slots2, &r->tileq, &r->scan_tmp, &r->dense, &r->segs, &r->seg_cnt, &r->seg_off, &r->recs, &r->seg_newc,
                          &r->seg_open, &r->seg_ecand_in, &r->seg_ecand, &r->inputs_dev})
            b->release();
        r->cells.release();
        r->heartbeat.release();
        r->free_fifo.release();
        r->inputs.release();
        for (auto &b : r->sugg_in) b.release();
        for (auto &b : r->piece_tab) b.release();
    }
    const bool unref = r->holds_engine_ref;
    delete r;
    if (e && unref) engine_unref(e);
}

int pbsgpu_ring_open(pbsgpu_ring *r, uint32_t *stream) {
    if (!r || !stream) return PBSGPU_E_INVALID;
    for (uint32_t i = 0; i < r->slots.size(); ++i)
        if (!r->slots[i].open) {
            r->slots[i] = StreamSlot{};
            r->slots[i].open = true;
            if (r->hold) r->held.open(i);
            if (i < r->piece_n.size()) r->piece_n[i] = 0;  // (a piece table left behind by the slot's previous stream is not this one's)
            *stream = i;
            r->st.streams_opened++;
            return PBSGPU_OK;
        }
    return PBSGPU_E_BUSY;
}

int pbsgpu_ring_close(pbsgpu_ring *r, uint32_t stream) {
    if (!r || stream >= r->slots.size() || !r->slots[stream].open) return PBSGPU_E_INVALID;
    StreamSlot &s = r->slots[stream];
    if (!s.final_done || !s.cells.empty()) return PBSGPU_E_STATE;  // finish it and poll its records first
    s.open = false;
    if (r->hold) r->held.close(stream, r->free_pages);  // (what the services still have of it comes back as nobody's page)
    return PBSGPU_OK;
}

// ---- held pages: release, and the chunks' bytes while they are held (PBSGPU_RING_F_HOLD_PAGES) ----

int pbsgpu_ring_release(pbsgpu_ring *r, uint32_t stream, uint64_t upto) {
    if (!r) return PBSGPU_E_INVALID;
    if (!r->hold) return PBSGPU_E_STATE;
    if (stream >= r->slots.size() || !r->slots[stream].open) return PBSGPU_E_INVALID;
    if (upto > r->slots[stream].polled_end) return PBSGPU_E_INVALID;  // only what poll has handed out can be done with
    ring_heartbeat(r);
    r->held.release(stream, upto, r->free_pages);
    return PBSGPU_OK;
}

int pbsgpu_ring_held(pbsgpu_ring *r, uint32_t stream, uint64_t *first_offset, uint32_t *pages_held) {
    if (!r || !first_offset || !pages_held) return PBSGPU_E_INVALID;
    if (!r->hold) return PBSGPU_E_STATE;
    if (stream >= r->slots.size() || !r->slots[stream].open) return PBSGPU_E_INVALID;
    ring_reap_free(r);
    *first_offset = r->held.first_offset(stream);
    *pages_held = r->held.pages_held(stream);
    return PBSGPU_OK;
}

// stream bytes [off, off + len) -> parts of the arena, one per page touched; false when a page is no longer (or not yet) there
static bool ring_parts_of(const pbsgpu_ring *r, uint32_t stream, uint64_t off, uint64_t len, SrcPart *out, uint32_t cap,
                          uint32_t *n) {
    *n = 0;
    uint64_t k = off / r->page_bytes, in = off - k * r->page_bytes;
    for (; len; ++k, in = 0) {
        const int64_t phys = r->held.phys_of(stream, k);
        if (phys < 0 || *n == cap) return false;
        const uint64_t take = std::min<uint64_t>(len, r->page_bytes - in);
        out[(*n)++] = SrcPart{(uint64_t)phys * r->stride + 128u + in, (uint32_t)take};
        len -= take;
    }
    return true;
}

// Why the encode kernel sees the pages' bytes: a record that poll has handed out was hashed, so the service
// read its bytes — in a kernel that follows, in stream order or by event, the fill or the commit of its pages.
int pbsgpu_ring_blob_encode_device(pbsgpu_ring *r, uint32_t stream, const pbsgpu_record *recs, uint64_t n, const uint8_t *skip,
                                   void *dst, uint64_t dst_cap, uint64_t *blob_off, uint32_t *crcs, uint64_t *used) {
    if (!r || !used || (n && (!recs || !blob_off)) || n >= (1ull << 32)) return PBSGPU_E_INVALID;
    if (!r->hold) return PBSGPU_E_STATE;
    std::vector<SrcPart> parts;  // two per selected record
    std::vector<uint64_t> doff;
    std::vector<uint32_t> which;
    parts.reserve(2 * (size_t)n);
    doff.reserve((size_t)n);
    which.reserve((size_t)n);
    uint64_t total = 0, first = 0, polled = 0;
    uint32_t cur = PBSGPU_RING_ANY_STREAM;  // the stream `first` and `polled` belong to
    for (uint64_t i = 0; i < n; ++i) {
        if (skip && skip[i]) continue;
        const pbsgpu_record &rc = recs[i];
        const uint32_t sid = stream == PBSGPU_RING_ANY_STREAM ? (rc.segment & 0x0fffffffu) : stream;
        if (sid != cur) {
            if (sid >= r->slots.size() || !r->slots[sid].open) return PBSGPU_E_INVALID;
            cur = sid;
            first = r->held.first_offset(sid);
            polled = r->slots[sid].polled_end;
        }
        if (rc.size > rc.end || rc.size > r->page_bytes) return PBSGPU_E_INVALID;  // (no chunk of this ring: it would touch three pages)
        const uint64_t start = rc.end - rc.size;
        if (rc.end > polled || start < first) return PBSGPU_E_STATE;
        SrcPart two[2] = {};
        uint32_t np = 0;
        if (!ring_parts_of(r, sid, start, rc.size, two, 2, &np)) return PBSGPU_E_STATE;
        parts.push_back(two[0]);
        parts.push_back(two[1]);
        doff.push_back(total);
        which.push_back((uint32_t)i);
        total += (uint64_t)rc.size + PBSGPU_BLOB_HEADER_SIZE;
    }
    *used = total;
    if (total > dst_cap) return PBSGPU_E_CAPACITY;
    for (size_t j = 0; j < which.size(); ++j) blob_off[which[j]] = doff[j];
    if (which.empty()) return PBSGPU_OK;
    CHK(set_device(r->eng));
    if (!dst || !is_device_pointer(dst)) return PBSGPU_E_INVALID;
    ring_heartbeat(r);
    std::vector<uint32_t> got(crcs ? which.size() : 0);
    CHK(blob_encode_parts(r->eng, r->arena.as<uint8_t>(), reinterpret_cast<const SrcPart(*)[2]>(parts.data()),
                          (uint32_t)which.size(), static_cast<uint8_t *>(dst), doff.data(), crcs ? got.data() : nullptr));
    for (size_t j = 0; j < got.size(); ++j) crcs[which[j]] = got[j];
    return PBSGPU_OK;
}

// The fused form: which records are new is decided on the device, so EVERY record must be available, and
// the host's part is per stream and per page: the span of stream bytes the batch touches, then one page-table entry per
// logical page of that span. A page inside [first available offset, last polled end) is always there — pages go only
// below the release watermark, and nothing beyond a polled record is uncommitted — so the two range checks per record
// refuse what the per-record page lookup of pbsgpu_ring_blob_encode_device refuses; the lookup per page stays as the proof.
// ring_upload_plan is the host's part (the payload-stream writer runs it under the ring's lock and the device work without
// it; stream.cpp).
}  // extern "C"

int pbse::ring_upload_plan(pbsgpu_ring *r, uint32_t stream, const pbsgpu_record *recs, uint64_t n, UploadPlan *plan) {
    struct Span {
        uint64_t lo = ~0ull, hi = 0;  // stream bytes [lo, hi) hold every chunk of the batch
    };
    std::vector<Span> span(r->slots.size());
    UploadSrc &us = plan->us;
    std::vector<uint64_t> &tabs = plan->tabs;
    uint64_t first = 0, polled = 0;
    uint32_t cur = PBSGPU_RING_ANY_STREAM;
    for (uint64_t i = 0; i < n; ++i) {
        const pbsgpu_record &rc = recs[i];
        const uint32_t sid = stream == PBSGPU_RING_ANY_STREAM ? (rc.segment & 0x0fffffffu) : stream;
        if (sid != cur) {
            if (sid >= r->slots.size() || !r->slots[sid].open) return PBSGPU_E_INVALID;
            cur = sid;
            first = r->held.first_offset(sid);
            polled = r->slots[sid].polled_end;
        }
        if (rc.size > rc.end || rc.size > r->page_bytes) return PBSGPU_E_INVALID;
        const uint64_t start = rc.end - rc.size;
        if (rc.end > polled || start < first) return PBSGPU_E_STATE;
        if (rc.size == 0) continue;
        span[sid].lo = std::min(span[sid].lo, start);
        span[sid].hi = std::max(span[sid].hi, rc.end);
        us.pieces_max += ((rc.size + (1ull << kBlobPieceLog) - 1) >> kBlobPieceLog) + 1;  // (+1: a chunk in two pages)
    }
    if (us.pieces_max >= (1ull << 32)) return PBSGPU_E_INVALID;
    tabs.assign(2 * span.size(), 0);  // PageTabs, then the pages
    for (uint32_t sid = 0; sid < span.size(); ++sid) {
        if (span[sid].lo >= span[sid].hi) continue;
        const uint64_t k0 = span[sid].lo / r->page_bytes, k1 = (span[sid].hi - 1) / r->page_bytes;
        tabs[2 * sid] = k0;
        tabs[2 * sid + 1] = (uint64_t)(tabs.size() - 2 * span.size()) | (k1 - k0 + 1) << 32;
        for (uint64_t pg = k0; pg <= k1; ++pg) {
            const int64_t phys = r->held.phys_of(sid, pg);
            if (phys < 0) return PBSGPU_E_STATE;
            tabs.push_back((uint64_t)phys * r->stride + 128u);
        }
    }
    ring_heartbeat(r);
    us.base = r->arena.as<uint8_t>();
    us.tabs = tabs.data();
    us.tab_words = tabs.size();
    us.nslots = (uint32_t)span.size();
    us.stream = stream;
    us.page_bytes = r->page_bytes;
    return PBSGPU_OK;
}

int pbse::ring_copy_plan(pbsgpu_ring *r, uint32_t stream, uint64_t offset, uint64_t length, std::vector<SrcPart> *parts) {
    if (offset + length > r->slots[stream].polled_end || offset < r->held.first_offset(stream)) return PBSGPU_E_STATE;
    parts->assign((size_t)(length / r->page_bytes) + 2, SrcPart{});
    uint32_t np = 0;
    if (!ring_parts_of(r, stream, offset, length, parts->data(), (uint32_t)parts->size(), &np)) return PBSGPU_E_STATE;
    parts->resize(np);
    ring_heartbeat(r);
    return PBSGPU_OK;
}

extern "C" {

int pbsgpu_ring_upload_new2_device(pbsgpu_ring *r, pbsgpu_known *k, uint32_t stream, const pbsgpu_record *recs, uint64_t n,
                                   int insert, uint32_t flags, void *dst, uint64_t dst_cap, uint8_t *known_out,
                                   uint64_t *blob_off, uint32_t *lens, uint8_t *kinds, uint32_t *crcs, uint64_t *used,
                                   pbsgpu_dedup_stats *stats, pbsgpu_encode_stats *enc_stats) {
    if (flags & ~PBSGPU_ENCODE_F_ZSTD) return PBSGPU_E_INVALID;
    if (!r || !k || !used || !stats || (n && (!recs || !blob_off)) || n >= (1ull << 32)) return PBSGPU_E_INVALID;
    if (!dst && dst_cap) return PBSGPU_E_INVALID;
    if (!r->hold) return PBSGPU_E_STATE;
    if (known_engine(k) != r->eng) return PBSGPU_E_INVALID;
    UploadPlan plan;
    CHK(ring_upload_plan(r, stream, recs, n, &plan));
    *used = 0;
    std::memset(stats, 0, sizeof(*stats));
    if (enc_stats) std::memset(enc_stats, 0, sizeof(*enc_stats));
    if (n == 0) return PBSGPU_OK;
    CHK(set_device(r->eng));
    if (dst && !is_device_pointer(dst)) return PBSGPU_E_INVALID;
    return upload_new(k, plan.us, recs, n, insert != 0, flags, static_cast<uint8_t *>(dst), dst_cap, known_out, blob_off, lens,
                      kinds, crcs, used, stats, enc_stats);
}

int pbsgpu_ring_upload_new_device(pbsgpu_ring *r, pbsgpu_known *k, uint32_t stream, const pbsgpu_record *recs, uint64_t n,
                                  int insert, void *dst, uint64_t dst_cap, uint8_t *known_out, uint64_t *blob_off,
                                  uint32_t *crcs, uint64_t *used, pbsgpu_dedup_stats *stats) {
    return pbsgpu_ring_upload_new2_device(r, k, stream, recs, n, insert, 0, dst, dst_cap, known_out, blob_off, nullptr, nullptr,
                                          crcs, used, stats, nullptr);
}

int pbsgpu_ring_copy_device(pbsgpu_ring *r, uint32_t stream, uint64_t offset, uint64_t length, void *dst) {
    if (!r || (length && !dst)) return PBSGPU_E_INVALID;
    if (!r->hold) return PBSGPU_E_STATE;
    if (stream >= r->slots.size() || !r->slots[stream].open || offset + length < offset) return PBSGPU_E_INVALID;
    if (offset + length > r->slots[stream].polled_end || offset < r->held.first_offset(stream)) return PBSGPU_E_STATE;
    if (length == 0) return PBSGPU_OK;
    std::vector<SrcPart> parts;
    CHK(ring_copy_plan(r, stream, offset, length, &parts));
    CHK(set_device(r->eng));
    if (!is_device_pointer(dst)) return PBSGPU_E_INVALID;
    return copy_parts(r->eng, r->arena.as<uint8_t>(), parts.data(), (uint32_t)parts.size(), static_cast<uint8_t *>(dst));
}

int pbsgpu_ring_reserve(pbsgpu_ring *r, uint32_t stream, void **dptr, uint64_t *cap) {
    if (!r || !dptr || !cap || stream >= r->slots.size() || !r->slots[stream].open) return PBSGPU_E_INVALID;
    StreamSlot &s = r->slots[stream];
    if (s.final_committed || s.reserved >= 0) return PBSGPU_E_STATE;
    if (r->error != PBSGPU_OK) return r->error;
    uint32_t phys = 0;
    CHK(ring_take_page(r, &phys));
    s.reserved = phys;
    *dptr = r->arena.as<uint8_t>() + (uint64_t)phys * r->stride + 128u;
    *cap = r->page_bytes;
    return PBSGPU_OK;
}

int pbsgpu_ring_commit(pbsgpu_ring *r, uint32_t stream, uint64_t nbytes, int final) {
    return ring_commit_dep(r, stream, nbytes, final, nullptr);
}

int pbsgpu_ring_suggest(pbsgpu_ring *r, uint32_t stream, uint64_t offset) {
    if (!r || stream >= r->slots.size() || !r->slots[stream].open) return PBSGPU_E_INVALID;
    StreamSlot &s = r->slots[stream];
    if (s.final_committed) return PBSGPU_E_STATE;
    if (!s.sugg.empty() && offset < s.sugg.back()) return PBSGPU_E_INVALID;  // ascending
    // a boundary at or before bytes that are already in a round can no longer take part in those rounds' cuts: it must be
    // announced before the bytes around it are committed (the stream writer announces at the current position or ahead)
    s.sugg.push_back(offset);
    return PBSGPU_OK;
}

int pbsgpu_ring_fill(pbsgpu_ring *r, uint32_t stream, uint64_t seed, uint32_t kind, uint64_t nbytes, int final,
                     uint64_t *taken) {
    if (!r || !taken || stream >= r->slots.size() || !r->slots[stream].open || kind > 4) return PBSGPU_E_INVALID;
    StreamSlot &s = r->slots[stream];
    *taken = 0;
    if (s.final_committed || s.reserved >= 0) return PBSGPU_E_STATE;
    if (r->error != PBSGPU_OK) return r->error;
    if (s.bytes_committed + nbytes > pbsk::kRingMaxStream) return PBSGPU_E_INVALID;
    if (nbytes == 0) {
        if (final) {
            s.zero_final = true;
            s.final_committed = true;
        }
        return PBSGPU_OK;
    }
    while (*taken < nbytes) {
        const uint64_t n = std::min<uint64_t>(r->page_bytes, nbytes - *taken);
        const bool last = (*taken + n == nbytes);
        if (n < r->page_bytes && !(last && final)) break;  // a short page only as the stream's last one
        uint32_t phys = 0;
        if (ring_take_page(r, &phys) != PBSGPU_OK) break;   // no page free right now: the caller pumps and retries
        PageReq q;
        q.phys = phys;
        q.k = s.next_k++;
        q.valid = (uint32_t)n;
        q.final = last && final;
        q.do_fill = true;
        q.seed = seed;
        q.kind = kind;
        q.fill_off = s.bytes_committed;  // the generator's stream offset = the page's offset in its stream
        if (r->hold) r->held.assign(stream, q.k, q.phys);
        s.ready.push_back(q);
        r->ready_bytes += n;
        s.bytes_committed += n;
        *taken += n;
        if (q.final) s.final_committed = true;
    }
    return PBSGPU_OK;
}

// Synthetic producer for EDITED streams (BASELINE.json configs[4] through the ring): the stream's bytes are defined by a
// piece table over generator 4 — kept extents of a base file and newly written extents, in stream order. The first call
// hands the table over (it is copied; pieces ascending and contiguous from 0, offsets and lengths multiples of 16), later
// calls pass NULL / 0 and continue. Otherwise like pbsgpu_ring_fill.
int pbsgpu_ring_fill_pieces(pbsgpu_ring *r, uint32_t stream, const pbsgpu_fill_piece *pieces, uint32_t npieces, uint64_t nbytes,
                            int final, uint64_t *taken) {
    if (!r || !taken || stream >= r->slots.size() || !r->slots[stream].open) return PBSGPU_E_INVALID;
    static_assert(sizeof(pbsgpu_fill_piece) == sizeof(pbsk::FillPiece), "piece layout");
    StreamSlot &s = r->slots[stream];
    *taken = 0;
    if (s.final_committed || s.reserved >= 0) return PBSGPU_E_STATE;
    if (r->error != PBSGPU_OK) return r->error;
    if (pieces) {
        if (npieces == 0 || s.bytes_committed != 0) return PBSGPU_E_INVALID;  // the table comes with the stream's first bytes
        uint64_t pos = 0;
        for (uint32_t i = 0; i < npieces; ++i) {
            if (pieces[i].dst_off != pos || pieces[i].len == 0 || ((pieces[i].dst_off | pieces[i].len | pieces[i].src_off) & 15u))
                return PBSGPU_E_INVALID;
            pos += pieces[i].len;
        }
        CHK(r->piece_tab[stream].ensure(std::max<size_t>((size_t)npieces * sizeof(pbsk::FillPiece), 4096)));
        std::memcpy(r->piece_tab[stream].p, pieces, (size_t)npieces * sizeof(pbsk::FillPiece));
        r->piece_n[stream] = npieces;
    }
    const uint32_t nt = r->piece_n[stream];
    if (nt == 0) return PBSGPU_E_STATE;
    const pbsk::FillPiece *tab = r->piece_tab[stream].as<pbsk::FillPiece>();
    const uint64_t total = tab[nt - 1].dst_off + tab[nt - 1].len;
    if (s.bytes_committed + nbytes > total || s.bytes_committed + nbytes > pbsk::kRingMaxStream) return PBSGPU_E_INVALID;
    if (nbytes == 0) {
        if (final) {
            s.zero_final = true;
            s.final_committed = true;
        }
        return PBSGPU_OK;
    }
    while (*taken < nbytes) {
        const uint64_t n = std::min<uint64_t>(r->page_bytes, nbytes - *taken);
        const bool last = (*taken + n == nbytes);
        if (n < r->page_bytes && !(last && final)) break;
        uint32_t phys = 0;
        if (ring_take_page(r, &phys) != PBSGPU_OK) break;
        PageReq q;
        q.phys = phys;
        q.k = s.next_k++;
        q.valid = (uint32_t)n;
        q.final = last && final;
        q.do_fill = true;
        q.kind = 5;
        q.tab = tab;
        q.ntab = nt;
        q.fill_off = s.bytes_committed;
        if (r->hold) r->held.assign(stream, q.k, q.phys);
        s.ready.push_back(q);
        r->ready_bytes += n;
        s.bytes_committed += n;
        *taken += n;
        if (q.final) s.final_committed = true;
    }
    return PBSGPU_OK;
}

int pbsgpu_ring_pump(pbsgpu_ring *r) {
    if (!r) return PBSGPU_E_INVALID;
    CHK(set_device(r->eng));
    ring_heartbeat(r);
    CHK(ring_service_check(r, false));
    if (r->svc == SvcState::Stopping) {  // parked: has the kernel gone yet? (then parked frees can go ahead)
        const hipError_t q = hipEventQuery(r->ev_svc1);
        if (q == hipSuccess) ring_service_ended(r);
        else (void)hipGetLastError();
    }
    ring_reap_free(r);
    ring_reap_rounds(r);
    if (r->svc == SvcState::Running) {
        // parked frees on this device have passed their cap (dev_free): every ring lets go of its service once per request;
        // the last one to end frees the memory, the next round starts the service again
        const uint32_t gen = service_park_generation(r->eng->device);
        if (gen && gen != r->park_gen_seen) {
            r->park_gen_seen = gen;
            CHK(ring_park(r));
            if (r->svc == SvcState::Stopping) r->parked_for_flush = true;
        }
    }
    bool any_round = false;
    for (int i = 0; i < 4; ++i) {
        bool did = false;
        CHK(ring_enqueue_round(r, &did));
        if (!did) break;
        any_round = true;
    }
    if (!r->defer_service && r->svc == SvcState::Stopped && r->deferred_bytes > 0) {
        // rounds were cut ahead of the service (lone stream): start it once nothing more is waiting to be cut right now, or
        // the deferral has lasted long enough
        bool waiting = false;
        for (auto &s : r->slots) waiting |= s.open && !s.ready.empty();
        const uint64_t lanes_worth = pbsp::lanes_worth(r->sha_cus, r->dense_service, r->eng->cfg.avg);
        // (Round 5 tried a 1 ms grace before "nothing waiting" ends the deferral — a feeder that commits a round's worth, pumps
        // and polls in a loop has nothing waiting after every pump, so its cut-ahead ends with the first poll: the file's last
        // bytes are cut ~7 ms sooner, its first chunks start ~25 ms later; one file alone 487-500 vs 496-502 ms on the same box,
        // the driver's line 589-592 vs 593-595: no gain, not kept. profiles/r05_ab_defer_grace.log)
        if ((!any_round && !waiting) || now_ms() - r->defer_t0 >= r->lone_defer_ms || r->deferred_bytes >= lanes_worth)
            CHK(ring_start_service(r));
    }
    if (r->autopark_ms > 0 && r->svc == SvcState::Running) {  // nothing anywhere in the ring: give the CUs (and hipFree) back
        if (ring_idle(r)) {
            const double t = now_ms();
            if (r->idle_since_ms == 0) r->idle_since_ms = t;
            else if (t - r->idle_since_ms >= r->autopark_ms) CHK(ring_park(r));
        } else {
            r->idle_since_ms = 0;
        }
    }
    return r->error;
}

int pbsgpu_ring_poll(pbsgpu_ring *r, uint32_t stream, pbsgpu_record *out, uint64_t cap, uint64_t *n, int *finished) {
    if (!r || !n || stream >= r->slots.size() || !r->slots[stream].open || (!out && cap)) return PBSGPU_E_INVALID;
    StreamSlot &s = r->slots[stream];
    ring_heartbeat(r);
    ring_reap_rounds(r);
    *n = 0;
    ring_pop_records(r, stream, out, cap, n);
    while (!r->rounds.empty() && r->rounds.front().reaped && r->rounds.front().live_cells == 0) r->rounds.pop_front();
    if (finished) *finished = (s.final_done && s.cells.empty()) ? 1 : 0;
    return r->error;
}

// Records of ANY open stream (each stream's in its own order), `segment` = stream id — for callers that drive hundreds
// or thousands of short streams (one per file) and cannot afford to ask every one of them after every pump. A stream
// that has ended and handed out its last record is reported once in `finished`.
int pbsgpu_ring_poll_any(pbsgpu_ring *r, pbsgpu_record *out, uint64_t cap, uint64_t *n, uint32_t *finished, uint32_t fcap,
                         uint32_t *nfinished) {
    if (!r || !n || !nfinished || (!out && cap) || (!finished && fcap)) return PBSGPU_E_INVALID;
    ring_heartbeat(r);
    ring_reap_rounds(r);
    *n = 0;
    *nfinished = 0;
    for (uint32_t si = 0; si < r->slots.size(); ++si) {
        StreamSlot &s = r->slots[si];
        if (!s.open || s.reported) continue;
        ring_pop_records(r, si, out, cap, n);
        if (s.final_done && s.cells.empty() && *nfinished < fcap) {
            finished[(*nfinished)++] = si;
            s.reported = true;
        }
    }
    while (!r->rounds.empty() && r->rounds.front().reaped && r->rounds.front().live_cells == 0) r->rounds.pop_front();
    return r->error;
}

// Diagnostic snapshot (text) of the device-side state: queue control words, per-page reference counts, stream states
// and what the host thinks. Safe while the service runs (plain copies on the null stream; the ring's streams are
// non-blocking).
int pbsgpu_ring_debug(pbsgpu_ring *r, char *buf, uint64_t cap) {
    if (!r || !buf || cap < 64) return PBSGPU_E_INVALID;
    CHK(set_device(r->eng));
    pbsk::RingCtl ctl{};
    std::vector<uint32_t> pend(r->npages);
    std::vector<pbsk::RingStreamState> sts(r->max_streams);
    HIPCHK(hipMemcpy(&ctl, r->ctl.p, sizeof(ctl), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(pend.data(), r->pending.p, (size_t)r->npages * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(sts.data(), r->streams.p, (size_t)r->max_streams * sizeof(pbsk::RingStreamState), hipMemcpyDeviceToHost));
    size_t o = 0;
    auto put = [&](const char *fmt, auto... a) {
        if (o + 1 < cap) o += (size_t)std::max(0, snprintf(buf + o, (size_t)(cap - o), fmt, a...));
        if (o >= cap) o = (size_t)cap - 1;
    };
    volatile uint32_t *hb = hb_words(r);
    put("ctl: tail=%u stop=%u head=%u ltail=%u lhead=%u free_count=%u error=%u rounds_done=%u | host: free_read=%u free_pages=%zu "
        "rounds=%zu next_seq=%u rounds_enq=%u service=%d tail_seen=%u claim_progress=%u backlog_limit=%llu intent=%u committed=%u\n",
        ctl.tail, ctl.stop, ctl.head, ctl.ltail, ctl.lhead, ctl.free_count, ctl.error, ctl.rounds_done, r->free_read,
        r->free_pages.size(), r->rounds.size(), r->next_seq, r->rounds_enq, (int)r->svc, r->tail_seen, hb[pbsk::kHbClaim],
        (unsigned long long)r->backlog_limit, hb[pbsk::kHbIntent], hb[pbsk::kHbCommitted]);
    {
        unsigned long long pr[16] = {};
        HIPCHK(hipMemcpy(pr, r->probe.p, sizeof(pr), hipMemcpyDeviceToHost));
        put("lanes service: cus=%u short_bytes=%u stail=%u shead=%u steps_sampled=%llu ns_per_block_step=%.1f lanes_busy=%.3f | pair cus=%u "
            "lanes_busy=%.3f (probe wave, intervals with a block in every step) express cus=%u\n",
            r->lanes_cus, r->short_bytes, ctl.stail, ctl.shead, pr[6], pr[6] ? (double)pr[7] * 10.0 / (double)pr[6] : 0.0,
            pr[6] ? (double)pr[9] / (64.0 * (double)pr[6]) : 0.0, r->sha_cus, pr[0] ? (double)pr[8] / (64.0 * (double)pr[0]) : 0.0, r->xp_cus);
        for (int cls = 0; cls < 2; ++cls)
            if (r->ctl_phase_rounds[cls])
                put("control kernel, %s rounds: %llu rounds, us per round: tiles+compaction %.1f, resolve %.1f, numbering %.1f, records %.1f, publish %.1f\n",
                    cls ? "large (>= 100 pages)" : "small (< 100 pages)", (unsigned long long)r->ctl_phase_rounds[cls],
                    r->ctl_phase_ticks[cls][0] * 0.01 / r->ctl_phase_rounds[cls], r->ctl_phase_ticks[cls][1] * 0.01 / r->ctl_phase_rounds[cls],
                    r->ctl_phase_ticks[cls][2] * 0.01 / r->ctl_phase_rounds[cls], r->ctl_phase_ticks[cls][3] * 0.01 / r->ctl_phase_rounds[cls],
                    r->ctl_phase_ticks[cls][4] * 0.01 / r->ctl_phase_rounds[cls]);
        put("probe raw: pair_steps=%llu pair_active=%llu lanes_steps=%llu lanes_active=%llu\n", pr[0], pr[8], pr[6], pr[9]);
    }
    uint32_t nz = 0;
    for (uint32_t p = 0; p < r->npages && nz < 64; ++p)
        if (pend[p]) {
            put("page %u pending=%u\n", p, pend[p]);
            ++nz;
        }
    for (uint32_t i = 0; i < r->slots.size(); ++i) {
        const StreamSlot &s = r->slots[i];
        if (!s.open) continue;
        put("stream %u: committed=%llu enqueued=%llu final_committed=%d final_enqueued=%d final_done=%d ready=%zu cells=%zu "
            "out=%llu | device c=%llu end=%llu\n", i, (unsigned long long)s.bytes_committed,
            (unsigned long long)s.bytes_enqueued, (int)s.final_committed, (int)s.final_enqueued, (int)s.final_done,
            s.ready.size(), s.cells.size(), (unsigned long long)s.records_out, (unsigned long long)sts[i].c,
            (unsigned long long)sts[i].end);
        if (!s.cells.empty()) {
            const uint8_t *c = r->cells.as<uint8_t>() + (size_t)s.cells.front().cell * pbsk::kCellBytes;
            pbsgpu_record rec;
            std::memcpy(&rec, c, sizeof(rec));
            put("  waiting for cell %u: end=%llu size=%u flag=%u\n", s.cells.front().cell, (unsigned long long)rec.end, rec.size,
                reinterpret_cast<const uint32_t *>(c)[pbsk::kCellFlag]);
        }
    }
    return PBSGPU_OK;
}

int pbsgpu_ring_express(pbsgpu_ring *r, uint32_t *express_cus, uint64_t *long_bytes) {
    if (!r) return PBSGPU_E_INVALID;
    if (express_cus) *express_cus = r->xp_cus;
    if (long_bytes) *long_bytes = r->xp_cus ? r->long_bytes : 0;
    return PBSGPU_OK;
}

int pbsgpu_ring_get_probe(pbsgpu_ring *r, pbsgpu_ring_probe *out) {
    if (!r || !out) return PBSGPU_E_INVALID;
    static_assert(sizeof(pbsgpu_ring_probe) == 48, "six counters");
    // While a service runs the answer comes from the newest reaped round's status block (k_ring_control copies the counters
    // there, mapped pinned: at most one round — about a millisecond — old; the probe waves sample every ~7 ms): no HIP call
    // of the host beside a persistent kernel. (Until the end of round 6 this was a hipMemcpy on the null stream inside
    // bench.py's timed region; pbsgpu_ring_debug, which still copies that way, was seen to stall for the service's idle
    // timeout in 2 of 6 diagnostic runs.) With the service stopped the device counters are read directly: exact.
    if (r->svc == SvcState::Running) {
        ring_reap_rounds(r);
        if (r->probe_seen_valid) {
            std::memcpy(out, r->probe_seen, sizeof(*out));
            return PBSGPU_OK;
        }
    }
    CHK(set_device(r->eng));
    HIPCHK(hipMemcpy(out, r->probe.p, sizeof(*out), hipMemcpyDeviceToHost));
    std::memcpy(r->probe_seen, out, sizeof(*out));  // (the counters only grow: a later answer from a status block is never older)
    r->probe_seen_valid = true;
    return PBSGPU_OK;
}

int pbsgpu_ring_get_stats(pbsgpu_ring *r, pbsgpu_ring_stats *out) {
    if (!r || !out) return PBSGPU_E_INVALID;
    ring_reap_free(r);
    r->st.pages_free = (uint32_t)r->free_pages.size();
    r->st.rounds_in_flight = 0;
    for (auto &ri : r->rounds) r->st.rounds_in_flight += ri.reaped ? 0 : 1;
    *out = r->st;
    return PBSGPU_OK;
}

}  // extern "C"
