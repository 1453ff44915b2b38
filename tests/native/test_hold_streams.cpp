// pbs_plus_amd/csrc/hold.h as the ENGINE's ring uses it: streams that hold their pages and streams that
// do not share one ring. Host only, own main, built with ASan + UBSan by tests/test_stream_upload_native.py.
// Seeded random interleavings of open (holding or not), commit, hand-back, release and close run against a model:
//   * a page of a stream that does not hold is freed by its hand-back, alone, so in hand-back order;
//   * a holder's page is freed once it was handed back AND lies wholly below the watermark, or when its stream closes;
//   * frees_without_release() is true exactly when the model finds a page, still with the services, that its hand-back
//     will free: nobody's page (a non-holder's, or a closed stream's) or one below its stream's watermark;
//   * a stream closed late — long after its last page was handed back, or with pages still out — returns every page once.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pbs_plus_amd/csrc/hold.h"

namespace {

#define REQUIRE(c)                                                                  \
    do {                                                                            \
        if (!(c)) {                                                                 \
            std::fprintf(stderr, "%s:%d: REQUIRE(%s) failed (seed %u step %d)\n", __FILE__, __LINE__, #c, g_seed, g_step); \
            std::exit(1);                                                           \
        }                                                                           \
    } while (0)

unsigned g_seed = 0;
int g_step = 0;
uint64_t g_stuck = 0, g_unstuck = 0;  // steps with no free page at which the predicate said "only a release" / "wait"

struct Rng {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
    uint32_t below(uint32_t n) { return next() % n; }
};

struct MPage {
    enum State { Free, Out, Held } state = Free;
    int slot = -1;  // -1: nobody's
    uint64_t k = 0;
};

struct MStream {
    bool open = false, holding = false;
    uint64_t mark = 0, next_k = 0;
};

struct Model {
    uint64_t page;
    std::vector<MPage> pages;
    std::vector<MStream> streams;
    uint64_t frees = 0;

    void free_page(uint32_t p, std::vector<uint32_t> &freed) {
        REQUIRE(pages[p].state != MPage::Free);  // never twice
        pages[p] = MPage{};
        freed.push_back(p);
        frees++;
    }
    bool below_mark(const MPage &pg) const { return (pg.k + 1) * page <= streams[(size_t)pg.slot].mark; }
    void back(uint32_t p, std::vector<uint32_t> &freed) {
        MPage &pg = pages[p];
        REQUIRE(pg.state == MPage::Out);
        if (pg.slot < 0 || below_mark(pg)) free_page(p, freed);
        else pg.state = MPage::Held;
    }
    void release(uint32_t s, uint64_t upto, std::vector<uint32_t> &freed) {
        streams[s].mark = std::max(streams[s].mark, upto);
        for (uint32_t p = 0; p < pages.size(); ++p)
            if (pages[p].state == MPage::Held && pages[p].slot == (int)s && below_mark(pages[p])) free_page(p, freed);
    }
    void close(uint32_t s, std::vector<uint32_t> &freed) {
        for (uint32_t p = 0; p < pages.size(); ++p) {
            if (pages[p].slot != (int)s) continue;
            if (pages[p].state == MPage::Held) free_page(p, freed);
            else if (pages[p].state == MPage::Out) pages[p].slot = -1;  // what the services still have becomes nobody's
        }
        streams[s] = MStream{};
    }
    // a page that is still with the services and that its hand-back will free
    bool can_come_back() const {
        for (const MPage &pg : pages)
            if (pg.state == MPage::Out && (pg.slot < 0 || below_mark(pg))) return true;
        return false;
    }
    uint32_t held(uint32_t s) const {
        uint32_t n = 0;
        for (const MPage &pg : pages) n += pg.state == MPage::Held && pg.slot == (int)s;
        return n;
    }
};

void same(std::vector<uint32_t> a, std::vector<uint32_t> b) {
    std::sort(a.begin(), a.end());
    std::sort(b.begin(), b.end());
    REQUIRE(a == b);
}

void run(unsigned seed, uint32_t npages, uint32_t nstreams, uint64_t page, int steps) {
    g_seed = seed;
    Rng rng{seed * 0x9e3779b97f4a7c15ull + 1};
    pbse::HeldPages h;
    h.init(npages, nstreams, page);
    Model m{page, std::vector<MPage>(npages), std::vector<MStream>(nstreams)};
    uint64_t stuck = 0, unstuck = 0, nobody_freed = 0, late_closes = 0;
    for (g_step = 0; g_step < steps; ++g_step) {
        std::vector<uint32_t> got, want;
        const uint32_t s = rng.below(nstreams);
        MStream &ms = m.streams[s];
        const uint32_t op = rng.below(12);
        std::vector<uint32_t> out, freep;
        for (uint32_t p = 0; p < npages; ++p) {
            if (m.pages[p].state == MPage::Out) out.push_back(p);
            if (m.pages[p].state == MPage::Free) freep.push_back(p);
        }
        if (!ms.open) {
            ms = MStream{};
            ms.open = true;
            ms.holding = rng.below(2) == 0;  // a slot serves holders and non-holders in turn
            h.open(s);
        } else if (op < 5 && !freep.empty()) {  // a page is committed
            const uint32_t p = freep[rng.below((uint32_t)freep.size())];
            m.pages[p].state = MPage::Out;
            m.pages[p].k = ms.next_k;
            if (ms.holding) {
                m.pages[p].slot = (int)s;
                h.assign(s, ms.next_k, p);
            } else {
                m.pages[p].slot = -1;
                h.unowned(p);
            }
            ms.next_k++;
        } else if (op < 8 && !out.empty()) {  // the services hand a page back
            const uint32_t p = out[rng.below((uint32_t)out.size())];
            const bool nobody = m.pages[p].slot < 0;
            m.back(p, want);
            h.handed_back(p, got);
            if (nobody) {  // freed at hand-back, that page alone: hand-back order is free-list order
                REQUIRE(got.size() == 1 && got[0] == p);
                nobody_freed++;
            }
        } else if (op < 10 && ms.holding) {
            const uint64_t hi = ms.next_k * page;
            const uint64_t choices[5] = {hi ? rng.next() % (hi + 1) : 0, hi, hi ? hi - 1 : 0, hi / page / 2 * page + 1, ms.mark / 2};
            const uint64_t upto = std::min(choices[rng.below(5)], hi);
            m.release(s, upto, want);
            h.release(s, upto, got);
        } else if (op == 10 && rng.below(3) == 0) {  // closed whenever: right away, or long after its last hand-back
            bool any_out = false;
            for (const MPage &pg : m.pages) any_out |= pg.state == MPage::Out && pg.slot == (int)s;
            late_closes += !any_out && m.held(s) > 0;
            m.close(s, want);
            h.close(s, got);
        }
        same(got, want);
        for (uint32_t t = 0; t < nstreams; ++t) {
            if (!m.streams[t].open || !m.streams[t].holding) continue;
            REQUIRE(h.pages_held(t) == m.held(t));
            REQUIRE(h.first_offset(t) == m.streams[t].mark / page * page);
        }
        // the predicate, after every step
        const bool can = m.can_come_back();
        REQUIRE(h.frees_without_release() == can);
        bool none_free = true;
        for (const MPage &pg : m.pages) none_free &= pg.state != MPage::Free;
        if (none_free) (can ? unstuck : stuck)++;
    }
    // everything comes back exactly once: hand back what is out, close every stream
    std::vector<uint32_t> got, want;
    for (uint32_t p = 0; p < npages; ++p)
        if (m.pages[p].state == MPage::Out) {
            m.back(p, want);
            h.handed_back(p, got);
        }
    for (uint32_t s = 0; s < nstreams; ++s)
        if (m.streams[s].open) {
            m.close(s, want);
            h.close(s, got);
        }
    same(got, want);
    for (const MPage &pg : m.pages) REQUIRE(pg.state == MPage::Free);
    REQUIRE(!h.frees_without_release());
    REQUIRE(m.frees > npages);   // pages went round more than once
    REQUIRE(nobody_freed > 0 && late_closes > 0);
    g_stuck += stuck;
    g_unstuck += unstuck;
    std::printf("seed %u: %d steps, %" PRIu64 " frees, full arena %" PRIu64 " times waiting for a release, %" PRIu64
                " times not\n", seed, steps, m.frees, stuck, unstuck);
}

// the rule at its edges, step by step
void fixed() {
    g_seed = 0;
    g_step = -1;
    pbse::HeldPages h;
    std::vector<uint32_t> f;
    h.init(3, 2, 100);
    REQUIRE(!h.frees_without_release());  // nothing is out
    h.open(0);                            // a holder
    h.open(1);                            // a stream that does not hold
    h.assign(0, 0, 0);
    h.assign(0, 1, 1);
    REQUIRE(!h.frees_without_release());  // both pages wait for a release
    h.unowned(2);
    REQUIRE(h.frees_without_release());   // the non-holder's page comes back by itself
    h.handed_back(2, f);
    REQUIRE(f == std::vector<uint32_t>{2} && !h.frees_without_release());
    h.release(0, 199, f);                 // page 0 lies below, page 1 does not; both still out
    REQUIRE(f.size() == 1 && h.frees_without_release());
    h.handed_back(0, f);
    REQUIRE((f == std::vector<uint32_t>{2, 0}) && !h.frees_without_release());
    h.handed_back(1, f);                  // held
    REQUIRE(f.size() == 2 && h.pages_held(0) == 1 && !h.frees_without_release());
    h.assign(0, 2, 2);
    h.close(0, f);                        // the held page now, the one that is out as nobody's
    REQUIRE((f == std::vector<uint32_t>{2, 0, 1}) && h.frees_without_release());
    h.handed_back(2, f);
    REQUIRE((f == std::vector<uint32_t>{2, 0, 1, 2}) && !h.frees_without_release());
    // the whole-section release of the payload stream: everything below, whatever its size
    h.open(0);
    h.assign(0, 0, 0);
    h.assign(0, 1, 1);
    h.handed_back(0, f);
    f.clear();
    h.release(0, ~0ull, f);
    REQUIRE(f == std::vector<uint32_t>{0} && h.frees_without_release());
    h.handed_back(1, f);
    REQUIRE((f == std::vector<uint32_t>{0, 1}) && h.pages_held(0) == 0);
}

}  // namespace

int main() {
    fixed();
    run(1, 4, 2, 4096, 20000);
    run(2, 12, 3, 65536, 30000);
    run(3, 40, 6, 1 << 20, 40000);
    run(4, 3, 4, 512, 20000);
    REQUIRE(g_stuck > 1000 && g_unstuck > 1000);  // the full arena was seen both ways, often
    std::printf("hold-streams-ok\n");
    return 0;
}
