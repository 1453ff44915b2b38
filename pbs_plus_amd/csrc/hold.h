// Held pages of a page ring created with PBSGPU_RING_F_HOLD_PAGES (ring.cpp): which stream and logical
// page every physical page carries, which pages the services have handed back, and each stream's release watermark.
// A page returns to the free list when BOTH hold: the services have handed it back, and it lies wholly below its
// stream's watermark (or the stream was closed). On the engine's ring streams that hold share the pages
// with streams that do not: the latter's pages are nobody's (`unowned`) and free at hand-back, and
// `frees_without_release` says whether a holder that waits for a page waits for itself. Host-only, no HIP:
// tests/test_ring_upload_surface.py and tests/native/test_hold_streams.cpp drive it against models.
#pragma once

#include <cstdint>
#include <deque>
#include <vector>

namespace pbse {

class HeldPages {
public:
    void init(uint32_t npages, uint32_t nstreams, uint64_t page_bytes) {
        page_ = page_bytes;
        owner_.assign(npages, Owner{});
        out_.assign(npages, 0);
        streams_.assign(nstreams, Stream{});
    }
    // a new stream takes the slot
    void open(uint32_t slot) {
        const uint32_t gen = streams_[slot].gen + 1;
        streams_[slot] = Stream{};
        streams_[slot].gen = gen;
    }
    // physical page `phys` now carries logical page k of the stream (k ascending per stream, as pages are committed)
    void assign(uint32_t slot, uint64_t k, uint32_t phys) {
        Stream &s = streams_[slot];
        if (s.pages.empty()) s.base_k = k;
        s.pages.push_back(Page{phys, kOut});
        owner_[phys] = Owner{slot, s.gen, k, true};
        out_[phys] = 1;
    }
    // the page was committed for a stream that does not hold: nobody's page, free the moment it is handed back
    void unowned(uint32_t phys) {
        owner_[phys].valid = false;
        out_[phys] = 1;
    }
    // the services are done with the page: held, or free at once when it is already released
    void handed_back(uint32_t phys, std::vector<uint32_t> &free_pages) {
        const Owner o = owner_[phys];
        owner_[phys].valid = false;
        out_[phys] = 0;
        if (!o.valid || streams_[o.slot].gen != o.gen) {  // no stream's page (any more: closed)
            free_pages.push_back(phys);
            return;
        }
        Stream &s = streams_[o.slot];
        Page &p = s.pages[(size_t)(o.k - s.base_k)];
        if (o.k < s.below) {
            p.state = kGone;
            free_pages.push_back(phys);
            trim(s);
        } else {
            p.state = kHeld;
            s.held++;
        }
    }
    // the stream's bytes below `upto` are no longer needed (the watermark only moves forward)
    void release(uint32_t slot, uint64_t upto, std::vector<uint32_t> &free_pages) {
        Stream &s = streams_[slot];
        if (upto <= s.mark) return;
        s.mark = upto;
        s.below = upto / page_;
        for (size_t i = 0; i < s.pages.size() && s.base_k + i < s.below; ++i) {
            Page &p = s.pages[i];
            if (p.state != kHeld) continue;  // (a page still with the services goes when they hand it back)
            p.state = kGone;
            s.held--;
            free_pages.push_back(p.phys);
        }
        trim(s);
    }
    // the stream is over: what it holds is free, what the services still have becomes nobody's
    void close(uint32_t slot, std::vector<uint32_t> &free_pages) {
        Stream &s = streams_[slot];
        for (Page &p : s.pages)
            if (p.state == kHeld) free_pages.push_back(p.phys);
        open(slot);
    }
    // offset from which the stream's bytes are still available
    uint64_t first_offset(uint32_t slot) const { return streams_[slot].below * page_; }
    uint64_t watermark(uint32_t slot) const { return streams_[slot].mark; }
    uint32_t pages_held(uint32_t slot) const { return streams_[slot].held; }
    // Can a page reach the free list without a release or a close? Only a page that is still with the services and that
    // handed_back will free: nobody's (its stream does not hold, or was closed) or wholly below its stream's watermark.
    // When this is false and the free list is empty, a holding stream that waits for a page waits for itself.
    bool frees_without_release() const {
        for (size_t p = 0; p < out_.size(); ++p) {
            if (!out_[p]) continue;
            const Owner &o = owner_[p];
            if (!o.valid || streams_[o.slot].gen != o.gen || o.k < streams_[o.slot].below) return true;
        }
        return false;
    }
    // physical page of an available logical page, -1 when it is released or was never committed
    int64_t phys_of(uint32_t slot, uint64_t k) const {
        const Stream &s = streams_[slot];
        if (k < s.below || k < s.base_k || k - s.base_k >= s.pages.size()) return -1;
        const Page &p = s.pages[(size_t)(k - s.base_k)];
        return p.state == kGone ? -1 : (int64_t)p.phys;
    }

private:
    enum : uint8_t { kGone = 0, kOut = 1, kHeld = 2 };  // freed / with the services / handed back and held
    struct Page {
        uint32_t phys;
        uint8_t state;
    };
    struct Stream {
        uint64_t base_k = 0;      // logical index of pages.front()
        std::deque<Page> pages;
        uint64_t mark = 0;
        uint64_t below = 0;       // mark / page: logical pages [0, below) lie wholly below the watermark
        uint32_t held = 0;
        uint32_t gen = 0;         // a page handed back for an earlier stream of this slot is nobody's
    };
    struct Owner {
        uint32_t slot = 0, gen = 0;
        uint64_t k = 0;
        bool valid = false;
    };
    static void trim(Stream &s) {
        while (!s.pages.empty() && s.pages.front().state == kGone) {
            s.pages.pop_front();
            s.base_k++;
        }
    }
    uint64_t page_ = 1;
    std::vector<Owner> owner_;
    std::vector<uint8_t> out_;  // per physical page: committed and not handed back yet
    std::vector<Stream> streams_;
};

}  // namespace pbse
