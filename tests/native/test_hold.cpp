// Driver for pbs_plus_amd/csrc/hold.h (the held-page bookkeeping of a PBSGPU_RING_F_HOLD_PAGES ring), host only.
// Reads one operation per line from stdin and answers each with the pages it freed and every stream's state:
//   init <npages> <nstreams> <page_bytes>
//   open <slot> | assign <slot> <k> <phys> | back <phys> | release <slot> <upto> | close <slot>
//   phys <slot> <k>   (answered with "phys <physical page or -1>" alone)
// answer: "free p p ... | first pages_held first pages_held ..." (one pair per stream slot)
// tests/test_ring_upload_surface.py generates the operations and compares the answers with its model.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pbs_plus_amd/csrc/hold.h"

int main() {
    pbse::HeldPages h;
    uint32_t nstreams = 0;
    char op[16];
    while (std::scanf("%15s", op) == 1) {
        std::vector<uint32_t> freed;
        unsigned long long a = 0, b = 0, c = 0;
        if (!std::strcmp(op, "init")) {
            if (std::scanf("%llu %llu %llu", &a, &b, &c) != 3) return 2;
            h.init((uint32_t)a, (uint32_t)b, c);
            nstreams = (uint32_t)b;
        } else if (!std::strcmp(op, "open")) {
            if (std::scanf("%llu", &a) != 1) return 2;
            h.open((uint32_t)a);
        } else if (!std::strcmp(op, "assign")) {
            if (std::scanf("%llu %llu %llu", &a, &b, &c) != 3) return 2;
            h.assign((uint32_t)a, b, (uint32_t)c);
        } else if (!std::strcmp(op, "back")) {
            if (std::scanf("%llu", &a) != 1) return 2;
            h.handed_back((uint32_t)a, freed);
        } else if (!std::strcmp(op, "release")) {
            if (std::scanf("%llu %llu", &a, &b) != 2) return 2;
            h.release((uint32_t)a, b, freed);
        } else if (!std::strcmp(op, "close")) {
            if (std::scanf("%llu", &a) != 1) return 2;
            h.close((uint32_t)a, freed);
        } else if (!std::strcmp(op, "phys")) {
            if (std::scanf("%llu %llu", &a, &b) != 2) return 2;
            std::printf("phys %lld\n", (long long)h.phys_of((uint32_t)a, b));
            continue;
        } else {
            return 3;
        }
        std::printf("free");
        for (uint32_t p : freed) std::printf(" %u", p);
        std::printf(" |");
        for (uint32_t s = 0; s < nstreams; ++s) std::printf(" %" PRIu64 " %u", h.first_offset(s), h.pages_held(s));
        std::printf("\n");
    }
    std::printf("hold-ok\n");
    return 0;
}
