// The zstd encoder's host block plan (pbs_plus_amd/csrc/zstd_plan.h) on its own, under ASan + UBSan.
// stdin: one case per line, "round_blocks block_bytes len len len ..." (no len: no chunks). For every case the plan is
// checked here — every block belongs to exactly one chunk, chunks have the blocks their lengths ask for, rounds hold whole
// chunks in order and at most round_blocks blocks unless one chunk alone has more, the totals match — and printed as
// "nblocks most | cuts ... | first ..." for the driver, which compares it with its own model. "plan-ok" at the end.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../pbs_plus_amd/csrc/zstd_plan.h"

#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);          \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        uint64_t round_blocks = 0, block_bytes = 0, v = 0;
        in >> round_blocks >> block_bytes;
        std::vector<uint32_t> lens;
        while (in >> v) lens.push_back((uint32_t)v);
        const uint32_t n = (uint32_t)lens.size();
        pbsz::enc::BlockPlan bp;
        const bool ok = pbsz::enc::plan_blocks(n, [&](uint32_t c) { return lens[c]; }, (uint32_t)block_bytes, (uint32_t)round_blocks, bp);
        uint64_t want = 0;
        for (uint32_t len : lens) want += ((uint64_t)len + block_bytes - 1) / block_bytes;
        if (want >= (1ull << 32)) {
            REQUIRE(!ok);
            std::printf("refused\n");
            continue;
        }
        REQUIRE(ok);
        REQUIRE(bp.nblocks == want && bp.first.size() == n && bp.bchunk.size() == want);
        // every block belongs to exactly one chunk: the chunks' block ranges tile [0, nblocks) in order
        std::vector<uint32_t> owners((size_t)want, 0);
        uint64_t at = 0;
        for (uint32_t c = 0; c < n; ++c) {
            const uint64_t nb = ((uint64_t)lens[c] + block_bytes - 1) / block_bytes;
            REQUIRE(bp.first[c] == at && bp.block_begin(c) == at && bp.block_end(c) == at + nb);
            for (uint64_t b = at; b < at + nb; ++b) {
                REQUIRE(bp.bchunk[b] == c);
                owners[b]++;
            }
            at += nb;
        }
        REQUIRE(at == want && bp.block_begin(n) == want);
        for (uint32_t o : owners) REQUIRE(o == 1);
        // rounds: whole chunks, in order, none empty unless there are no chunks
        REQUIRE(bp.cuts.size() >= 2 && bp.cuts.front() == 0 && bp.cuts.back() == n);
        uint64_t most = 0, total = 0;
        for (size_t r = 0; r + 1 < bp.cuts.size(); ++r) {
            const uint32_t c0 = bp.cuts[r], c1 = bp.cuts[r + 1];
            REQUIRE(c0 < c1 || n == 0);
            const uint64_t blocks = (uint64_t)bp.block_begin(c1) - bp.block_begin(c0);
            REQUIRE(blocks <= round_blocks || c1 - c0 == 1);
            if (r + 2 < bp.cuts.size())  // a round ends only because the next chunk would not fit
                REQUIRE((uint64_t)bp.block_end(c1) - bp.block_begin(c0) > round_blocks);
            most = blocks > most ? blocks : most;
            total += blocks;
        }
        REQUIRE(most == bp.most && total == want);
        std::printf("%llu %llu |", (unsigned long long)bp.nblocks, (unsigned long long)bp.most);
        for (uint32_t c : bp.cuts) std::printf(" %u", c);
        std::printf(" |");
        for (uint32_t f : bp.first) std::printf(" %u", f);
        std::printf("\n");
    }
    std::printf("plan-ok\n");
    return 0;
}
