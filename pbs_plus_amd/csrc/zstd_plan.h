// The host's block plan of the zstd encoder (zstd_encode.hip): the chunks of a call laid out in one block index space, and
// that space cut into rounds. It needs the chunks' LENGTHS only, so it is the same for a call whose chunks are all
// encoded (pbsgpu_zstd_encode_device, pbsgpu_blob_encode2_device) and for one where the device decides which are
// (pbsgpu_*_upload_new2_device). Plain C++: tests/native/test_zstd_plan.cpp runs it under sanitizers.
#pragma once

#include <cstdint>
#include <vector>

namespace pbsz {
namespace enc {

struct BlockPlan {
    std::vector<uint32_t> first;   // n: a chunk's first block; it has ceil(len / block_bytes) of them (none when empty)
    std::vector<uint32_t> bchunk;  // nblocks: the chunk of every block
    std::vector<uint32_t> cuts;    // round r = chunks [cuts[r], cuts[r + 1]); cuts.front() = 0, cuts.back() = n
    uint64_t nblocks = 0;
    uint64_t most = 0;             // blocks of the largest round
    // blocks [block_begin(c), block_end(c)) are chunk c's; block_begin(n) = nblocks
    uint32_t block_begin(uint32_t c) const { return c < first.size() ? first[c] : (uint32_t)nblocks; }
    uint32_t block_end(uint32_t c) const { return block_begin(c + 1); }
};

// Rounds hold whole chunks and round_blocks blocks at the most, unless one chunk alone has more. false: 2^32 blocks or
// more in one call (512 TiB at 128 KiB), and bp is then unspecified.
template <class LenOf>
bool plan_blocks(uint32_t n, LenOf len_of, uint32_t block_bytes, uint32_t round_blocks, BlockPlan &bp) {
    bp = BlockPlan{};
    bp.first.resize(n);
    uint64_t nblocks = 0;
    for (uint32_t c = 0; c < n; ++c) {
        if (nblocks >= (1ull << 32)) return false;
        bp.first[c] = (uint32_t)nblocks;
        nblocks += ((uint64_t)len_of(c) + block_bytes - 1) / block_bytes;
    }
    if (nblocks >= (1ull << 32)) return false;
    bp.nblocks = nblocks;
    bp.bchunk.resize((size_t)nblocks);
    for (uint32_t c = 0; c < n; ++c)
        for (uint64_t b = bp.first[c], end = bp.block_end(c); b < end; ++b) bp.bchunk[b] = c;
    bp.cuts.push_back(0);
    for (uint32_t c = 0, from = 0; c < n; ++c) {
        const uint64_t end = bp.block_end(c);
        if (end - bp.first[from] > round_blocks && c > from) {
            bp.cuts.push_back(c);
            from = c;
        }
        if (end - bp.first[from] > bp.most) bp.most = end - bp.first[from];
    }
    bp.cuts.push_back(n);
    return true;
}

}  // namespace enc
}  // namespace pbsz
