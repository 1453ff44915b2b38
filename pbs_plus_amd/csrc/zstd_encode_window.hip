// The block kernels of the zstd encoder's long-range match finder (pbsgpu_engine_options::zstd_window_log = 17, 18 or 19;
// include/pbsgpu.h): k_zenc_wblocks is k_zenc_blocks (zstd_encode.hip) and k_zenc_wtblocks is
// k_zenc_tblocks (zstd_encode_tables.hip) with a match finder whose candidates may lie in the block's history, up to
// 1 << window_log bytes of the same chunk in front of the block. Same grid, jobs, counter and result word, so that the
// launch site picks one of four and k_zenc_assemble puts any one's blocks together. They live here so that the other two
// translation units stay the kernels they were.
//   * The table (1 << 14 words, 64 KiB) lies in the workgroup's part of the slot's scratch, in global memory: in LDS it
//     would leave two workgroups per CU where the grid runs four, one per SIMD, and every wave is bound by its own serial
//     chain. All lanes zero it per block, the history is inserted with vector atomicMax, and the lookups are plain loads
//     behind a workgroup barrier. LDS is what the other two kernels take: WState and WTState add nothing to State and
//     TState, whose 16 KiB union serves only as the decoder's State while FSE tables are built.
//   * A chunk in two parts (a ring chunk in two pages) is read in place through enc::Src2; nothing is staged, because the
//     seam may lie anywhere in the history. Every address comes from the plan's pointers: global loads only.
// No scratch memory, no spills (tests/test_zstd_window_surface.py; make usage-zstd-encode-window).
#include "zstd_encode_blocks.h"

namespace pbsk {
namespace zenc {

__global__ __launch_bounds__(64) void k_zenc_wblocks(Plan pl) {
    __shared__ ze::WState st;
    encode_blocks(pl, st);
}

__global__ __launch_bounds__(64) void k_zenc_wtblocks(Plan pl) {
    __shared__ ze::WTState st;
    encode_blocks(pl, st);
}

hipError_t launch_blocks_window(const Plan &pl, uint32_t grid, bool tables, hipStream_t st) {
    if (tables) hipLaunchKernelGGL(k_zenc_wtblocks, dim3(grid), dim3(64), 0, st, pl);
    else hipLaunchKernelGGL(k_zenc_wblocks, dim3(grid), dim3(64), 0, st, pl);
    return hipGetLastError();
}

}  // namespace zenc
}  // namespace pbsk
