// The block kernel of the zstd encoder's mode with per-block sequence tables and repeat codes
// (pbsgpu_engine_options::zstd_seq_tables = 1; include/pbsgpu.h). It is k_zenc_blocks (zstd_encode.hip) on a
// larger State: the same grid, jobs, counter, scratch and result word, so that the launch site picks one or the other and
// k_zenc_assemble puts either's blocks together. It lives here so that zstd_encode.hip stays the two kernels it was.
// LDS: enc::TState = enc::State + three tables of 512 states, three histograms and three descriptions, about 25.5 KiB:
// six workgroups fit a CU's 160 KiB, and the grid runs four per CU. No scratch memory, no spills
// (tests/test_zstd_encode_tables_surface.py; make usage-zstd-encode-tables).
#include "zstd_encode_blocks.h"

namespace pbsk {
namespace zenc {

__global__ __launch_bounds__(64) void k_zenc_tblocks(Plan pl) {
    __shared__ ze::TState st;
    encode_blocks(pl, st);
}

hipError_t launch_blocks_tables(const Plan &pl, uint32_t grid, hipStream_t st) {
    hipLaunchKernelGGL(k_zenc_tblocks, dim3(grid), dim3(64), 0, st, pl);
    return hipGetLastError();
}

}  // namespace zenc
}  // namespace pbsk
