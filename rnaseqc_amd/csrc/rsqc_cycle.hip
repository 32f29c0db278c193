// rsqc_cycle.hip -- base quality and composition by read cycle on MI355X (gfx950): the kernels around cycle_block (rsqc_cycle.h,
// shared with the host emulation of the tests) and their launches.  One launch per decode window, behind the window's parse stage:
// blockIdx.y is the tile of 128 cycles a workgroup of 16 waves owns in LDS (69 KB: two workgroups per CU), blockIdx.x its share of the records.
#include <hip/hip_runtime.h>

#include "rsqc_cycle.h"

namespace rsqc {

__global__ __launch_bounds__(CYC_THREADS) void cycle_bam_kernel(CycleBamSrc src, CycleTables T) {
    if (src.W.sum->status) return;                                   // (a window the stages refused: the pass ends with its error)
    cycle_block(src, src.W.sum->n_rec, T, blockIdx.y, blockIdx.x, gridDim.x);
}
__global__ __launch_bounds__(CYC_THREADS) void cycle_sam_kernel(CycleSamSrc src, CycleTables T) {
    if (src.S.W.sum->status) return;
    cycle_block(src, src.S.W.sum->n_rec, T, blockIdx.y, blockIdx.x, gridDim.x);
}

// the record count is on the device: a grid for the most records the window can hold, at most 256 workgroups per tile -- with reads
// shorter than a tile nearly all the work is the first tile's, and its workgroups (blockIdx.y == 0: dispatched first) then fill half the
// chip's slots (256 CUs, two workgroups each) while the other tiles' pass through the rest; every wave takes 64 records per step
void launch_cycle_bam(hipStream_t s, const DecodeWindow &W, const CycleTables &T) {
    cycle_bam_kernel<<<dim3(capped_grid(decode_max_records(W), CYC_THREADS, 256u), CYC_TILES), CYC_THREADS, 0, s>>>(CycleBamSrc{W}, T);
}
void launch_cycle_sam(hipStream_t s, const SamWindow &S, const CycleTables &T) {
    cycle_sam_kernel<<<dim3(capped_grid(S.rec_cap, CYC_THREADS, 256u), CYC_TILES), CYC_THREADS, 0, s>>>(CycleSamSrc{S}, T);
}

}  // namespace rsqc
