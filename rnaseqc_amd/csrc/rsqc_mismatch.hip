// rsqc_mismatch.hip -- errors by read cycle against the reference on MI355X (gfx950): the pack kernel of the reference (four bits per
// base), the kernels around mismatch_block (rsqc_mismatch.h, shared with the host emulation of the tests) and their launches.  One launch
// per decode window, behind the window's parse stage: a workgroup of 16 waves holds the whole cycle table in LDS (33 KB) and takes its
// share of the records, blockIdx.x of gridDim.x.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rsqc_mismatch.h"

namespace rsqc {

// eight bases per thread and word; the places of the last word behind the contig's end are written too (code 4)
__global__ __launch_bounds__(256) void mismatch_pack_kernel(const uint8_t *ascii, uint64_t len, uint32_t *words) {
    const uint64_t n_words = (len + 7) / 8;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * blockDim.x) words[w] = mismatch_pack_word(ascii, len, w);
}

__global__ __launch_bounds__(MM_THREADS) void mismatch_bam_kernel(MismatchBamSrc src, MismatchPackedRef ref, uint32_t min_mapq, MismatchTables T) {
    if (src.W.sum->status) return;                                   // (a window the stages refused: the pass ends with its error)
    mismatch_block(src, src.W.sum->n_rec, ref, min_mapq, T, blockIdx.x, gridDim.x);
}
__global__ __launch_bounds__(MM_THREADS) void mismatch_sam_kernel(MismatchSamSrc src, MismatchPackedRef ref, uint32_t min_mapq, MismatchTables T) {
    if (src.S.W.sum->status) return;
    mismatch_block(src, src.S.W.sum->n_rec, ref, min_mapq, T, blockIdx.x, gridDim.x);
}

void launch_mismatch_pack(hipStream_t s, const uint8_t *ascii, uint64_t len, uint32_t *words) {
    const uint64_t n_words = (len + 7) / 8;
    if (!n_words) return;
    mismatch_pack_kernel<<<dim3((unsigned)std::min<uint64_t>((n_words + 255) / 256, 65536)), dim3(256), 0, s>>>(ascii, len, words);
}

// the record count is on the device: a grid for the most records the window can hold, at most 256 workgroups (one per CU; the flush of a
// workgroup is up to 6 000 global atomics, so more workgroups than the records can feed only add flushes); every wave takes 64 records
// per step
void launch_mismatch_bam(hipStream_t s, const DecodeWindow &W, const MismatchPackedRef &ref, uint32_t min_mapq, const MismatchTables &T) {
    mismatch_bam_kernel<<<dim3(capped_grid(decode_max_records(W), MM_THREADS, 256u)), MM_THREADS, 0, s>>>(MismatchBamSrc{W}, ref, min_mapq, T);
}
void launch_mismatch_sam(hipStream_t s, const SamWindow &S, const MismatchPackedRef &ref, uint32_t min_mapq, const MismatchTables &T) {
    mismatch_sam_kernel<<<dim3(capped_grid(S.rec_cap, MM_THREADS, 256u)), MM_THREADS, 0, s>>>(MismatchSamSrc{S}, ref, min_mapq, T);
}

}  // namespace rsqc
