// rsqc_allele.hip -- base counts at known variant sites on MI355X (gfx950): the kernels around allele_block (rsqc_allele.h, shared with
// the host emulation of the tests) and their launches.  One launch per decode window, behind the window's parse stage: a lane per record,
// workgroups of four waves, blockIdx.x of gridDim.x takes its share of the records.
#include <hip/hip_runtime.h>

#include "rsqc_allele.h"

namespace rsqc {

template <bool MERGE> __global__ __launch_bounds__(AL_THREADS) void allele_bam_kernel(MismatchBamSrc src, AlleleSites sites, uint32_t min_mapq, uint32_t min_baseq, AlleleTables T) {
    if (src.W.sum->status) return;                                   // (a window the stages refused: the pass ends with its error)
    allele_block<MERGE>(src, src.W.sum->n_rec, sites, min_mapq, min_baseq, T, blockIdx.x, gridDim.x);
}
template <bool MERGE> __global__ __launch_bounds__(AL_THREADS) void allele_sam_kernel(MismatchSamSrc src, AlleleSites sites, uint32_t min_mapq, uint32_t min_baseq, AlleleTables T) {
    if (src.S.W.sum->status) return;
    allele_block<MERGE>(src, src.S.W.sum->n_rec, sites, min_mapq, min_baseq, T, blockIdx.x, gridDim.x);
}

// the record count is on the device: a grid for the most records the window can hold, a record per lane, at most 2048 workgroups (eight
// per CU: a workgroup's end is at most nine LDS atomics per lane and sixteen global ones, so a large grid costs little and hides the
// long records behind the short ones)
void launch_allele_bam(hipStream_t s, const DecodeWindow &W, const AlleleSites &sites, uint32_t min_mapq, uint32_t min_baseq, const AlleleTables &T, bool merge) {
    const dim3 grid(capped_grid(decode_max_records(W), AL_THREADS, 2048u));
    if (merge) allele_bam_kernel<true><<<grid, AL_THREADS, 0, s>>>(MismatchBamSrc{W}, sites, min_mapq, min_baseq, T);
    else allele_bam_kernel<false><<<grid, AL_THREADS, 0, s>>>(MismatchBamSrc{W}, sites, min_mapq, min_baseq, T);
}
void launch_allele_sam(hipStream_t s, const SamWindow &S, const AlleleSites &sites, uint32_t min_mapq, uint32_t min_baseq, const AlleleTables &T, bool merge) {
    const dim3 grid(capped_grid(S.rec_cap, AL_THREADS, 2048u));
    if (merge) allele_sam_kernel<true><<<grid, AL_THREADS, 0, s>>>(MismatchSamSrc{S}, sites, min_mapq, min_baseq, T);
    else allele_sam_kernel<false><<<grid, AL_THREADS, 0, s>>>(MismatchSamSrc{S}, sites, min_mapq, min_baseq, T);
}

}  // namespace rsqc
