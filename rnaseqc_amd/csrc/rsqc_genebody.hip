// rsqc_genebody.hip -- launcher of the --gene-body kernel (rsqc_genebody.h); the host side that drives it is rsqc_genebody_api.cpp.
#define RSQC_GENEBODY_KERNELS
#include "rsqc_genebody.h"

namespace rsqc {

void launch_genebody_bins(hipStream_t s, const uint32_t *S, const uint64_t *off, const GeneModel &M, const GenebodyItem *items, uint64_t n_items, unsigned long long *sums, unsigned long long *total) {
    if (!n_items) return;
    const uint32_t grid = (uint32_t)((n_items + RSQC_GENEBODY_WAVES - 1) / RSQC_GENEBODY_WAVES);
    genebody_bins_kernel<<<grid, RSQC_GENEBODY_THREADS, 0, s>>>(S, off, M, items, n_items, sums, total);
}

}  // namespace rsqc
