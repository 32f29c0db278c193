// rsqc_tin.hip -- launchers of the --tin kernels (rsqc_tin.h); the host side that drives them is rsqc_tin_api.cpp.
#define RSQC_TIN_KERNELS
#include "rsqc_tin.h"

namespace rsqc {

void launch_tin_items(hipStream_t s, const uint32_t *S, const uint64_t *off, const GeneModel &M, const TinItem *items, uint64_t n_items, rsqc_tin_row *part) {
    if (!n_items) return;
    const uint32_t grid = (uint32_t)((n_items + RSQC_TIN_WAVES - 1) / RSQC_TIN_WAVES);
    tin_items_kernel<<<grid, RSQC_TIN_THREADS, 0, s>>>(S, off, M, items, n_items, part);
}

void launch_tin_rows(hipStream_t s, const rsqc_tin_row *part, const uint64_t *item_off, uint32_t n_genes, rsqc_tin_row *rows) {
    if (!n_genes) return;
    const uint32_t grid = (n_genes + RSQC_TIN_THREADS - 1) / RSQC_TIN_THREADS;
    tin_rows_kernel<<<grid, RSQC_TIN_THREADS, 0, s>>>(part, item_off, n_genes, rows);
}

}  // namespace rsqc
