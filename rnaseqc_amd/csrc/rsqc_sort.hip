// rsqc_sort.hip -- launchers of the --sort kernels (rsqc_sort.h); the host side that drives them is rsqc_sort_api.cpp.
#define RSQC_SORT_KERNELS
#include "rsqc_sort.h"

namespace rsqc {

static inline uint32_t blocks_for(uint64_t n, uint32_t per_block) { return (uint32_t)((n + per_block - 1) / per_block); }

void launch_sort_append(hipStream_t s, const rsqc_rec_core *core, uint64_t n, const int32_t *seg_tid, const uint64_t *seg_start, uint32_t n_seg, uint64_t *key_out, uint64_t rec0,
                        const uint64_t *wide_index, const int32_t *wide_nm, const int32_t *wide_lq, const uint32_t *wide_nc, uint32_t n_wide,
                        uint64_t *c_wide_index, int32_t *c_wide_nm, int32_t *c_wide_lq, uint32_t *c_wide_nc) {
    const uint64_t lanes = n > n_wide ? n : n_wide;
    if (!lanes) return;
    sort_append_kernel<<<blocks_for(lanes, RSQC_SORT_THREADS), RSQC_SORT_THREADS, 0, s>>>(core, n, seg_tid, seg_start, n_seg, key_out, rec0, wide_index, wide_nm, wide_lq, wide_nc, n_wide,
                                                                                          c_wide_index, c_wide_nm, c_wide_lq, c_wide_nc);
}

void launch_sort_prepare(hipStream_t s, const uint64_t *key, uint64_t n, uint32_t *idx, unsigned long long *part, uint32_t grid) {
    sort_prepare_kernel<<<grid, RSQC_SORT_THREADS, 0, s>>>(key, n, idx, part);
}

void launch_sort_scan(hipStream_t s, uint32_t *data, uint64_t m, unsigned long long *chunk_sum, unsigned long long *total_out) {
    const uint32_t chunks = blocks_for(m, RSQC_SCAN_CHUNK);
    if (chunks) sort_scan_sum_kernel<<<chunks, RSQC_SORT_THREADS, 0, s>>>(data, m, chunk_sum);
    sort_scan_top_kernel<<<1, RSQC_SORT_THREADS, 0, s>>>(chunk_sum, chunks, total_out);
    if (chunks) sort_scan_apply_kernel<<<chunks, RSQC_SORT_THREADS, 0, s>>>(data, m, chunk_sum);
}

void launch_sort_pass(hipStream_t s, const uint64_t *key_in, const uint32_t *idx_in, uint64_t *key_out, uint32_t *idx_out, uint64_t n, int shift,
                      uint32_t *hist, unsigned long long *chunk_sum, unsigned long long *total_out) {
    const uint32_t tiles = blocks_for(n, RSQC_SORT_TILE);
    if (!tiles) return;
    sort_hist_kernel<<<tiles, RSQC_SORT_THREADS, 0, s>>>(key_in, n, shift, hist, tiles);
    launch_sort_scan(s, hist, (uint64_t)256 * tiles, chunk_sum, total_out);
    sort_scatter_kernel<<<tiles, RSQC_SORT_THREADS, 0, s>>>(key_in, idx_in, key_out, idx_out, n, shift, hist, tiles);
}

void launch_sort_gather_count(hipStream_t s, const SortCollection &C, const uint64_t *key, const uint32_t *idx, uint64_t r0, uint32_t n,
                              uint32_t *n_ops, uint32_t *seg_mark, uint32_t *wide_mark, uint32_t *moved_part) {
    sort_gather_count_kernel<<<blocks_for(n, RSQC_SORT_THREADS), RSQC_SORT_THREADS, 0, s>>>(C, key, idx, r0, n, n_ops, seg_mark, wide_mark, moved_part);
}

void launch_sort_gather(hipStream_t s, const SortCollection &C, const uint64_t *key, const uint32_t *idx, uint64_t r0, uint32_t n,
                        const uint32_t *ops_at, const uint32_t *seg_at, const uint32_t *wide_at, uint32_t total_ops, uint32_t n_seg, const SortOutput &O) {
    sort_gather_kernel<<<blocks_for(n, RSQC_SORT_THREADS), RSQC_SORT_THREADS, 0, s>>>(C, key, idx, r0, n, ops_at, seg_at, wide_at, total_ops, n_seg, O);
}

}  // namespace rsqc
