// rsqc_junction.hip -- launchers of the --junctions kernels (rsqc_junction.h); the host side that drives them is rsqc_junction_api.cpp.
#define RSQC_JUNCTION_KERNELS
#include "rsqc_junction.h"

namespace rsqc {

static inline uint32_t blocks_for(uint64_t n, uint32_t per_block) { return (uint32_t)((n + per_block - 1) / per_block); }

void launch_junction_extract(hipStream_t s, const JunctionBatch &B, int32_t n_contigs, uint32_t mapq_threshold, const JunctionCollection &C, int *error) {
    if (!B.n) return;
    junction_extract_kernel<<<blocks_for(B.n, RSQC_JUNC_THREADS), RSQC_JUNC_THREADS, 0, s>>>(B, n_contigs, mapq_threshold, C, error);
}
void launch_junction_widen(hipStream_t s, const uint32_t *end, uint64_t n, uint64_t *key) {
    if (n) junction_widen_kernel<<<blocks_for(n, RSQC_JUNC_THREADS), RSQC_JUNC_THREADS, 0, s>>>(end, n, key);
}
void launch_junction_permute(hipStream_t s, const uint64_t *key_hi, const uint32_t *idx, uint64_t n, uint64_t *key) {
    if (n) junction_permute_kernel<<<blocks_for(n, RSQC_JUNC_THREADS), RSQC_JUNC_THREADS, 0, s>>>(key_hi, idx, n, key);
}
void launch_junction_heads(hipStream_t s, const uint64_t *key, const uint32_t *idx, const uint32_t *end, uint64_t n, uint32_t *mark) {
    if (n) junction_heads_kernel<<<blocks_for(n, RSQC_JUNC_THREADS), RSQC_JUNC_THREADS, 0, s>>>(key, idx, end, n, mark);
}
void launch_junction_reduce(hipStream_t s, const uint64_t *key, const uint32_t *idx, const uint32_t *end, const uint32_t *info, uint64_t n,
                            const uint32_t *row_at, const unsigned long long *total, const JunctionRows &R) {
    if (n) junction_reduce_kernel<<<blocks_for(n, RSQC_JUNC_THREADS), RSQC_JUNC_THREADS, 0, s>>>(key, idx, end, info, n, row_at, total, R);
}

}  // namespace rsqc
