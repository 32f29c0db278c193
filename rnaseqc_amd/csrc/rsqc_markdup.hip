// rsqc_markdup.hip -- launchers of the --mark-duplicates kernels (rsqc_markdup.h); the host side that drives them is rsqc_markdup_api.cpp.
#define RSQC_MARKDUP_KERNELS
#include "rsqc_markdup.h"

namespace rsqc {

static inline uint32_t blocks_for(uint64_t n, uint32_t per_block) { return (uint32_t)((n + per_block - 1) / per_block); }

void launch_markdup_mark(hipStream_t s, const MarkdupCollection &C, uint32_t *block_anchors, unsigned long long *counters) {
    if (!C.n) return;
    markdup_mark_kernel<<<blocks_for(C.n, RSQC_MD_THREADS), RSQC_MD_THREADS, 0, s>>>(C, block_anchors, counters);
}

void launch_markdup_signature(hipStream_t s, const MarkdupCollection &C, const uint32_t *block_slot, uint64_t n_anchors, uint64_t *k_hi, uint64_t *k_lo, uint64_t *k_lo_sort, uint32_t *ci) {
    if (!C.n || !n_anchors) return;
    markdup_signature_kernel<<<blocks_for(C.n, RSQC_MD_THREADS), RSQC_MD_THREADS, 0, s>>>(C, block_slot, n_anchors, k_hi, k_lo, k_lo_sort, ci);
}

void launch_markdup_permute(hipStream_t s, const uint64_t *k_hi, const uint32_t *idx, uint64_t n, uint64_t *key) {
    if (!n) return;
    markdup_permute_kernel<<<blocks_for(n, RSQC_MD_THREADS), RSQC_MD_THREADS, 0, s>>>(k_hi, idx, n, key);
}

void launch_markdup_heads(hipStream_t s, const uint64_t *key, const uint32_t *idx, const uint64_t *k_lo, uint64_t n, uint32_t *mark) {
    if (!n) return;
    markdup_heads_kernel<<<blocks_for(n, RSQC_MD_THREADS), RSQC_MD_THREADS, 0, s>>>(key, idx, k_lo, n, mark);
}

void launch_markdup_list(hipStream_t s, const uint32_t *at, const unsigned long long *total, const uint32_t *idx, const uint32_t *ci, uint64_t n, uint32_t *dup_list) {
    if (!n) return;
    markdup_list_kernel<<<blocks_for(n, RSQC_MD_THREADS), RSQC_MD_THREADS, 0, s>>>(at, total, idx, ci, n, dup_list);
}

void launch_markdup_umi_keys(hipStream_t s, const MarkdupCollection &C, const uint32_t *ci, uint64_t n_anchors, uint64_t *k_umi, unsigned long long *counters) {
    if (!n_anchors) return;
    markdup_umi_keys_kernel<<<blocks_for(n_anchors, RSQC_MD_THREADS), RSQC_MD_THREADS, 0, s>>>(C, ci, n_anchors, k_umi, counters);
}

void launch_markdup_heads_umi(hipStream_t s, const uint64_t *key, const uint32_t *idx, const uint64_t *k_lo, const uint64_t *k_umi, uint64_t n, uint32_t *mark, unsigned long long *counters) {
    if (!n) return;
    markdup_heads_umi_kernel<<<blocks_for(n, RSQC_MD_THREADS), RSQC_MD_THREADS, 0, s>>>(key, idx, k_lo, k_umi, n, mark, counters);
}

void launch_markdup_heads_pos(hipStream_t s, const uint64_t *key, const uint32_t *idx, const uint64_t *k_lo, uint64_t n, uint32_t *mark_pos) {
    if (!n) return;
    markdup_heads_pos_kernel<<<blocks_for(n, RSQC_MD_THREADS), RSQC_MD_THREADS, 0, s>>>(key, idx, k_lo, n, mark_pos);
}

void launch_markdup_group_nodes(hipStream_t s, const uint32_t *at, const uint32_t *at_pos, const unsigned long long *tot, const uint32_t *idx, const uint64_t *k_lo, const uint64_t *k_umi, uint64_t n,
                                uint64_t *node_key, uint32_t *node_head, uint64_t *node_best, uint32_t *node_set, uint32_t *set_first, unsigned long long *group_best) {
    if (!n) return;
    markdup_group_nodes_kernel<<<blocks_for(n, RSQC_MD_THREADS), RSQC_MD_THREADS, 0, s>>>(at, at_pos, tot, idx, k_lo, k_umi, n, node_key, node_head, node_best, node_set, set_first, group_best);
}

void launch_markdup_group_parents(hipStream_t s, const uint64_t *node_key, const uint32_t *node_head, const uint32_t *node_set, const uint32_t *set_first, uint32_t n_nodes, uint32_t n_sets,
                                  uint32_t *parent, unsigned long long *counters) {
    if (!n_nodes) return;
    markdup_group_parents_kernel<<<blocks_for(n_nodes, RSQC_MD_THREADS), RSQC_MD_THREADS, 0, s>>>(node_key, node_head, node_set, set_first, n_nodes, n_sets, parent, counters);
}

void launch_markdup_group_roots(hipStream_t s, const uint32_t *parent, const uint32_t *node_set, const uint32_t *set_first, const uint64_t *node_best, uint32_t n_nodes, uint32_t n_sets, uint32_t *root,
                                unsigned long long *group_best) {
    if (!n_nodes) return;
    markdup_group_roots_kernel<<<blocks_for(n_nodes, RSQC_MD_THREADS), RSQC_MD_THREADS, 0, s>>>(parent, node_set, set_first, node_best, n_nodes, n_sets, root, group_best);
}

void launch_markdup_group_marks(hipStream_t s, const uint32_t *at, const unsigned long long *tot, const uint32_t *idx, const uint64_t *k_lo, const uint32_t *root, const unsigned long long *group_best,
                                uint64_t n, uint32_t n_nodes, uint32_t *mark) {
    if (!n) return;
    markdup_group_marks_kernel<<<blocks_for(n, RSQC_MD_THREADS), RSQC_MD_THREADS, 0, s>>>(at, tot, idx, k_lo, root, group_best, n, n_nodes, mark);
}

void launch_markdup_insert(hipStream_t s, const MarkdupCollection &C, const uint32_t *dup_list, uint64_t n_dup, uint32_t *table, uint32_t mask) {
    if (!n_dup) return;
    markdup_insert_kernel<<<blocks_for(n_dup, RSQC_MD_THREADS), RSQC_MD_THREADS, 0, s>>>(C, dup_list, n_dup, table, mask);
}

void launch_markdup_apply(hipStream_t s, const MarkdupCollection &C, const uint32_t *dup_list, uint64_t n_dup, const uint32_t *table, uint32_t mask, uint8_t *verdict, unsigned long long *counters) {
    if (!C.n) return;
    markdup_apply_kernel<<<blocks_for(C.n, RSQC_MD_THREADS), RSQC_MD_THREADS, 0, s>>>(C, dup_list, n_dup, table, mask, verdict, counters);
}

}  // namespace rsqc
