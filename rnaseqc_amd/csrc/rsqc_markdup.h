// rsqc_markdup.h -- the kernels of --mark-duplicates (rsqc_markdup_begin / rsqc_markdup_end / rsqc_markdup_verdicts): one block of
// work at the head of rsqc_sort_end, on the complete collection, that rewrites flag bit 0x400 of every record.  The contract is
// written out in include/rnaseqc_amd.h and restated in tests/markdup_ref.py.  Written like rsqc_sort.h against the HIP wave
// intrinsics only (__ballot, __shfl*, LDS, global atomics): the same source runs under the 64-lane emulation of
// tests/hostemu/wavemu.h (tests/hostemu/markdup_emu.cpp).  No rocPRIM.  One lane per item everywhere:
//
//   markdup_mark_kernel        per record the anchor predicate; a workgroup leaves the NUMBER of its anchors (and adds its population
//                              records to a counter with one atomic).  launch_sort_scan over those per-workgroup numbers gives every
//                              workgroup its first slot -- 4 bytes per 256 records instead of 4 per record
//   markdup_signature_kernel   the predicate again, a workgroup scan for the slot inside the workgroup (lanes are records in arrival
//                              order, so slots keep that order: the tie rule needs it), and per anchor K_hi, K_lo and its collection index
//   (the order: rsqc_sort.h's radix pass, launch_sort_pass, LSD in two stages -- by K_lo with the slot as payload, then stably by K_hi
//    gathered through the payload with markdup_permute_kernel; dead digit positions are skipped in both)
//   markdup_heads_kernel       1 where a sorted anchor has the signature of its predecessor: a duplicate anchor
//   markdup_list_kernel        after the prefix sum of those marks: D, the collection indices of the duplicate anchors
//   markdup_insert_kernel      the names of D into an open-addressing table of uint32 slots (index in D), linear probing from
//                              qhash & mask; names are compared through D's records, which are complete before the kernel: WHICH index
//                              of an equal name wins a slot depends on the schedule, whether a name is in the table does not
//   markdup_apply_kernel       per record: probe until an equal name or an empty slot, rewrite the flag of its OWN record (a 16-bit
//                              store: other lanes read the qhash beside it), the verdict byte, and two counters -- a ballot and a
//                              popcount per wave, then one atomic per wave and counter
//
// rsqc_markdup_use_umi (--umi-tag / --umi-qname): the anchor's UMI key (rsqc_umi.h) is the LAST component of the signature.  Two more
// kernels, every kernel above unchanged:
//   markdup_umi_keys_kernel    per anchor slot its record's key from the collection's umi column (through ci), and how many are not 0
//   (the order becomes (K_hi, K_lo >> 8, umi, 255 - mapq, arrival): LSD in FOUR stages of the same radix pass -- the mapq byte of K_lo,
//    the live digits of the UMI keys, K_lo above its mapq byte, K_hi -- each stage's keys gathered through the payload of the stage
//    before with markdup_permute_kernel; a stage without a live digit is skipped with its gather.  The UMI has to rank ABOVE the mapq
//    byte: below it, anchors of one signature and UMI but different mapq would not be adjacent)
//   markdup_heads_umi_kernel   1 where signature AND key are the predecessor's; beside it the number of anchors whose signature alone
//                              is the predecessor's -- what the marking without the UMI would have called (position_duplicate_fragments)
//
// rsqc_markdup_umi_edits(1) (--umi-edits=1): the last component is the ROOT of the anchor's UMI -- UMIs of one position set that are one
// substitution apart merge towards the higher count (the contract: include/rnaseqc_amd.h, tests/markdup_umi_group_ref.py).  Five more
// kernels between the heads and the list, every kernel above unchanged:
//   markdup_heads_pos_kernel      1 where the position signature alone is the predecessor's; with the marks above and two scans every
//                                 rank knows its node (a distinct UMI of a position set) and its set
//   markdup_group_nodes_kernel    head ranks write the node columns: key, head rank (counts are differences), best anchor, set
//   markdup_group_parents_kernel  the hot one: per node 3 L neighbour keys, each a binary search among the nodes of its own set
//   markdup_group_roots_kernel    parent[] walked to the root (into a separate column), the node's best anchor merged into the root's
//   markdup_group_marks_kernel    per rank: a duplicate unless it is its group's best anchor; then the scan and the list as ever
#pragma once

#if !defined(RSQC_WAVE_EMU)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "../../include/rnaseqc_amd.h"

#define RSQC_MD_THREADS 256
#define RSQC_MD_EMPTY 0xFFFFFFFFu
#define RSQC_MD_MIN_TABLE 1024u
#define RSQC_MD_EXCLUDED (RSQC_FUNMAP | RSQC_FSECONDARY | RSQC_FQCFAIL | RSQC_FSUPP)
#define RSQC_MD_SINGLE 0u
#define RSQC_MD_PAIR 1u
#define RSQC_MD_SPLIT 2u

namespace rsqc {

// the collection of rsqc_sort_begin as this stage reads it (device pointers).  `aux` is written: the flag of every record
struct MarkdupCollection {
    const rsqc_rec_core *core; rsqc_rec_aux *aux; const uint32_t *qhash2 /* or null: the name is qhash alone */; const uint64_t *key; const uint32_t *cigar;
    uint64_t n;                                                        // records
    const uint64_t *batch_rec0, *batch_pool0; uint32_t n_batches;      // first record / first operation of input batch k
    const uint64_t *wide_index; const uint32_t *wide_n_cigar; uint64_t n_wide;
    uint64_t n_ops;                                                    // operations in `cigar`: no record reads past them
    const uint64_t *umi;                                               // rsqc_markdup_use_umi: the records' UMI keys; null otherwise (no kernel above the _umi ones reads it)
};

// the size of the name table for n_dup duplicate anchors: a power of two, at least twice their number and at least 1024
inline uint64_t markdup_table_size(uint64_t n_dup) {
    uint64_t s = RSQC_MD_MIN_TABLE;
    while (s < 2 * n_dup) s <<= 1;
    return s;
}

#if defined(RSQC_MARKDUP_KERNELS) || defined(RSQC_WAVE_EMU)      /* the kernels: rsqc_markdup.hip and the emulation only */
// exclusive prefix sum over the 256 lanes of a workgroup (every lane calls); total = the sum over all of them
__device__ inline uint32_t md_block_scan(uint32_t v, uint32_t &total) {
    __shared__ uint32_t s_wave[RSQC_MD_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t x = v;
    for (uint32_t o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(x, o, 64); if (lane >= o) x += t; }
    if (lane == 63) s_wave[w] = x;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (uint32_t k = 0; k < RSQC_MD_THREADS / 64; ++k) { const uint32_t s = s_wave[k]; if (k < w) base += s; tot += s; }
    __syncthreads();                                   // (the next call writes s_wave again)
    total = tot;
    return base + x - v;
}

// population and anchor of record i (i < C.n): kind is set for an anchor
__device__ inline bool md_is_anchor(const MarkdupCollection &C, uint64_t i, const rsqc_rec_aux &a, bool &member, uint32_t &kind) {
    const int32_t tid = (int32_t)(uint32_t)(C.key[i] >> 32);
    member = (a.flag & RSQC_MD_EXCLUDED) == 0 && tid >= 0;
    kind = RSQC_MD_SINGLE;
    if (!member) return false;
    if (!(a.flag & RSQC_FPAIRED) || (a.flag & RSQC_FMUNMAP)) return true;
    if (a.tagbits & RSQC_TB_MTID_SAME) {
        kind = RSQC_MD_PAIR;
        const rsqc_rec_core c = C.core[i];
        return c.pos < c.mpos || (c.pos == c.mpos && (a.flag & RSQC_FREAD1));
    }
    kind = RSQC_MD_SPLIT;
    return (a.flag & RSQC_FREAD1) != 0;
}

// the unclipped 5' coordinate of record i, in 32-bit two's-complement arithmetic
__device__ inline uint32_t md_u5(const MarkdupCollection &C, uint64_t i, const rsqc_rec_core &c, const rsqc_rec_aux &a) {
    uint32_t n_ops = a.n_cigar;
    if (a.n_cigar == RSQC_NCIGAR_ESCAPE) {             // the true count is in the wide table (an escape value without an entry: no operations)
        uint64_t lo = 0, hi = C.n_wide;
        while (lo < hi) { const uint64_t m = (lo + hi) >> 1; if (C.wide_index[m] < i) lo = m + 1; else hi = m; }
        n_ops = (lo < C.n_wide && C.wide_index[lo] == i) ? C.wide_n_cigar[lo] : 0u;
    }
    // the input batch of the record: the last one that starts at or before it (cigar_off is relative to ITS pool)
    uint32_t lo = 0, hi = C.n_batches;
    while (hi - lo > 1) { const uint32_t m = (lo + hi) >> 1; if (C.batch_rec0[m] <= i) lo = m; else hi = m; }
    const uint64_t src = C.batch_pool0[lo] + c.cigar_off;
    if (src >= C.n_ops) n_ops = 0u; else if ((uint64_t)n_ops > C.n_ops - src) n_ops = (uint32_t)(C.n_ops - src);
    const uint32_t *ops = C.cigar + src;
    uint32_t u = (uint32_t)c.pos;
    if (!(a.flag & RSQC_FREVERSE)) {
        for (uint32_t k = 0; k < n_ops; ++k) {
            const uint32_t op = ops[k], code = op & 15u;
            if (code != 4u && code != 5u) break;
            u -= op >> 4;
        }
        return u;
    }
    uint32_t trail = 0; bool in_tail = true;           // from the last operation down: the trailing run of S / H ends at the first other code
    for (uint32_t k = n_ops; k > 0; --k) {
        const uint32_t op = ops[k - 1], code = op & 15u, len = op >> 4;
        if (in_tail && (code == 4u || code == 5u)) { trail += len; continue; }
        in_tail = false;
        if (code == 0u || code == 2u || code == 3u || code == 7u || code == 8u) u += len;
    }
    return u + trail;
}

__device__ inline bool md_same_name(const MarkdupCollection &C, uint64_t i, uint64_t qhash, uint32_t qh2) {
    return C.aux[i].qhash == qhash && (!C.qhash2 || C.qhash2[i] == qh2);
}

// ---- stage 1: the anchors of every workgroup -----------------------------------------------------------------------------------
__global__ __launch_bounds__(RSQC_MD_THREADS) void markdup_mark_kernel(MarkdupCollection C, uint32_t *block_anchors, unsigned long long *counters /* [0] population */) {
    const uint64_t i = (uint64_t)blockIdx.x * RSQC_MD_THREADS + threadIdx.x;
    bool member = false, anchor = false; uint32_t kind;
    if (i < C.n) anchor = md_is_anchor(C, i, C.aux[i], member, kind);
    uint32_t anchors = 0, members = 0;
    (void)md_block_scan(anchor ? 1u : 0u, anchors);
    (void)md_block_scan(member ? 1u : 0u, members);
    if (threadIdx.x == 0) {
        block_anchors[blockIdx.x] = anchors;
        if (members) atomicAdd(&counters[0], (unsigned long long)members);
    }
}

// ---- stage 2: block_slot = the exclusive prefix sum of block_anchors; n_anchors = their sum ------------------------------------
__global__ __launch_bounds__(RSQC_MD_THREADS) void markdup_signature_kernel(MarkdupCollection C, const uint32_t *block_slot, uint64_t n_anchors,
                                                                             uint64_t *k_hi, uint64_t *k_lo, uint64_t *k_lo_sort /* a second copy: the sort's first buffer */, uint32_t *ci) {
    const uint64_t i = (uint64_t)blockIdx.x * RSQC_MD_THREADS + threadIdx.x;
    bool member = false, anchor = false; uint32_t kind = 0;
    rsqc_rec_aux a{};
    if (i < C.n) { a = C.aux[i]; anchor = md_is_anchor(C, i, a, member, kind); }
    uint32_t total = 0;
    const uint32_t at = md_block_scan(anchor ? 1u : 0u, total);
    if (!anchor) return;
    const uint64_t slot = (uint64_t)block_slot[blockIdx.x] + at;
    if (slot >= n_anchors) return;                     // (never: a store is not let out of the columns)
    const rsqc_rec_core c = C.core[i];
    const uint32_t u5 = md_u5(C, i, c, a);
    const uint32_t w = kind == RSQC_MD_PAIR ? (uint32_t)c.isize : kind == RSQC_MD_SPLIT ? (uint32_t)c.mpos : 0u;
    const uint32_t rev = (a.flag & RSQC_FREVERSE) ? 1u : 0u, mrev = (kind != RSQC_MD_SINGLE && (a.flag & RSQC_FMREVERSE)) ? 1u : 0u;
    const uint64_t hi = (C.key[i] & 0xFFFFFFFF00000000ull) | (uint64_t)(u5 ^ 0x80000000u);
    const uint64_t lo = ((uint64_t)w << 32) | (uint64_t)(kind << 10) | (uint64_t)(rev << 9) | (uint64_t)(mrev << 8) | (uint64_t)(255u - (uint32_t)a.mapq);
    k_hi[slot] = hi; k_lo[slot] = lo; k_lo_sort[slot] = lo; ci[slot] = (uint32_t)i;
}

// ---- stage 3 (between the two sort stages): K_hi in the order of the first stage ------------------------------------------------
__global__ __launch_bounds__(RSQC_MD_THREADS) void markdup_permute_kernel(const uint64_t *k_hi, const uint32_t *idx, uint64_t n, uint64_t *key) {
    const uint64_t r = (uint64_t)blockIdx.x * RSQC_MD_THREADS + threadIdx.x;
    if (r < n) { const uint32_t s = idx[r]; key[r] = s < n ? k_hi[s] : 0ull; }
}

// ---- stage 4: key = K_hi in sorted order, idx[r] = the slot of rank r, k_lo by slot ---------------------------------------------
__global__ __launch_bounds__(RSQC_MD_THREADS) void markdup_heads_kernel(const uint64_t *key, const uint32_t *idx, const uint64_t *k_lo, uint64_t n, uint32_t *mark) {
    const uint64_t r = (uint64_t)blockIdx.x * RSQC_MD_THREADS + threadIdx.x;
    if (r >= n) return;
    uint32_t dup = 0u;
    if (r > 0 && key[r] == key[r - 1]) {
        const uint32_t s = idx[r], p = idx[r - 1];
        if (s < n && p < n && (k_lo[s] >> 8) == (k_lo[p] >> 8)) dup = 1u;
    }
    mark[r] = dup;
}
// at: the exclusive prefix sum of the marks, total[0] their sum: rank r is a duplicate when the sum moves on behind it
__global__ __launch_bounds__(RSQC_MD_THREADS) void markdup_list_kernel(const uint32_t *at, const unsigned long long *total, const uint32_t *idx, const uint32_t *ci, uint64_t n, uint32_t *dup_list) {
    const uint64_t r = (uint64_t)blockIdx.x * RSQC_MD_THREADS + threadIdx.x;
    if (r >= n) return;
    const uint32_t before = at[r], through = r + 1 < n ? at[r + 1] : (uint32_t)total[0];
    const uint32_t s = idx[r];
    if (through != before && (uint64_t)before < total[0] && s < n) dup_list[before] = ci[s];
}

// ---- rsqc_markdup_use_umi: the UMI key is the LAST component of the signature ----------------------------------------------------
// stage 2b: the anchors' own keys by slot, gathered through ci; counters[3] += anchors whose key is not 0
__global__ __launch_bounds__(RSQC_MD_THREADS) void markdup_umi_keys_kernel(MarkdupCollection C, const uint32_t *ci, uint64_t n_anchors, uint64_t *k_umi, unsigned long long *counters) {
    const uint64_t a = (uint64_t)blockIdx.x * RSQC_MD_THREADS + threadIdx.x;
    uint64_t u = 0;
    if (a < n_anchors) {
        const uint64_t i = ci[a];
        if (C.umi && i < C.n) u = C.umi[i];
        k_umi[a] = u;
    }
    uint32_t with = 0;                                 // (one atomic per workgroup: nearly every wave has such an anchor, and they all add to ONE word)
    (void)md_block_scan(u != 0 ? 1u : 0u, with);
    if (threadIdx.x == 0 && with) atomicAdd(&counters[3], (unsigned long long)with);
}
// stage 4 in this mode.  The order is (K_hi, K_lo >> 8, umi, 255 - mapq, arrival): anchors of one position signature are adjacent, and
// inside them the anchors of one UMI.  mark = 1 where signature AND UMI are the predecessor's; counters[4] += anchors whose position
// signature alone is the predecessor's -- the duplicate fragments of a marking without the UMI
__global__ __launch_bounds__(RSQC_MD_THREADS) void markdup_heads_umi_kernel(const uint64_t *key, const uint32_t *idx, const uint64_t *k_lo, const uint64_t *k_umi, uint64_t n, uint32_t *mark,
                                                                             unsigned long long *counters) {
    const uint64_t r = (uint64_t)blockIdx.x * RSQC_MD_THREADS + threadIdx.x;
    bool pos_dup = false, dup = false;
    if (r < n) {
        if (r > 0 && key[r] == key[r - 1]) {
            const uint32_t s = idx[r], p = idx[r - 1];
            if (s < n && p < n && (k_lo[s] >> 8) == (k_lo[p] >> 8)) { pos_dup = true; dup = k_umi[s] == k_umi[p]; }
        }
        mark[r] = dup ? 1u : 0u;
    }
    uint32_t pm = 0;
    (void)md_block_scan(pos_dup ? 1u : 0u, pm);
    if (threadIdx.x == 0 && pm) atomicAdd(&counters[4], (unsigned long long)pm);
}

// ---- rsqc_markdup_umi_edits(1): the signature's last component is the ROOT of the anchor's UMI ------------------------------------
// Ranks are in the order above, so a position set is a run of ranks and its distinct UMIs -- the NODES -- ascend inside it.  at / at_pos:
// the exclusive prefix sums of markdup_heads_umi_kernel's marks and of the position marks below, tot[0] / tot[1] their sums.  A rank
// whose sum does not move on behind it is a head; the node of rank r is r - (the sum through r), its set likewise.
__global__ __launch_bounds__(RSQC_MD_THREADS) void markdup_heads_pos_kernel(const uint64_t *key, const uint32_t *idx, const uint64_t *k_lo, uint64_t n, uint32_t *mark_pos) {
    const uint64_t r = (uint64_t)blockIdx.x * RSQC_MD_THREADS + threadIdx.x;
    if (r >= n) return;
    uint32_t same = 0u;
    if (r > 0 && key[r] == key[r - 1]) {
        const uint32_t s = idx[r], p = idx[r - 1];
        if (s < n && p < n && (k_lo[s] >> 8) == (k_lo[p] >> 8)) same = 1u;
    }
    mark_pos[r] = same;
}
// the head rank of a node writes its columns: the key, the rank itself (node_head; the count of node m is node_head[m + 1] -
// node_head[m], node_head[n_nodes] = n), its set, and node_best = ((255 - mapq) << 32) | slot of the head anchor -- the order makes the
// head the node's best anchor, slots are in arrival order.  A set's head writes set_first[set]; set_first[n_sets] = n_nodes
__global__ __launch_bounds__(RSQC_MD_THREADS) void markdup_group_nodes_kernel(const uint32_t *at, const uint32_t *at_pos, const unsigned long long *tot, const uint32_t *idx, const uint64_t *k_lo,
                                                                               const uint64_t *k_umi, uint64_t n, uint64_t *node_key, uint32_t *node_head, uint64_t *node_best, uint32_t *node_set,
                                                                               uint32_t *set_first, unsigned long long *group_best) {
    const uint64_t r = (uint64_t)blockIdx.x * RSQC_MD_THREADS + threadIdx.x;
    if (r >= n || tot[0] >= n || tot[1] >= n) return;
    const uint32_t n_nodes = (uint32_t)(n - tot[0]), n_sets = (uint32_t)(n - tot[1]);
    if (r == 0) { node_head[n_nodes] = (uint32_t)n; set_first[n_sets] = n_nodes; }
    const uint32_t before = at[r], through = r + 1 < n ? at[r + 1] : (uint32_t)tot[0];
    if (through != before) return;                     // not a head
    const uint32_t before_pos = at_pos[r], through_pos = r + 1 < n ? at_pos[r + 1] : (uint32_t)tot[1];
    const uint32_t node = (uint32_t)r - before, set = (uint32_t)r - through_pos;
    if (node >= n_nodes || set >= n_sets) return;      // (never: a store is not let out of the columns)
    const uint32_t s = idx[r];
    node_key[node] = s < n ? k_umi[s] : 0ull;
    node_best[node] = s < n ? ((k_lo[s] & 0xFFull) << 32) | (uint64_t)s : ~0ull;
    node_head[node] = (uint32_t)r; node_set[node] = set;
    group_best[node] = ~0ull;
    if (through_pos == before_pos) set_first[set] = node;
}
// the node that holds key q in node_key[lo, hi) (ascending), or RSQC_MD_EMPTY
__device__ inline uint32_t md_find_node(const uint64_t *node_key, uint32_t lo, uint32_t hi, uint64_t q) {
    const uint32_t end = hi;
    while (lo < hi) { const uint32_t m = lo + ((hi - lo) >> 1); if (node_key[m] < q) lo = m + 1; else hi = m; }
    return (lo < end && node_key[lo] == q) ? lo : RSQC_MD_EMPTY;
}
// one lane per node: the 3 L keys one substitution from its own -- k ^ (x << 2j), never the length bit -- are looked up in the nodes
// of ITS set only (a smaller key in front of the node, a larger one behind it).  parent = the eligible neighbour with the highest
// count, ties to the smallest key; eligible: count(p) >= 2 count(k) - 1 in 64 bits, and count(p) > count(k) or equal with p < k.
// Key 0 has no neighbours.  counters[5] += nodes with a parent, [6] += nodes, [7] += keys looked up: one atomic per workgroup each
__global__ __launch_bounds__(RSQC_MD_THREADS) void markdup_group_parents_kernel(const uint64_t *node_key, const uint32_t *node_head, const uint32_t *node_set, const uint32_t *set_first,
                                                                                 uint32_t n_nodes, uint32_t n_sets, uint32_t *parent, unsigned long long *counters) {
    const uint64_t nd64 = (uint64_t)blockIdx.x * RSQC_MD_THREADS + threadIdx.x;
    uint32_t best = RSQC_MD_EMPTY, probes = 0;
    if (nd64 < n_nodes) {
        const uint32_t nd = (uint32_t)nd64, set = node_set[nd];
        const uint64_t k = node_key[nd];
        if (k != 0 && set < n_sets) {
            const uint32_t lo = set_first[set], hi = set_first[set + 1] < n_nodes ? set_first[set + 1] : n_nodes;
            if (lo <= nd && nd < hi && hi - lo > 1) {
                const uint32_t c = node_head[nd + 1] - node_head[nd];
                const uint64_t need = 2ull * c - 1ull;
                const uint32_t L = (uint32_t)(63 - __builtin_clzll(k)) >> 1;
                uint32_t best_c = 0; uint64_t best_key = 0;
                for (uint32_t j = 0; j < L; ++j)
                    for (uint64_t x = 1; x < 4; ++x) {
                        const uint64_t q = k ^ (x << (2 * j));
                        const uint32_t m = q < k ? md_find_node(node_key, lo, nd, q) : md_find_node(node_key, nd + 1, hi, q);
                        if (m == RSQC_MD_EMPTY) continue;
                        const uint32_t cp = node_head[m + 1] - node_head[m];
                        if ((uint64_t)cp >= need && (cp > c || (cp == c && q < k)) && (cp > best_c || (cp == best_c && q < best_key))) { best = m; best_c = cp; best_key = q; }
                    }
                probes = 3 * L;
            }
        }
        parent[nd] = best;
    }
    uint32_t merged = 0, nodes = 0, looked = 0;
    (void)md_block_scan(best != RSQC_MD_EMPTY ? 1u : 0u, merged);
    (void)md_block_scan(nd64 < n_nodes ? 1u : 0u, nodes);
    (void)md_block_scan(probes, looked);
    if (threadIdx.x == 0) {
        if (merged) atomicAdd(&counters[5], (unsigned long long)merged);
        if (nodes) atomicAdd(&counters[6], (unsigned long long)nodes);
        if (looked) atomicAdd(&counters[7], (unsigned long long)looked);
    }
}
// every node walks parent[] (read only: nothing is written in place, so nothing races) to its root -- at most as many steps as its set
// has nodes -- writes root[] and merges its best anchor into the root's: group_best[] is all ones before the kernel
__global__ __launch_bounds__(RSQC_MD_THREADS) void markdup_group_roots_kernel(const uint32_t *parent, const uint32_t *node_set, const uint32_t *set_first, const uint64_t *node_best,
                                                                               uint32_t n_nodes, uint32_t n_sets, uint32_t *root, unsigned long long *group_best) {
    const uint64_t nd = (uint64_t)blockIdx.x * RSQC_MD_THREADS + threadIdx.x;
    if (nd >= n_nodes) return;
    const uint32_t set = node_set[nd];
    const uint32_t size = set < n_sets ? set_first[set + 1] - set_first[set] : 0u;
    uint32_t r = (uint32_t)nd;
    for (uint32_t step = 0; step < size; ++step) { const uint32_t p = parent[r]; if (p >= n_nodes) break; r = p; }
    root[nd] = r;
    // a 64-bit minimum as a compare-and-swap loop (the first guess is the value the column starts with): the one 64-bit atomic besides
    // the add that the kernels of this file are written against
    const unsigned long long v = (unsigned long long)node_best[nd];
    unsigned long long old = ~0ull;
    while (v < old) { const unsigned long long seen = atomicCAS(&group_best[r], old, v); if (seen == old) break; old = seen; }
}
// per rank: a duplicate exactly when the anchor is not the best of its root's group.  These marks take the way of the plain ones
__global__ __launch_bounds__(RSQC_MD_THREADS) void markdup_group_marks_kernel(const uint32_t *at, const unsigned long long *tot, const uint32_t *idx, const uint64_t *k_lo, const uint32_t *root,
                                                                               const unsigned long long *group_best, uint64_t n, uint32_t n_nodes, uint32_t *mark) {
    const uint64_t r = (uint64_t)blockIdx.x * RSQC_MD_THREADS + threadIdx.x;
    if (r >= n) return;
    const uint32_t through = r + 1 < n ? at[r + 1] : (uint32_t)tot[0];
    const uint32_t node = (uint32_t)r - through, s = idx[r];
    uint32_t dup = 0u;
    if (s < n && node < n_nodes) {
        const uint32_t rt = root[node];
        if (rt < n_nodes) dup = ((((k_lo[s] & 0xFFull) << 32) | (uint64_t)s) != group_best[rt]) ? 1u : 0u;
    }
    mark[r] = dup;
}

// ---- stage 5: the names of the duplicate anchors; table: mask + 1 slots, all RSQC_MD_EMPTY --------------------------------------
__global__ __launch_bounds__(RSQC_MD_THREADS) void markdup_insert_kernel(MarkdupCollection C, const uint32_t *dup_list, uint64_t n_dup, uint32_t *table, uint32_t mask) {
    const uint64_t j = (uint64_t)blockIdx.x * RSQC_MD_THREADS + threadIdx.x;
    if (j >= n_dup) return;
    const uint64_t i = dup_list[j];
    if (i >= C.n) return;
    const uint64_t qhash = C.aux[i].qhash; const uint32_t qh2 = C.qhash2 ? C.qhash2[i] : 0u;
    uint32_t h = (uint32_t)qhash & mask;
    for (uint32_t step = 0; step <= mask; ++step) {    // (the table is at most half full: an empty slot comes long before the probe wraps)
        const uint32_t old = atomicCAS(&table[h], RSQC_MD_EMPTY, (uint32_t)j);
        if (old == RSQC_MD_EMPTY) return;              // inserted
        if ((uint64_t)old < n_dup) { const uint64_t o = dup_list[old]; if (o < C.n && md_same_name(C, o, qhash, qh2)) return; }   // the name is there
        h = (h + 1u) & mask;
    }
}

// ---- stage 6: table == nullptr: no duplicate anchor, every record leaves with 0x400 clear ---------------------------------------
__global__ __launch_bounds__(RSQC_MD_THREADS) void markdup_apply_kernel(MarkdupCollection C, const uint32_t *dup_list, uint64_t n_dup, const uint32_t *table, uint32_t mask,
                                                                         uint8_t *verdict, unsigned long long *counters /* [1] flagged, [2] cleared */) {
    const uint64_t i = (uint64_t)blockIdx.x * RSQC_MD_THREADS + threadIdx.x;
    bool dup = false, cleared = false;
    if (i < C.n) {
        const rsqc_rec_aux a = C.aux[i];
        if (table) {
            const uint32_t qh2 = C.qhash2 ? C.qhash2[i] : 0u;
            uint32_t h = (uint32_t)a.qhash & mask;
            for (uint32_t step = 0; step <= mask; ++step) {
                const uint32_t s = table[h];
                if (s == RSQC_MD_EMPTY) break;
                if ((uint64_t)s < n_dup) { const uint64_t o = dup_list[s]; if (o < C.n && md_same_name(C, o, a.qhash, qh2)) { dup = true; break; } }
                h = (h + 1u) & mask;
            }
        }
        cleared = (a.flag & RSQC_FDUP) && !dup;
        const uint16_t flag = (uint16_t)((a.flag & ~RSQC_FDUP) | (dup ? RSQC_FDUP : 0));
        if (flag != a.flag) C.aux[i].flag = flag;
        verdict[i] = dup ? 1u : 0u;
    }
    const unsigned long long dmask = __ballot(dup), cmask = __ballot(cleared);
    if ((threadIdx.x & 63u) == 0u) {
        if (dmask) atomicAdd(&counters[1], (unsigned long long)__popcll(dmask));
        if (cmask) atomicAdd(&counters[2], (unsigned long long)__popcll(cmask));
    }
}
#endif

#if !defined(RSQC_WAVE_EMU)
// launchers (rsqc_markdup.hip)
void launch_markdup_mark(hipStream_t s, const MarkdupCollection &C, uint32_t *block_anchors, unsigned long long *counters);
void launch_markdup_signature(hipStream_t s, const MarkdupCollection &C, const uint32_t *block_slot, uint64_t n_anchors, uint64_t *k_hi, uint64_t *k_lo, uint64_t *k_lo_sort, uint32_t *ci);
void launch_markdup_permute(hipStream_t s, const uint64_t *k_hi, const uint32_t *idx, uint64_t n, uint64_t *key);
void launch_markdup_heads(hipStream_t s, const uint64_t *key, const uint32_t *idx, const uint64_t *k_lo, uint64_t n, uint32_t *mark);
void launch_markdup_list(hipStream_t s, const uint32_t *at, const unsigned long long *total, const uint32_t *idx, const uint32_t *ci, uint64_t n, uint32_t *dup_list);
void launch_markdup_umi_keys(hipStream_t s, const MarkdupCollection &C, const uint32_t *ci, uint64_t n_anchors, uint64_t *k_umi, unsigned long long *counters);
void launch_markdup_heads_umi(hipStream_t s, const uint64_t *key, const uint32_t *idx, const uint64_t *k_lo, const uint64_t *k_umi, uint64_t n, uint32_t *mark, unsigned long long *counters);
void launch_markdup_heads_pos(hipStream_t s, const uint64_t *key, const uint32_t *idx, const uint64_t *k_lo, uint64_t n, uint32_t *mark_pos);
void launch_markdup_group_nodes(hipStream_t s, const uint32_t *at, const uint32_t *at_pos, const unsigned long long *tot, const uint32_t *idx, const uint64_t *k_lo, const uint64_t *k_umi, uint64_t n,
                                uint64_t *node_key, uint32_t *node_head, uint64_t *node_best, uint32_t *node_set, uint32_t *set_first, unsigned long long *group_best);
void launch_markdup_group_parents(hipStream_t s, const uint64_t *node_key, const uint32_t *node_head, const uint32_t *node_set, const uint32_t *set_first, uint32_t n_nodes, uint32_t n_sets,
                                  uint32_t *parent, unsigned long long *counters);
void launch_markdup_group_roots(hipStream_t s, const uint32_t *parent, const uint32_t *node_set, const uint32_t *set_first, const uint64_t *node_best, uint32_t n_nodes, uint32_t n_sets, uint32_t *root,
                                unsigned long long *group_best);
void launch_markdup_group_marks(hipStream_t s, const uint32_t *at, const unsigned long long *tot, const uint32_t *idx, const uint64_t *k_lo, const uint32_t *root, const unsigned long long *group_best,
                                uint64_t n, uint32_t n_nodes, uint32_t *mark);
void launch_markdup_insert(hipStream_t s, const MarkdupCollection &C, const uint32_t *dup_list, uint64_t n_dup, uint32_t *table, uint32_t mask);
void launch_markdup_apply(hipStream_t s, const MarkdupCollection &C, const uint32_t *dup_list, uint64_t n_dup, const uint32_t *table, uint32_t mask, uint8_t *verdict, unsigned long long *counters);
#endif

}  // namespace rsqc
