// rsqc_k3_plan.h -- the launch plan of K3, the end-of-file coverage stage (rsqc_k3.h): which genes go to which instance of
// gene_coverage_kernel.  Host arithmetic only, plain C++ and no HIP types: the library (rsqc_api.cpp counts the classes,
// rsqc_kernels.hip launches the plan) and the host emulation of the tests (tests/hostemu/k3_emu.cpp) share it, so the plan that
// runs on the GPU is the plan the CPU tests check.
#pragma once

#include <stdint.h>

// coding-length classes of the end-of-file coverage stage: one wave / 256 threads with the vector in LDS, 1024 threads in memory
#ifndef RSQC_K3_SMALL_MAX
#define RSQC_K3_SMALL_MAX 4096
#endif
#define RSQC_K3_MEDIUM_MAX 12288
#define RSQC_K3_LARGE_LDS16 73000      /* bases a 1024-thread workgroup keeps in LDS as 16-bit depths (146 KB of the CU's 160 KB) */
#define RSQC_K3_LARGE2_LDS16 32768     /* ... the shorter genes of that class: 64 KB */
#ifndef RSQC_K3_SMALL_SPLIT
#define RSQC_K3_SMALL_SPLIT 1
#endif
#define RSQC_K3_LAUNCHES 8

namespace rsqc {

// genes per class, counted from the coding lengths (the thresholds are those of the instances below)
struct K3Counts {
    uint32_t n_large, n_medium, n_xlarge;                 // > 12 288 bases; 4 097 .. 12 288; > 32 768 (a part of n_large)
    uint32_t n_le6144, n_le3072, n_le2048, n_le1024;      // genes of up to 6 144 / 3 072 / 2 048 / 1 024 bases
};

// one launch: `count` workgroups of `threads` threads over gene_order[first, first + count); the gene's coverage vector stays in LDS
// as `cov_bits`-bit depths while it has at most `cap` bases (longer genes, and deeper ones at 16 bits, run the in-memory mode);
// `stream`: 0 .. 2, which of the stage's three side streams takes it
struct K3Launch {
    uint32_t threads, cov_bits, cap, count, first, stream;
};

// the eight instances in launch order.  The one-wave classes go behind the 256-thread ones (0.3 + 0.2 ms), NOT behind the 64 KB class:
// beside the fragment kernels that one takes 0.8 ms, and queued behind it the one-wave classes ended after the fragment count -- the
// stage's last kernel (timeline of call r6k)
constexpr uint32_t K3_THREADS[RSQC_K3_LAUNCHES] = {1024, 256, 256, 1024, 64, 64, 64, 64};
constexpr uint32_t K3_COV_BITS[RSQC_K3_LAUNCHES] = {16, 32, 32, 16, 32, 32, 32, 32};
constexpr uint32_t K3_CAPS[RSQC_K3_LAUNCHES] = {RSQC_K3_LARGE_LDS16, RSQC_K3_MEDIUM_MAX, 6144, RSQC_K3_LARGE2_LDS16, RSQC_K3_SMALL_MAX, 3072, 2048, 1024};
constexpr uint32_t K3_STREAM[RSQC_K3_LAUNCHES] = {0, 1, 1, 2, 1, 1, 1, 1};

// gene_coding[gene_order[k]], k < n: the listed genes' coding lengths (any order: only counts come out)
inline K3Counts k3_count_classes(const uint32_t *gene_coding, const uint32_t *gene_order, uint32_t n) {
    K3Counts c{};
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t len = gene_coding[gene_order[k]];
        if (len > (uint32_t)RSQC_K3_MEDIUM_MAX) c.n_large++; else if (len > (uint32_t)RSQC_K3_SMALL_MAX) c.n_medium++;
        if (len > (uint32_t)RSQC_K3_LARGE2_LDS16) c.n_xlarge++;
        if (len <= 6144u) c.n_le6144++;
        if (len <= 3072u) c.n_le3072++;
        if (len <= 2048u) c.n_le2048++;
        if (len <= 1024u) c.n_le1024++;
    }
    return c;
}

// gene_order is sorted by coding length, longest first: [0, n_large) x 1024 threads, [n_large, n_large + n_medium) x 256 threads, the
// rest one wave each; the launches are independent (disjoint genes).  The entries come in launch order.
// The 1024-thread class in two LDS sizes: a workgroup that holds 146 KB keeps its CU to itself, one that holds 64 KB leaves
// room for the fragment workgroups running beside it.  (The runtime maps streams onto four hardware queues: with K4 on the
// context's stream there are three for K3; the 64 KB class goes in front of the one-wave classes.)
// The other classes in several LDS sizes too (round 6): a workgroup's LDS is its gene's coverage vector, and sized for the LONGEST gene of
// a class it limits the workgroups a CU holds -- 8 one-wave workgroups (16 KB each: a quarter of the CU's wave slots) for the 53 k genes
// of up to 4 096 bases, of which 38 k have at most 1 024 -- and takes the LDS the fragment kernels beside them need.  gene_order is sorted
// by coding length, longest first, so a class is a range of it; the counts of genes of up to 6 144 / 3 072 / 2 048 / 1 024 bases come
// from the host (end-of-file kernels 1.57 -> 1.46 ms with the one-wave class in three sizes, call r6j).
inline void k3_plan(uint32_t n, uint32_t n_large, uint32_t n_medium, uint32_t n_xlarge, uint32_t n_le6144, uint32_t n_le3072,
                    uint32_t n_le2048, uint32_t n_le1024, K3Launch (&out)[RSQC_K3_LAUNCHES]) {
    static_assert(RSQC_K3_SMALL_MAX == 4096 && RSQC_K3_MEDIUM_MAX == 12288, "the split points below sit inside these classes");
    const uint32_t n_small = n - n_large - n_medium;
    if (!RSQC_K3_SMALL_SPLIT || n_le3072 > n_small || n_le6144 < n_small || n_le6144 > n_small + n_medium) { n_le6144 = n_small; n_le3072 = 0; n_le2048 = 0; n_le1024 = 0; }
    if (n_le2048 > n_le3072) n_le2048 = n_le3072;
    if (n_le1024 > n_le2048) n_le1024 = n_le2048;
    const uint32_t n_med_short = n_le6144 - n_small;                       // genes of 4 097 .. 6 144 bases: the end of the medium class
    const uint32_t count[RSQC_K3_LAUNCHES] = {n_xlarge, n_medium - n_med_short, n_med_short, n_large - n_xlarge,
                                              n_small - n_le3072, n_le3072 - n_le2048, n_le2048 - n_le1024, n_le1024};
    const uint32_t first[RSQC_K3_LAUNCHES] = {0u, n_large, n_large + n_medium - n_med_short, n_xlarge,
                                              n_large + n_medium, n - n_le3072, n - n_le2048, n - n_le1024};
    for (int k = 0; k < RSQC_K3_LAUNCHES; ++k) out[k] = K3Launch{K3_THREADS[k], K3_COV_BITS[k], K3_CAPS[k], count[k], first[k], K3_STREAM[k]};
}

}  // namespace rsqc
