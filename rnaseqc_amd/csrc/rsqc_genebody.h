// rsqc_genebody.h -- the stage of --gene-body (rsqc_genebody_begin / rsqc_genebody_end / rsqc_genebody_sums): the depth of the pass's
// coverage track (rsqc_track.h) summed along every gene's body, 5' to 3', into RSQC_GENEBODY_BINS bins per gene.  Written like
// rsqc_track.h against the HIP wave intrinsics only (__shfl, LDS, atomics): the same source runs under the 64-lane emulation of
// tests/hostemu/wavemu.h (tests/hostemu/genebody_emu.cpp) against a plain restatement of the contract (tests/genebody_ref.py).
// No rocPRIM.
//
// The contract, in integers:
//   model        the model of rsqc_genemodel.h (segments on one contig, non-empty, ascending, disjoint; L the sum of their lengths)
//                with one `reverse` byte per gene
//   coordinate   u of a model position p as in rsqc_genemodel.h; t = u (forward) or L - 1 - u (reverse);
//                bin(p) = floor(t * 100 / L), the product in 64 bits
//   sums         sum[g][k]: the total of depth(p) over the positions of gene g with bin(p) = k, uint64_t and exact; depth is the
//                track's.  Genes with L < 100 are not measured (100 zeroes); genes that share positions each see the full depth
//   info         n_genes; n_measured (L >= 100); model_bases (the sum of L over the measured genes); depth_sum (the sum of all bins)
// The sums do not depend on the order of the records, on the batches, or on RSQC_TRACK_MERGE.
//
// The plan (host, genebody_plan below): gene_tile of rsqc_genemodel.h over the genes with L >= 100, items of at most RSQC_GENEBODY_ITEM
// model bases; an item carries L and the strand.
//
//   genebody_bins_kernel   one wave per item, the walk of rsqc_genemodel.h (gene_walk).  A lane adds the depth of its position to a
//                          private (bin, sum) pair; when its bin changes the pair goes to the wave's 100 LDS bins with one 64-bit LDS
//                          atomicAdd.  At the item's end the non-zero bins are added to the gene's row with one non-returning 64-bit
//                          atomicAdd each (lanes k and k + 64 own bins k and k + 64: 512 contiguous bytes a wave instruction); the
//                          items of one gene meet there.  The item's total goes to depth_sum
#pragma once

#include "../../include/rnaseqc_amd.h"
#include "rsqc_genemodel.h"

#define RSQC_GENEBODY_THREADS 256
#define RSQC_GENEBODY_WAVES (RSQC_GENEBODY_THREADS / 64)     /* items of one workgroup */
#define RSQC_GENEBODY_ITEM 4096u                             /* most model bases of one item: 64 rounds of a wave */

namespace rsqc {

// one wave's work: the item of rsqc_genemodel.h and len_rev: L | reverse << 31
struct GenebodyItem : GeneItem { uint32_t len_rev; };
static_assert(sizeof(GenebodyItem) == 24, "an item is six words: gene, u0, u1, seg, seg_u, len_rev");
using GenebodyPlan = GeneTiling<GenebodyItem>;
using GenebodyModel = GeneModel;                             // (the name a caller written before rsqc_genemodel.h knows it by)

// The launch plan of a model that passed genebody_check: the items of every measured gene tile its [0, L) once, in gene order
inline void genebody_plan(int32_t n_genes, const uint32_t *seg_off, const uint32_t *seg_start, const uint32_t *seg_end, const uint8_t *reverse, uint32_t item, GenebodyPlan &P) {
    gene_tile(n_genes, seg_off, seg_start, seg_end, RSQC_GENEBODY_BINS, item, P,
              [&](const GeneItem &I, uint64_t L) { return GenebodyItem{I, (uint32_t)L | (reverse[I.gene] ? 0x80000000u : 0u)}; });
}

#if defined(RSQC_GENEBODY_KERNELS) || defined(RSQC_WAVE_EMU)      /* the kernel: rsqc_genebody.hip and the emulation only */
// S: the exclusive prefix sum of the track's difference array (the depth of slot i at i + 1); off: the contigs' first slots;
// sums: [n_genes][RSQC_GENEBODY_BINS]; total: depth_sum
__global__ __launch_bounds__(RSQC_GENEBODY_THREADS) void genebody_bins_kernel(const uint32_t *S, const uint64_t *off, GeneModel M, const GenebodyItem *items, uint64_t n_items,
                                                                              unsigned long long *sums, unsigned long long *total) {
    __shared__ unsigned long long s_bin[RSQC_GENEBODY_WAVES][128];      // (100 bins a wave; 128: lanes k and k + 64 own two without a test)
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t it = (uint64_t)blockIdx.x * RSQC_GENEBODY_WAVES + wv;
    s_bin[wv][lane] = 0ull; s_bin[wv][lane + 64u] = 0ull;
    __syncthreads();
    GenebodyItem I{{0u, 0u, 0u, 0u, 0u}, 1u};                          // (a wave behind the last item: an empty item, no round)
    if (it < n_items) I = items[it];
    const uint32_t L = I.len_rev & 0x7FFFFFFFu;
    const bool rev = (I.len_rev >> 31) != 0u;
    uint32_t bin = 0u; unsigned long long acc = 0ull;                  // this lane's open pair
    gene_walk(S, off, M, I, lane, [&](uint32_t u, uint32_t d) {
        const uint32_t t = rev ? L - 1u - u : u;
        const uint32_t b = (uint32_t)(((unsigned long long)t * RSQC_GENEBODY_BINS) / L);     // (an exact float-estimated quotient instead measured the same: DESIGN 6b)
        if (b != bin) { if (acc) atomicAdd(&s_bin[wv][bin], acc); acc = 0ull; bin = b; }
        acc += d;
    });
    if (acc) atomicAdd(&s_bin[wv][bin], acc);
    __syncthreads();
    const unsigned long long v0 = s_bin[wv][lane], v1 = s_bin[wv][lane + 64u];      // (no bin >= 100 is ever added to: v1 is 0 there)
    unsigned long long *row = sums + (uint64_t)I.gene * RSQC_GENEBODY_BINS;
    if (v0) atomicAdd(&row[lane], v0);
    if (v1) atomicAdd(&row[lane + 64u], v1);
    unsigned long long tot = v0 + v1;
    for (int o = 32; o >= 1; o >>= 1) tot += __shfl_xor(tot, o, 64);
    if (lane == 0u && tot) atomicAdd(total, tot);
}
#endif

#if !defined(RSQC_WAVE_EMU)
// launcher (rsqc_genebody.hip)
void launch_genebody_bins(hipStream_t s, const uint32_t *S, const uint64_t *off, const GeneModel &M, const GenebodyItem *items, uint64_t n_items, unsigned long long *sums, unsigned long long *total);
#endif

}  // namespace rsqc
