// rsqc_tin.h -- the stage of --tin (rsqc_tin_begin / rsqc_tin_end / rsqc_tin_rows): per gene, over the depth of the pass's coverage
// track (rsqc_track.h) along the gene's model positions, the four figures the transcript integrity number is made of.  Written like
// rsqc_genebody.h against the HIP wave intrinsics only (__shfl_xor): the same source runs under the 64-lane emulation of
// tests/hostemu/wavemu.h (tests/hostemu/tin_emu.cpp) against a plain restatement of the contract (tests/tin_ref.py).  No rocPRIM, no
// LDS, no atomics.
//
// The contract:
//   model        the model of rsqc_genemodel.h (segments on one contig, non-empty, ascending, disjoint; L the sum of their lengths);
//                no `reverse` byte: the figures are symmetric in the strand
//   row          rsqc_tin_row of gene g, over its model positions p with d = depth(p), the track's:
//                depth_sum = sum d, covered = #{d > 0}, max_depth = max d (all exact), dlog2d = sum over d >= 2 of d * log2(d) (a
//                double; depths 0 and 1 add exactly 0).  A gene with L = 0 has an all-zero row.  A gene is measured when L >= 1
//   the double   the order of its additions is fixed: a lane adds its positions in round order, the wave combines its lanes with one
//                butterfly (xor 32, 16, .., 1: both partners add the same two values, and a + b == b + a), every item writes its
//                partial to a slot of its own, and ONE lane adds a gene's slots in item order.  No floating atomic anywhere: two
//                passes over the same records give the same bits, whatever the record order, the batches or RSQC_TRACK_MERGE.
//                Against an exactly rounded sum the relative error is at most (items_g + 80) * 2^-52: up to 64 additions a lane, 6
//                butterfly steps, items_g additions a gene, a few ulp for log2 and the product
//   info         n_genes; n_measured (L >= 1); model_bases (the sum of L); depth_sum, covered_bases (the sums over the rows, added
//                on the host)
//
// The plan (host, tin_plan below): gene_tile of rsqc_genemodel.h over the genes with L >= 1, items of at most RSQC_TIN_ITEM model
// bases; item_off[g] .. item_off[g + 1] are gene g's items, contiguous and in u order.
//
//   tin_items_kernel   one wave per item, four items a workgroup, the walk of rsqc_genemodel.h (gene_walk).  A lane keeps its four
//                      figures in registers; log2 is taken where d >= 2 only.  At the item's end one butterfly over the four and
//                      lane 0 stores the 24-byte partial to slot `it`: every slot of a launched item is written (no memset), the
//                      all-zero ones included
//   tin_rows_kernel    one lane per gene: the gene's slots added in item order into its row (a gene of 300 k bases has 74 slots);
//                      genes without an item get a zero row.  The sequential loop IS the order
#pragma once

#include <math.h>

#include "../../include/rnaseqc_amd.h"
#include "rsqc_genemodel.h"

#define RSQC_TIN_THREADS 256
#define RSQC_TIN_WAVES (RSQC_TIN_THREADS / 64)               /* items of one workgroup */
#define RSQC_TIN_ITEM 4096u                                  /* most model bases of one item: 64 rounds of a wave */

namespace rsqc {

using TinItem = GeneItem;                                    // one wave's work
using TinModel = GeneModel;                                  // (the name a caller written before rsqc_genemodel.h knows it by)
struct TinPlan : GeneTiling<TinItem> {
    std::vector<uint64_t> item_off;                          // [n_genes + 1]: gene g's items are [item_off[g], item_off[g + 1])
};

// The launch plan of a model that passed genebody_check: the items of every measured gene tile its [0, L) once, in gene order
inline void tin_plan(int32_t n_genes, const uint32_t *seg_off, const uint32_t *seg_start, const uint32_t *seg_end, uint32_t item, TinPlan &P) {
    gene_tile(n_genes, seg_off, seg_start, seg_end, 1, item, P, [](const GeneItem &I, uint64_t) { return I; });
    P.item_off.assign((size_t)(n_genes > 0 ? n_genes : 0) + 1, 0ull);
    for (const TinItem &I : P.items) ++P.item_off[(size_t)I.gene + 1];                              // (a gene without an item: an empty range)
    for (size_t g = 1; g < P.item_off.size(); ++g) P.item_off[g] += P.item_off[g - 1];
}

#if defined(RSQC_TIN_KERNELS) || defined(RSQC_WAVE_EMU)          /* the kernels: rsqc_tin.hip and the emulation only */
// S: the exclusive prefix sum of the track's difference array (the depth of slot i at i + 1); off: the contigs' first slots;
// part: [n_items], one slot an item
__global__ __launch_bounds__(RSQC_TIN_THREADS) void tin_items_kernel(const uint32_t *S, const uint64_t *off, GeneModel M, const TinItem *items, uint64_t n_items, rsqc_tin_row *part) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t it = (uint64_t)blockIdx.x * RSQC_TIN_WAVES + wv;
    if (it >= n_items) return;                                         // (a wave behind the last item, as a whole)
    const TinItem I = items[it];                                       // (u0 < u1: the plan makes no empty item)
    unsigned long long sum = 0ull; uint32_t cov = 0u, mx = 0u; double e = 0.0;      // this lane's figures
    gene_walk(S, off, M, I, lane, [&](uint32_t, uint32_t d) {
        sum += d; cov += d ? 1u : 0u; mx = d > mx ? d : mx;
        if (d >= 2u) e += (double)d * log2((double)d);                 // (in round order: the lane's part of the fixed order)
    });
    for (int o = 32; o >= 1; o >>= 1) {                                // the butterfly: after it every lane holds the same four
        sum += __shfl_xor(sum, o, 64); cov += __shfl_xor(cov, o, 64);
        const uint32_t m = __shfl_xor(mx, o, 64); mx = m > mx ? m : mx;
        e += __shfl_xor(e, o, 64);
    }
    if (lane == 0u) { rsqc_tin_row r; r.depth_sum = sum; r.covered = cov; r.max_depth = mx; r.dlog2d = e; part[it] = r; }
}

// rows: [n_genes]; item_off: [n_genes + 1]
__global__ __launch_bounds__(RSQC_TIN_THREADS) void tin_rows_kernel(const rsqc_tin_row *part, const uint64_t *item_off, uint32_t n_genes, rsqc_tin_row *rows) {
    const uint64_t g = (uint64_t)blockIdx.x * RSQC_TIN_THREADS + threadIdx.x;
    if (g >= n_genes) return;
    rsqc_tin_row r; r.depth_sum = 0ull; r.covered = 0u; r.max_depth = 0u; r.dlog2d = 0.0;
    for (uint64_t k = item_off[g]; k < item_off[g + 1]; ++k) {        // in item order: the gene's part of the fixed order
        const rsqc_tin_row p = part[k];
        r.depth_sum += p.depth_sum; r.covered += p.covered; r.max_depth = p.max_depth > r.max_depth ? p.max_depth : r.max_depth; r.dlog2d += p.dlog2d;
    }
    rows[g] = r;
}
#endif

#if !defined(RSQC_WAVE_EMU)
// launchers (rsqc_tin.hip)
void launch_tin_items(hipStream_t s, const uint32_t *S, const uint64_t *off, const GeneModel &M, const TinItem *items, uint64_t n_items, rsqc_tin_row *part);
void launch_tin_rows(hipStream_t s, const rsqc_tin_row *part, const uint64_t *item_off, uint32_t n_genes, rsqc_tin_row *rows);
#endif

}  // namespace rsqc
