// rsqc_tin.h -- the stage of --tin (rsqc_tin_begin / rsqc_tin_end / rsqc_tin_rows): per gene, over the depth of the pass's coverage
// track (rsqc_track.h) along the gene's model positions, the four figures the transcript integrity number is made of.  Written like
// rsqc_genebody.h against the HIP wave intrinsics only (__shfl_xor): the same source runs under the 64-lane emulation of
// tests/hostemu/wavemu.h (tests/hostemu/tin_emu.cpp) against a plain restatement of the contract (tests/tin_ref.py).  No rocPRIM, no
// LDS, no atomics.
//
// The contract:
//   model        the model of rsqc_genebody.h without the `reverse` byte (the figures are symmetric in the strand): a gene is a list
//                of segments (tid, start, end), 0-based, end exclusive, on ONE contig of the track and inside it, non-empty, ascending
//                and disjoint (abutting is allowed); a gene may have no segment.  L is the sum of the segment lengths.  The rules are
//                checked with genebody_check
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
// The plan (host, tin_plan below): every measured gene's [0, L) is cut into items of at most RSQC_TIN_ITEM model bases; an item knows
// the segment that holds its first base; item_off[g] .. item_off[g + 1] are gene g's items, contiguous and in u order.
//
//   tin_items_kernel   one wave per item, four items a workgroup.  The walk of genebody_bins_kernel: rounds of 64 consecutive u, a
//                      lane walks from the wave-uniform segment cursor (index, first u, start and length in registers) to the
//                      segment of its u; the cursor of the next round is lane 63's; the depth of slot i of the scanned difference
//                      array is at i + 1.  A lane keeps its four figures in registers; log2 is taken where d >= 2 only.  At the
//                      item's end one butterfly over the four and lane 0 stores the 24-byte partial to slot `it`: every slot of a
//                      launched item is written (no memset), the all-zero ones included
//   tin_rows_kernel    one lane per gene: the gene's slots added in item order into its row (a gene of 300 k bases has 74 slots);
//                      genes without an item get a zero row.  The sequential loop IS the order
#pragma once

#if !defined(RSQC_WAVE_EMU)
#include <hip/hip_runtime.h>
#endif
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/rnaseqc_amd.h"

#define RSQC_TIN_THREADS 256
#define RSQC_TIN_WAVES (RSQC_TIN_THREADS / 64)               /* items of one workgroup */
#define RSQC_TIN_ITEM 4096u                                  /* most model bases of one item: 64 rounds of a wave */

namespace rsqc {

// one wave's work: u in [u0, u1) of `gene`; seg: the segment (index into the model's columns) that holds u0, seg_u: the u of that
// segment's first base
struct TinItem { uint32_t gene, u0, u1, seg, seg_u; };
// the model's columns (device pointers in the kernel)
struct TinModel { const int32_t *seg_tid; const uint32_t *seg_start, *seg_end; };

struct TinPlan {
    std::vector<TinItem> items;
    std::vector<uint64_t> item_off;                          // [n_genes + 1]: gene g's items are [item_off[g], item_off[g + 1])
    uint32_t n_measured = 0;
    uint64_t model_bases = 0;
};

// The launch plan of a model that passed genebody_check: the items of every measured gene tile its [0, L) once, in gene order
inline void tin_plan(int32_t n_genes, const uint32_t *seg_off, const uint32_t *seg_start, const uint32_t *seg_end, uint32_t item, TinPlan &P) {
    P = TinPlan{};
    P.item_off.assign((size_t)(n_genes > 0 ? n_genes : 0) + 1, 0ull);
    for (int32_t g = 0; g < n_genes; ++g) {
        uint64_t L = 0;
        for (uint32_t k = seg_off[g]; k < seg_off[g + 1]; ++k) L += seg_end[k] - seg_start[k];      // (one contig: at most 2^31 - 1)
        if (L) { ++P.n_measured; P.model_bases += L; }
        uint32_t seg = seg_off[g], seg_u = 0;
        for (uint64_t u0 = 0; u0 < L; u0 += item) {
            while ((uint64_t)seg_u + (seg_end[seg] - seg_start[seg]) <= u0) { seg_u += seg_end[seg] - seg_start[seg]; ++seg; }
            const uint64_t u1 = u0 + item < L ? u0 + item : L;
            P.items.push_back(TinItem{(uint32_t)g, (uint32_t)u0, (uint32_t)u1, seg, seg_u});
        }
        P.item_off[(size_t)g + 1] = P.items.size();
    }
}

#if defined(RSQC_TIN_KERNELS) || defined(RSQC_WAVE_EMU)          /* the kernels: rsqc_tin.hip and the emulation only */
// S: the exclusive prefix sum of the track's difference array (the depth of slot i at i + 1); off: the contigs' first slots;
// part: [n_items], one slot an item
__global__ __launch_bounds__(RSQC_TIN_THREADS) void tin_items_kernel(const uint32_t *S, const uint64_t *off, TinModel M, const TinItem *items, uint64_t n_items, rsqc_tin_row *part) {
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t it = (uint64_t)blockIdx.x * RSQC_TIN_WAVES + wv;
    if (it >= n_items) return;                                         // (a wave behind the last item, as a whole)
    const TinItem I = items[it];                                       // (u0 < u1: the plan makes no empty item)
    const uint64_t base = off[M.seg_tid[I.seg]];                       // (every segment of a gene lies on one contig)
    // wave-uniform, in registers: the segment of the round's first u -- a lane inside it needs no load to know its position
    uint32_t seg = I.seg, seg_u = I.seg_u, seg_start = M.seg_start[seg], seg_len = M.seg_end[seg] - seg_start;
    unsigned long long sum = 0ull; uint32_t cov = 0u, mx = 0u; double e = 0.0;      // this lane's figures
    for (uint32_t ur = I.u0; ur < I.u1; ur += 64u) {
        const bool live = ur + lane < I.u1;
        const uint32_t u = live ? ur + lane : I.u1 - 1u;               // (a lane behind the item's end walks to its last base and adds nothing)
        uint32_t s = seg, su = seg_u, start = seg_start, len = seg_len;
        while (u - su >= len) { su += len; ++s; start = M.seg_start[s]; len = M.seg_end[s] - start; }
        if (live) {
            const uint32_t d = S[base + start + (u - su) + 1ull];
            sum += d; cov += d ? 1u : 0u; mx = d > mx ? d : mx;
            if (d >= 2u) e += (double)d * log2((double)d);             // (in round order: the lane's part of the fixed order)
        }
        seg = __shfl(s, 63, 64); seg_u = __shfl(su, 63, 64); seg_start = __shfl(start, 63, 64); seg_len = __shfl(len, 63, 64);
    }
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
void launch_tin_items(hipStream_t s, const uint32_t *S, const uint64_t *off, const TinModel &M, const TinItem *items, uint64_t n_items, rsqc_tin_row *part);
void launch_tin_rows(hipStream_t s, const rsqc_tin_row *part, const uint64_t *item_off, uint32_t n_genes, rsqc_tin_row *rows);
#endif

}  // namespace rsqc
