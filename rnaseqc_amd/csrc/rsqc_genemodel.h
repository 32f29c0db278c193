// rsqc_genemodel.h -- what the stages over the pass's coverage track (rsqc_track.h) that follow a gene model share: --gene-body
// (rsqc_genebody.h) and --tin (rsqc_tin.h).  The model and its rules, the tiling of the genes into one wave's work each, and the walk
// of a wave along its item.  Written like the two headers it serves against the HIP wave intrinsics only (__shfl): the same source
// runs under the 64-lane emulation of tests/hostemu/wavemu.h.  The device code sits behind the units' *_KERNELS defines.
//
//   model        a gene is a list of segments (tid, start, end), 0-based, end exclusive; all segments of one gene lie on ONE contig of
//                the track and inside [0, length[tid]); they are non-empty, ascending and disjoint (abutting is allowed); a gene may
//                have no segment.  L is the sum of the segment lengths
//   coordinate   u of a model position p: the model bases in front of it in genomic order
#pragma once

#if !defined(RSQC_WAVE_EMU)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include <string>
#include <vector>

namespace rsqc {

// the model's columns (device pointers in the kernels)
struct GeneModel { const int32_t *seg_tid; const uint32_t *seg_start, *seg_end; };
// one wave's work: u in [u0, u1) of `gene`; seg: the segment (index into the model's columns) that holds u0, seg_u: the u of that
// segment's first base
struct GeneItem { uint32_t gene, u0, u1, seg, seg_u; };
static_assert(sizeof(GeneItem) == 20, "an item is five words: gene, u0, u1, seg, seg_u");

// the items of a model, in gene order and, inside a gene, in u order.  Item: GeneItem, or a type that starts with one
template <class Item> struct GeneTiling {
    std::vector<Item> items;
    uint32_t n_measured = 0;                                 // genes with L >= min_len
    uint64_t model_bases = 0;                                // the sum of their L
};

// The model rules, gene by gene; the first violation as text ("" when there is none).  length: the track's contigs
inline std::string genebody_check(int32_t n_genes, const uint32_t *seg_off, const int32_t *seg_tid, const uint32_t *seg_start, const uint32_t *seg_end,
                                    int32_t n_contigs, const uint32_t *length) {
    if (n_genes && seg_off[0] != 0u) return "seg_off[0] is " + std::to_string(seg_off[0]) + " (it must be 0)";
    for (int32_t g = 0; g < n_genes; ++g) {
        if (seg_off[g + 1] < seg_off[g]) return "gene " + std::to_string(g) + ": seg_off is not ascending";
        for (uint32_t k = seg_off[g]; k < seg_off[g + 1]; ++k) {
            const bool foreign = seg_tid[k] < 0 || seg_tid[k] >= n_contigs, other = !foreign && seg_tid[k] != seg_tid[seg_off[g]];
            const bool empty = seg_start[k] >= seg_end[k], beyond = !foreign && seg_end[k] > length[seg_tid[k]];
            const bool order = k > seg_off[g] && seg_start[k] < seg_end[k - 1];
            if (!(foreign || other || empty || beyond || order)) continue;
            // (the texts are made for a segment that breaks a rule only: a GENCODE-sized model has 350 k segments)
            const std::string who = "gene " + std::to_string(g) + ", segment " + std::to_string(k - seg_off[g]) + ": ";
            const std::string iv = "[" + std::to_string(seg_start[k]) + ", " + std::to_string(seg_end[k]) + ")";
            if (foreign) return who + "contig " + std::to_string(seg_tid[k]) + " is not one of the track's " + std::to_string(n_contigs);
            if (other) return who + "contig " + std::to_string(seg_tid[k]) + " is another contig than the gene's first segment's (" + std::to_string(seg_tid[seg_off[g]]) + ")";
            if (empty) return who + iv + " is empty";
            if (beyond) return who + iv + " ends beyond the contig's " + std::to_string(length[seg_tid[k]]) + " positions";
            return who + iv + " is not ascending and disjoint (the segment in front of it ends at " + std::to_string(seg_end[k - 1]) + ")";
        }
    }
    return std::string();
}

// The tiling of a model that passed genebody_check: the items, of at most `item` bases, of every gene with L >= min_len tile its
// [0, L) once -- the work is balanced by bases, not by genes (10^2 .. 10^6 bases a gene).  make(GeneItem, L): the stage's item
template <class Item, class Make>
inline void gene_tile(int32_t n_genes, const uint32_t *seg_off, const uint32_t *seg_start, const uint32_t *seg_end, uint64_t min_len, uint32_t item, GeneTiling<Item> &P, Make make) {
    P.items.clear(); P.n_measured = 0; P.model_bases = 0;
    for (int32_t g = 0; g < n_genes; ++g) {
        uint64_t L = 0;
        for (uint32_t k = seg_off[g]; k < seg_off[g + 1]; ++k) L += seg_end[k] - seg_start[k];      // (one contig: at most 2^31 - 1)
        if (L < min_len) continue;
        ++P.n_measured; P.model_bases += L;
        uint32_t seg = seg_off[g], seg_u = 0;
        for (uint64_t u0 = 0; u0 < L; u0 += item) {
            while ((uint64_t)seg_u + (seg_end[seg] - seg_start[seg]) <= u0) { seg_u += seg_end[seg] - seg_start[seg]; ++seg; }
            const uint64_t u1 = u0 + item < L ? u0 + item : L;
            P.items.push_back(make(GeneItem{(uint32_t)g, (uint32_t)u0, (uint32_t)u1, seg, seg_u}, L));
        }
    }
}

#if defined(RSQC_GENEBODY_KERNELS) || defined(RSQC_TIN_KERNELS) || defined(RSQC_WAVE_EMU)      /* the walk: the kernels' units and the emulation only */
// The walk of one wave along item I: f(u, d) with the depth d of the model position u, for every u in [u0, u1) -- on the lane that
// holds u, a lane's calls in round order.  S: the exclusive prefix sum of the track's difference array (slot i's depth is at i + 1);
// off: the contigs' first slots.  Rounds of 64 consecutive u: a lane walks from the wave-uniform segment cursor to the segment of its
// u -- no step and no load for a lane inside the cursor's segment; the cursor of the next round is lane 63's -- and consecutive lanes
// read consecutive words inside a segment.  An empty item (u0 >= u1) does no load and no round
template <class F>
__device__ __forceinline__ void gene_walk(const uint32_t *S, const uint64_t *off, const GeneModel &M, const GeneItem &I, uint32_t lane, F &&f) {
    if (I.u0 >= I.u1) return;
    const uint64_t base = off[M.seg_tid[I.seg]];                       // (every segment of a gene lies on one contig)
    // wave-uniform, in registers: the segment of the round's first u -- a lane inside it needs no load to know its position
    uint32_t seg = I.seg, seg_u = I.seg_u, seg_start = M.seg_start[seg], seg_len = M.seg_end[seg] - seg_start;
    for (uint32_t ur = I.u0; ur < I.u1; ur += 64u) {
        const bool live = ur + lane < I.u1;
        const uint32_t u = live ? ur + lane : I.u1 - 1u;               // (a lane behind the item's end walks to its last base and adds nothing)
        uint32_t s = seg, su = seg_u, start = seg_start, len = seg_len;
        while (u - su >= len) { su += len; ++s; start = M.seg_start[s]; len = M.seg_end[s] - start; }
        if (live) f(u, S[base + start + (u - su) + 1ull]);
        seg = __shfl(s, 63, 64); seg_u = __shfl(su, 63, 64); seg_start = __shfl(start, 63, 64); seg_len = __shfl(len, 63, 64);
    }
}
#endif

}  // namespace rsqc
