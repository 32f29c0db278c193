// rsqc_genebody.h -- the stage of --gene-body (rsqc_genebody_begin / rsqc_genebody_end / rsqc_genebody_sums): the depth of the pass's
// coverage track (rsqc_track.h) summed along every gene's body, 5' to 3', into RSQC_GENEBODY_BINS bins per gene.  Written like
// rsqc_track.h against the HIP wave intrinsics only (__shfl, LDS, atomics): the same source runs under the 64-lane emulation of
// tests/hostemu/wavemu.h (tests/hostemu/genebody_emu.cpp) against a plain restatement of the contract (tests/genebody_ref.py).
// No rocPRIM.
//
// The contract, in integers:
//   model        a gene is a list of segments (tid, start, end), 0-based, end exclusive; all segments of one gene lie on ONE contig of
//                the track and inside [0, length[tid]); they are non-empty, ascending and disjoint (abutting is allowed); one `reverse`
//                byte per gene; a gene may have no segment.  L is the sum of the segment lengths
//   coordinate   u of a model position p: the model bases in front of it in genomic order; t = u (forward) or L - 1 - u (reverse);
//                bin(p) = floor(t * 100 / L), the product in 64 bits
//   sums         sum[g][k]: the total of depth(p) over the positions of gene g with bin(p) = k, uint64_t and exact; depth is the
//                track's.  Genes with L < 100 are not measured (100 zeroes); genes that share positions each see the full depth
//   info         n_genes; n_measured (L >= 100); model_bases (the sum of L over the measured genes); depth_sum (the sum of all bins)
// The sums do not depend on the order of the records, on the batches, or on RSQC_TRACK_MERGE.
//
// The plan (host, genebody_plan below): every measured gene's [0, L) is cut into items of at most RSQC_GENEBODY_ITEM model bases, so
// the work is balanced by bases, not by genes (10^2 .. 10^6 bases a gene).  An item knows the segment that holds its first base.
//
//   genebody_bins_kernel   one wave per item.  Rounds of 64 consecutive u: a lane walks from the wave-uniform segment cursor (index,
//                          first u, start and length in registers) to the segment of its u -- no step and no load for a lane inside
//                          the cursor's segment; the cursor of the next round is lane 63's -- reads the depth of its position from the
//                          scanned difference array (slot i's depth is at i + 1) -- consecutive lanes read consecutive words inside a
//                          segment -- and adds it to a private (bin, sum) pair; when its bin changes the pair goes to the wave's 100
//                          LDS bins with one 64-bit LDS atomicAdd.  At the item's end the non-zero bins are added to the gene's row
//                          with one non-returning 64-bit atomicAdd each (lanes k and k + 64 own bins k and k + 64: 512 contiguous
//                          bytes a wave instruction); the items of one gene meet there.  The item's total goes to depth_sum
#pragma once

#if !defined(RSQC_WAVE_EMU)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/rnaseqc_amd.h"

#define RSQC_GENEBODY_THREADS 256
#define RSQC_GENEBODY_WAVES (RSQC_GENEBODY_THREADS / 64)     /* items of one workgroup */
#define RSQC_GENEBODY_ITEM 4096u                             /* most model bases of one item: 64 rounds of a wave */

namespace rsqc {

// one wave's work: u in [u0, u1) of `gene`; seg: the segment (index into the model's columns) that holds u0, seg_u: the u of that
// segment's first base; len_rev: L | reverse << 31
struct GenebodyItem { uint32_t gene, u0, u1, seg, seg_u, len_rev; };
// the model's columns (device pointers in the kernel)
struct GenebodyModel { const int32_t *seg_tid; const uint32_t *seg_start, *seg_end; };

struct GenebodyPlan {
    std::vector<GenebodyItem> items;
    uint32_t n_measured = 0;
    uint64_t model_bases = 0;
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

// The launch plan of a model that passed genebody_check: the items of every measured gene tile its [0, L) once, in gene order
inline void genebody_plan(int32_t n_genes, const uint32_t *seg_off, const uint32_t *seg_start, const uint32_t *seg_end, const uint8_t *reverse, uint32_t item, GenebodyPlan &P) {
    P = GenebodyPlan{};
    for (int32_t g = 0; g < n_genes; ++g) {
        uint64_t L = 0;
        for (uint32_t k = seg_off[g]; k < seg_off[g + 1]; ++k) L += seg_end[k] - seg_start[k];      // (one contig: at most 2^31 - 1)
        if (L < RSQC_GENEBODY_BINS) continue;
        ++P.n_measured; P.model_bases += L;
        uint32_t seg = seg_off[g], seg_u = 0;
        for (uint64_t u0 = 0; u0 < L; u0 += item) {
            while ((uint64_t)seg_u + (seg_end[seg] - seg_start[seg]) <= u0) { seg_u += seg_end[seg] - seg_start[seg]; ++seg; }
            const uint64_t u1 = u0 + item < L ? u0 + item : L;
            P.items.push_back(GenebodyItem{(uint32_t)g, (uint32_t)u0, (uint32_t)u1, seg, seg_u, (uint32_t)L | (reverse[g] ? 0x80000000u : 0u)});
        }
    }
}

#if defined(RSQC_GENEBODY_KERNELS) || defined(RSQC_WAVE_EMU)      /* the kernel: rsqc_genebody.hip and the emulation only */
// S: the exclusive prefix sum of the track's difference array (the depth of slot i at i + 1); off: the contigs' first slots;
// sums: [n_genes][RSQC_GENEBODY_BINS]; total: depth_sum
__global__ __launch_bounds__(RSQC_GENEBODY_THREADS) void genebody_bins_kernel(const uint32_t *S, const uint64_t *off, GenebodyModel M, const GenebodyItem *items, uint64_t n_items,
                                                                              unsigned long long *sums, unsigned long long *total) {
    __shared__ unsigned long long s_bin[RSQC_GENEBODY_WAVES][128];      // (100 bins a wave; 128: lanes k and k + 64 own two without a test)
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t it = (uint64_t)blockIdx.x * RSQC_GENEBODY_WAVES + wv;
    s_bin[wv][lane] = 0ull; s_bin[wv][lane + 64u] = 0ull;
    __syncthreads();
    GenebodyItem I{0u, 0u, 0u, 0u, 0u, 1u};                            // (a wave behind the last item: no round)
    if (it < n_items) I = items[it];
    const uint32_t L = I.len_rev & 0x7FFFFFFFu;
    const bool rev = (I.len_rev >> 31) != 0u;
    const uint64_t base = I.u0 < I.u1 ? off[M.seg_tid[I.seg]] : 0ull;   // (every segment of a gene lies on one contig)
    // wave-uniform, in registers: the segment of the round's first u -- a lane inside it needs no load to know its position
    uint32_t seg = I.seg, seg_u = I.seg_u, seg_start = 0u, seg_len = 0u;
    if (I.u0 < I.u1) { seg_start = M.seg_start[seg]; seg_len = M.seg_end[seg] - seg_start; }
    uint32_t bin = 0u; unsigned long long acc = 0ull;                  // this lane's open pair
    for (uint32_t ur = I.u0; ur < I.u1; ur += 64u) {
        const bool live = ur + lane < I.u1;
        const uint32_t u = live ? ur + lane : I.u1 - 1u;               // (a lane behind the item's end walks to its last base and adds nothing)
        uint32_t s = seg, su = seg_u, start = seg_start, len = seg_len;
        while (u - su >= len) { su += len; ++s; start = M.seg_start[s]; len = M.seg_end[s] - start; }
        if (live) {
            const uint32_t d = S[base + start + (u - su) + 1ull];
            const uint32_t t = rev ? L - 1u - u : u;
            const uint32_t b = (uint32_t)(((unsigned long long)t * RSQC_GENEBODY_BINS) / L);     // (an exact float-estimated quotient instead measured the same: DESIGN 6b)
            if (b != bin) { if (acc) atomicAdd(&s_bin[wv][bin], acc); acc = 0ull; bin = b; }
            acc += d;
        }
        seg = __shfl(s, 63, 64); seg_u = __shfl(su, 63, 64); seg_start = __shfl(start, 63, 64); seg_len = __shfl(len, 63, 64);
    }
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
void launch_genebody_bins(hipStream_t s, const uint32_t *S, const uint64_t *off, const GenebodyModel &M, const GenebodyItem *items, uint64_t n_items, unsigned long long *sums, unsigned long long *total);
#endif

}  // namespace rsqc
