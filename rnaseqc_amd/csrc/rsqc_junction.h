// rsqc_junction.h -- the kernels of --junctions (rsqc_junctions_begin / rsqc_junctions_end): reads per splice junction.  Every `N`
// operation of a contributing record is one INSTANCE (tid, start, end) -- 1-based closed coordinates of the intron's first and last
// base, STAR's SJ.out.tab convention -- with the record's mapping-quality bit and the instance's overhang; the table has one row per
// distinct (tid, start, end), ascending, with the number of instances, of high-quality instances and the largest overhang.
// Written like rsqc_sort.h against the HIP wave intrinsics only (__ballot, __shfl*, LDS): the same source runs under the 64-lane
// emulation of tests/hostemu/wavemu.h (tests/hostemu/junction_emu.cpp) against a plain restatement of the contract.  No rocPRIM.
//
//   junction_extract_kernel   per batch, one lane per record: the population test, the record's segment, the walk over its CIGAR
//                             (twice: counting, then writing).  A workgroup reserves room for all its instances with ONE memory
//                             atomic on the collection's cursor; an instance that finds the collection full raises the error flag
//   junction_widen_kernel     `end` as a 64-bit key for the first stage of the order
//   junction_permute_kernel   key_hi in the order of the first stage, the key of the second
//   junction_heads_kernel     1 where a sorted instance differs from its predecessor in (key_hi, end)
//   junction_reduce_kernel    the rows: the lanes of a wave that share a row are contiguous (the instances are sorted), so a ballot
//                             of the heads cuts the wave into runs; a run's length and its high-quality count are popcounts, its
//                             largest overhang a segmented shuffle scan, and its last lane issues one atomicAdd each for reads and
//                             hq_reads and one atomicMax for max_overhang -- no lane loops over a run, however long
// The order itself is rsqc_sort.h's radix pass (launch_sort_pass), in two stages because the key has 96 bits and a pass takes 64:
// first over `end` with the instance index as payload, then over key_hi permuted by that index (LSD: the second stage is stable).
#pragma once

#if !defined(RSQC_WAVE_EMU)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "../../include/rnaseqc_amd.h"

#define RSQC_JUNC_THREADS 256
#define RSQC_JUNC_CAP0 65536ull                 /* instances the collection starts with (RSQC_JUNCTION_CAP0 overrides) */
#define RSQC_JUNC_MAX 0xFFFFFFF0ull             /* instances of one pass: fewer than this */
#define RSQC_JUNC_EXCLUDED (RSQC_FUNMAP | RSQC_FSECONDARY | RSQC_FQCFAIL | RSQC_FSUPP)

namespace rsqc {

// what the extraction reads of one batch (device pointers; the columns of DevBatch)
struct JunctionBatch {
    const rsqc_rec_core *core; const rsqc_rec_aux *aux; const uint32_t *cigar; uint64_t n, n_ops;
    const int32_t *seg_tid; const uint64_t *seg_start; uint32_t n_seg;
    const uint64_t *wide_index; const uint32_t *wide_n_cigar; uint32_t n_wide;
};
// the instances collected so far, in no particular order: key_hi = (tid << 32) | start, end, info = hq << 31 | min(overhang, 2^31 - 1)
struct JunctionCollection {
    uint64_t *key_hi; uint32_t *end, *info; uint64_t cap;
    unsigned long long *cursor;                 // [0] instances reserved so far (the true count: it moves on past cap), [1] contributing records
};
// the table's columns (device pointers), n rows: reads / hq_reads / max_overhang zeroed before junction_reduce_kernel
struct JunctionRows { int32_t *tid, *start, *end; uint32_t *reads, *hq_reads, *max_overhang; };

#if defined(RSQC_JUNCTION_KERNELS) || defined(RSQC_WAVE_EMU)      /* the kernels: rsqc_junction.hip and the emulation only */
// exclusive prefix sum over the 256 lanes of a workgroup (every lane calls); total = the sum over all of them
__device__ inline uint32_t junc_block_scan(uint32_t v, uint32_t &total) {
    __shared__ uint32_t s_wave[RSQC_JUNC_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t x = v;
    for (uint32_t o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(x, o, 64); if (lane >= o) x += t; }
    if (lane == 63) s_wave[w] = x;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (uint32_t k = 0; k < RSQC_JUNC_THREADS / 64; ++k) { const uint32_t s = s_wave[k]; if (k < w) base += s; tot += s; }
    __syncthreads();                                   // (the next call writes s_wave again)
    total = tot;
    return base + x - v;
}
__device__ inline int junc_top_bit(unsigned long long x) {           // index of the highest set bit, x != 0
#if defined(RSQC_WAVE_EMU)
    return 63 - __builtin_clzll(x);
#else
    return 63 - __clzll((long long)x);
#endif
}

// The walk over one record's operations.  WRITE = false: the number of instances; WRITE = true: they are written to slots
// [slot, slot + that number).  An instance's right overhang is known at the next `N` or at the record's end: it is held until then.
// Every `N`, of length 0 or dropped for its end included, closes the aligned block in front of it.
template <bool WRITE>
__device__ inline uint32_t junc_walk(const uint32_t *ops, uint32_t n_ops, int32_t pos, uint64_t tid_hi, uint32_t hq_bit, const JunctionCollection &C, uint64_t slot) {
    long long p = pos;
    unsigned long long cur = 0, left = 0;              // M = X bases since the previous N; those in front of the held instance
    uint32_t count = 0; bool held = false; uint64_t held_at = 0;
    for (uint32_t k = 0; k < n_ops; ++k) {
        const uint32_t op = ops[k], len = op >> 4, code = op & 15u;
        if (code == 3u) {                              // N
            if (WRITE && held) { const unsigned long long ov = left < cur ? left : cur; C.info[held_at] = hq_bit | (uint32_t)(ov < 0x7FFFFFFFull ? ov : 0x7FFFFFFFull); held = false; }
            if (len >= 1u && p + (long long)len <= 0x7FFFFFFFll) {
                if (WRITE) { C.key_hi[slot + count] = tid_hi | (uint64_t)(uint32_t)(p + 1); C.end[slot + count] = (uint32_t)(p + (long long)len); held = true; held_at = slot + count; left = cur; }
                ++count;
            }
            cur = 0; p += len;
        } else if (code == 0u || code == 7u || code == 8u) { cur += len; p += len; }      // M = X
        else if (code == 2u) p += len;                                                   // D
    }
    if (WRITE && held) { const unsigned long long ov = left < cur ? left : cur; C.info[held_at] = hq_bit | (uint32_t)(ov < 0x7FFFFFFFull ? ov : 0x7FFFFFFFull); }
    return count;
}

__global__ __launch_bounds__(RSQC_JUNC_THREADS) void junction_extract_kernel(JunctionBatch B, int32_t n_contigs, uint32_t mapq_threshold, JunctionCollection C, int *error) {
    __shared__ unsigned long long s_base;
    const uint64_t i = (uint64_t)blockIdx.x * RSQC_JUNC_THREADS + threadIdx.x;
    const uint32_t *ops = B.cigar; uint32_t n_ops = 0, count = 0, member = 0, hq_bit = 0; int32_t pos = 0; uint64_t tid_hi = 0;
    if (i < B.n && B.n_seg) {
        const rsqc_rec_aux a = B.aux[i];
        // the segment of record i: the last one that starts at or before it (empty segments share a start: the last of them holds the record)
        uint32_t lo = 0, hi = B.n_seg;
        while (hi - lo > 1) { const uint32_t m = (lo + hi) >> 1; if (B.seg_start[m] <= i) lo = m; else hi = m; }
        const int32_t tid = B.seg_tid[lo];
        if ((a.flag & RSQC_JUNC_EXCLUDED) == 0 && tid >= 0 && tid < n_contigs) {
            member = 1u;
            const rsqc_rec_core c = B.core[i];
            n_ops = a.n_cigar;
            if (a.n_cigar == RSQC_NCIGAR_ESCAPE) {     // the true count is in the wide table (an escape value without an entry: no operations)
                uint32_t wl = 0, wh = B.n_wide;
                while (wl < wh) { const uint32_t m = (wl + wh) >> 1; if (B.wide_index[m] < i) wl = m + 1; else wh = m; }
                n_ops = (wl < B.n_wide && B.wide_index[wl] == i) ? B.wide_n_cigar[wl] : 0u;
            }
            // (no record reads past the batch's pool, whatever it claims)
            if ((uint64_t)c.cigar_off >= B.n_ops) n_ops = 0u; else if ((uint64_t)n_ops > B.n_ops - c.cigar_off) n_ops = (uint32_t)(B.n_ops - c.cigar_off);
            ops = B.cigar + c.cigar_off; pos = c.pos; tid_hi = (uint64_t)(uint32_t)tid << 32;
            hq_bit = (uint32_t)a.mapq >= mapq_threshold ? 0x80000000u : 0u;
            count = junc_walk<false>(ops, n_ops, pos, tid_hi, hq_bit, C, 0);
        }
    }
    uint32_t total = 0, members = 0;
    const uint32_t first = junc_block_scan(count, total);
    (void)junc_block_scan(member, members);
    if (threadIdx.x == 0) {
        s_base = total ? atomicAdd(&C.cursor[0], (unsigned long long)total) : 0ull;      // the workgroup's ONE reservation
        if (members) atomicAdd(&C.cursor[1], (unsigned long long)members);
    }
    __syncthreads();
    const uint64_t base = s_base;
    if (base + total > C.cap) {                        // the collection is full: nothing of this workgroup is written, the pass ends with RSQC_ERR_CAPACITY
        if (threadIdx.x == 0) atomicExch(error, RSQC_ERR_CAPACITY);
        return;
    }
    if (count) (void)junc_walk<true>(ops, n_ops, pos, tid_hi, hq_bit, C, base + first);
}

__global__ __launch_bounds__(RSQC_JUNC_THREADS) void junction_widen_kernel(const uint32_t *end, uint64_t n, uint64_t *key) {
    const uint64_t i = (uint64_t)blockIdx.x * RSQC_JUNC_THREADS + threadIdx.x;
    if (i < n) key[i] = end[i];
}
__global__ __launch_bounds__(RSQC_JUNC_THREADS) void junction_permute_kernel(const uint64_t *key_hi, const uint32_t *idx, uint64_t n, uint64_t *key) {
    const uint64_t r = (uint64_t)blockIdx.x * RSQC_JUNC_THREADS + threadIdx.x;
    if (r < n) key[r] = key_hi[idx[r]];
}
// key: key_hi in sorted order; idx[r]: the collection index of rank r
__global__ __launch_bounds__(RSQC_JUNC_THREADS) void junction_heads_kernel(const uint64_t *key, const uint32_t *idx, const uint32_t *end, uint64_t n, uint32_t *mark) {
    const uint64_t r = (uint64_t)blockIdx.x * RSQC_JUNC_THREADS + threadIdx.x;
    if (r < n) mark[r] = (r == 0 || key[r] != key[r - 1] || end[idx[r]] != end[idx[r - 1]]) ? 1u : 0u;
}
// row_at: the exclusive prefix sum of the head marks (launch_sort_scan), total[0] their sum: the row of rank r is (the prefix
// sum INCLUDING r) - 1, and r is a head when the two differ
__global__ __launch_bounds__(RSQC_JUNC_THREADS) void junction_reduce_kernel(const uint64_t *key, const uint32_t *idx, const uint32_t *end, const uint32_t *info, uint64_t n,
                                                                             const uint32_t *row_at, const unsigned long long *total, JunctionRows R) {
    const uint64_t r = (uint64_t)blockIdx.x * RSQC_JUNC_THREADS + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const bool valid = r < n;
    uint32_t before = 0, through = 0, e = 0, inf = 0; uint64_t k = 0;
    if (valid) {
        before = row_at[r]; through = r + 1 < n ? row_at[r + 1] : (uint32_t)total[0];
        const uint32_t j = idx[r];
        k = key[r]; e = end[j]; inf = info[j];
    }
    const bool head = valid && through != before;
    const unsigned long long vmask = __ballot(valid);
    if (vmask == 0ull) return;                         // (the whole wave: valid ranks are the low lanes)
    const unsigned long long hmask = (__ballot(head) | 1ull) & vmask, hqmask = __ballot(valid && (inf >> 31));
    // the run of this lane inside the wave: from the last head at or below it to the lane in front of the next head (or the last valid lane)
    const unsigned long long upto = (2ull << lane) - 1ull;            // bits [0, lane]  (lane 63: 2 << 63 wraps to 0, minus 1 = all)
    const uint32_t run_lo = (uint32_t)junc_top_bit((hmask & upto) | 1ull);
    const unsigned long long above = hmask & ~upto;
    const uint32_t run_hi = above ? (uint32_t)__ffsll(above) - 2u : (uint32_t)junc_top_bit(vmask);
    uint32_t ov = inf & 0x7FFFFFFFu;
    for (uint32_t o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(ov, o, 64); if (lane >= o && lane - o >= run_lo && t > ov) ov = t; }
    if (valid && lane == run_hi) {                     // the run's last lane holds its maximum: one atomic each per run and wave
        const unsigned long long run = ((2ull << run_hi) - 1ull) & ~((1ull << run_lo) - 1ull);
        const uint32_t row = through - 1u;
        atomicAdd(&R.reads[row], run_hi - run_lo + 1u);
        atomicAdd(&R.hq_reads[row], (uint32_t)__popcll(hqmask & run));
        atomicMax(&R.max_overhang[row], ov);
    }
    if (head) { const uint32_t row = through - 1u; R.tid[row] = (int32_t)(uint32_t)(k >> 32); R.start[row] = (int32_t)(uint32_t)k; R.end[row] = (int32_t)e; }
}
#endif

#if !defined(RSQC_WAVE_EMU)
// launchers (rsqc_junction.hip)
void launch_junction_extract(hipStream_t s, const JunctionBatch &B, int32_t n_contigs, uint32_t mapq_threshold, const JunctionCollection &C, int *error);
void launch_junction_widen(hipStream_t s, const uint32_t *end, uint64_t n, uint64_t *key);
void launch_junction_permute(hipStream_t s, const uint64_t *key_hi, const uint32_t *idx, uint64_t n, uint64_t *key);
void launch_junction_heads(hipStream_t s, const uint64_t *key, const uint32_t *idx, const uint32_t *end, uint64_t n, uint32_t *mark);
void launch_junction_reduce(hipStream_t s, const uint64_t *key, const uint32_t *idx, const uint32_t *end, const uint32_t *info, uint64_t n,
                            const uint32_t *row_at, const unsigned long long *total, const JunctionRows &R);
#endif

}  // namespace rsqc
