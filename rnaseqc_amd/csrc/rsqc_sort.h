// rsqc_sort.h -- the kernels of --sort (rsqc_sort_begin / rsqc_sort_end): records that arrive in any order are collected on the
// device, ordered stably by (tid as unsigned, pos as signed) with an LSD radix sort over 8-bit digits, and gathered into ordinary
// batches for the per-read kernels.  Written against the HIP wave intrinsics only (__ballot, __shfl*, LDS atomics): the same source
// runs under the 64-lane emulation of tests/hostemu/wavemu.h (tests/hostemu/sort_emu.cpp) against std::stable_sort.  No rocPRIM.
//
// One radix pass = three steps, no cursor shared between workgroups:
//   sort_hist_kernel     a workgroup counts the digits of ITS tile in LDS and leaves hist[digit * n_tiles + tile]
//   sort_scan_*          exclusive prefix sum over that table in digit-major order: entry (d, t) becomes the first output slot of
//                        tile t's keys of digit d -- every smaller digit of every tile, and digit d of the tiles before t, come first
//   sort_scatter_kernel  a workgroup ranks the keys of its tile again and writes (key, index) to slot + rank.  The rank of a key among
//                        the keys of ITS digit: lanes of a wave find the lanes that hold the same digit with eight ballots (match
//                        mask), the rounds of a wave add up in a per-wave LDS counter, and the waves of the workgroup are laid one
//                        behind the other by a 256-lane step -- a wave owns a contiguous piece of the tile, so equal digits keep
//                        their input order inside a wave, across the waves and (by the scan) across the workgroups: the pass is stable.
#pragma once

#if !defined(RSQC_WAVE_EMU)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "../../include/rnaseqc_amd.h"

#define RSQC_SORT_THREADS 256
#define RSQC_SORT_ROUNDS 8                                             /* keys per lane and tile */
#define RSQC_SORT_TILE (RSQC_SORT_THREADS * RSQC_SORT_ROUNDS)          /* 2048 keys; LDS: 4 waves x 256 counters = 4 KiB, allocated as four 1 280-byte granules (5 120 B, 1 024 B of them unused) */
#define RSQC_SCAN_ITEMS 16
#define RSQC_SCAN_CHUNK (RSQC_SORT_THREADS * RSQC_SCAN_ITEMS)          /* entries one workgroup of the scan owns */
#define RSQC_SORT_PREP_GRID 1024                                       /* workgroups of sort_prepare_kernel: the size of its read-back */

namespace rsqc {

// the order of --sort: tid as UNSIGNED 32 bits (unplaced records, tid -1, go last; an unrecognised RefID sorts where its value puts
// it), then pos as SIGNED (the sign bit flipped: -1 sorts in front of 0)
inline __host__ __device__ uint64_t sort_key(int32_t tid, int32_t pos) { return ((uint64_t)(uint32_t)tid << 32) | (uint64_t)((uint32_t)pos ^ 0x80000000u); }
inline __host__ __device__ int32_t sort_key_tid(uint64_t key) { return (int32_t)(uint32_t)(key >> 32); }

// the digit positions a sort has to run: those in which the keys differ (OR and AND of all keys disagree).  Returns their number,
// the shifts ascending in `shift`
inline int sort_live_digits(uint64_t key_or, uint64_t key_and, int shift[8]) {
    const uint64_t differ = key_or ^ key_and;
    int n = 0;
    for (int d = 0; d < 8; ++d) if ((differ >> (8 * d)) & 0xFFu) shift[n++] = 8 * d;
    return n;
}

// what has been collected (device pointers): the records of every input batch one behind the other, their CIGAR pools likewise (a
// record's cigar_off stays relative to ITS batch's pool: the collection's pool may pass 2^32 operations), the wide tables merged
// (wide_index = index in the collection, ascending)
struct SortCollection {
    const rsqc_rec_core *core; const rsqc_rec_aux *aux; const uint32_t *qhash2; const uint32_t *cigar;
    const uint64_t *batch_rec0, *batch_pool0; uint32_t n_batches;      // first record / first operation of input batch k; batch_rec0[n_batches] = records
    const uint64_t *wide_index; const int32_t *wide_nm, *wide_l_qseq; const uint32_t *wide_n_cigar; uint64_t n_wide;
    uint64_t n_ops;                                                    // operations in `cigar`: no record reads past them, whatever its batch claimed
};
// one output batch (device pointers): the columns of rsqc_batch
struct SortOutput {
    rsqc_rec_core *core; rsqc_rec_aux *aux; uint32_t *qhash2; uint32_t *cigar;
    int32_t *seg_tid; uint64_t *seg_start;
    uint64_t *wide_index; int32_t *wide_nm, *wide_l_qseq; uint32_t *wide_n_cigar;
};

#if defined(RSQC_SORT_KERNELS) || defined(RSQC_WAVE_EMU)      /* the kernels: rsqc_sort.hip and the emulation only */
// exclusive prefix sum over the 256 lanes of a workgroup (every lane calls); total = the sum over all of them
__device__ inline unsigned long long sort_block_scan(unsigned long long v, unsigned long long &total) {
    __shared__ unsigned long long s_wave[RSQC_SORT_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    unsigned long long x = v;
    for (uint32_t o = 1; o < 64; o <<= 1) { const unsigned long long t = __shfl_up(x, o, 64); if (lane >= o) x += t; }
    if (lane == 63) s_wave[w] = x;
    __syncthreads();
    unsigned long long base = 0, tot = 0;
    for (uint32_t k = 0; k < RSQC_SORT_THREADS / 64; ++k) { const unsigned long long s = s_wave[k]; if (k < w) base += s; tot += s; }
    __syncthreads();                                   // (the next call writes s_wave again)
    total = tot;
    return base + x - v;
}
// first entry of the ascending table that is >= x, in [0, n]
__device__ inline uint64_t sort_lower_bound(const uint64_t *t, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t m = (lo + hi) >> 1; if (t[m] < x) lo = m + 1; else hi = m; }
    return lo;
}

// ---- collecting: the keys of one arriving batch (one lane per record), its wide table moved to collection indices --------------
__global__ __launch_bounds__(RSQC_SORT_THREADS) void sort_append_kernel(const rsqc_rec_core *core, uint64_t n, const int32_t *seg_tid, const uint64_t *seg_start, uint32_t n_seg,
                                                                         uint64_t *key_out /* at the batch's first record */, uint64_t rec0,
                                                                         const uint64_t *wide_index, const int32_t *wide_nm, const int32_t *wide_lq, const uint32_t *wide_nc, uint32_t n_wide,
                                                                         uint64_t *c_wide_index, int32_t *c_wide_nm, int32_t *c_wide_lq, uint32_t *c_wide_nc /* at the batch's first wide entry */) {
    const uint64_t i = (uint64_t)blockIdx.x * RSQC_SORT_THREADS + threadIdx.x;
    if (i < n) {
        // the segment of record i: the last one that starts at or before it (empty segments share a start: the last of them holds the record)
        uint32_t lo = 0, hi = n_seg;
        while (hi - lo > 1) { const uint32_t m = (lo + hi) >> 1; if (seg_start[m] <= i) lo = m; else hi = m; }
        key_out[i] = sort_key(n_seg ? seg_tid[lo] : -1, core[i].pos);
    }
    if (i < n_wide) {
        c_wide_index[i] = rec0 + wide_index[i];
        c_wide_nm[i] = wide_nm[i]; c_wide_lq[i] = wide_lq[i]; c_wide_nc[i] = wide_nc[i];
    }
}

// ---- before the sort: the payload (collection index), and per workgroup the OR and the AND of its keys and whether one of them is
// smaller than its predecessor -- part[3 * workgroup + {0, 1, 2}], one small read-back decides which digit positions run, if any
__global__ __launch_bounds__(RSQC_SORT_THREADS) void sort_prepare_kernel(const uint64_t *key, uint64_t n, uint32_t *idx, unsigned long long *part) {
    __shared__ unsigned long long s_or[RSQC_SORT_THREADS / 64], s_and[RSQC_SORT_THREADS / 64], s_dis[RSQC_SORT_THREADS / 64];
    unsigned long long o = 0ull, a = ~0ull, dis = 0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * RSQC_SORT_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RSQC_SORT_THREADS) {
        const unsigned long long k = key[i];
        o |= k; a &= k;
        if (i > 0 && key[i - 1] > k) dis = 1ull;
        idx[i] = (uint32_t)i;
    }
    for (int s = 32; s > 0; s >>= 1) { o |= __shfl_xor(o, s, 64); a &= __shfl_xor(a, s, 64); dis |= __shfl_xor(dis, s, 64); }
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) { s_or[w] = o; s_and[w] = a; s_dis[w] = dis; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t k = 1; k < RSQC_SORT_THREADS / 64; ++k) { o |= s_or[k]; a &= s_and[k]; dis |= s_dis[k]; }
        part[3 * blockIdx.x] = o; part[3 * blockIdx.x + 1] = a; part[3 * blockIdx.x + 2] = dis;
    }
}

// ---- one radix pass ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RSQC_SORT_THREADS) void sort_hist_kernel(const uint64_t *key, uint64_t n, int shift, uint32_t *hist, uint32_t n_tiles) {
    __shared__ uint32_t s_hist[256];
    s_hist[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * RSQC_SORT_TILE;
#pragma unroll
    for (int r = 0; r < RSQC_SORT_ROUNDS; ++r) {
        const uint64_t i = base + (uint64_t)r * RSQC_SORT_THREADS + threadIdx.x;
        if (i < n) atomicAdd(&s_hist[(uint32_t)(key[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(uint64_t)threadIdx.x * n_tiles + blockIdx.x] = s_hist[threadIdx.x];
}

// exclusive prefix sum of m 32-bit entries in place, sums carried in 64 bits: (1) a workgroup adds up its chunk, (2) ONE workgroup
// scans the chunk sums (total[0] = the sum of everything), (3) a workgroup scans its chunk from its chunk's base
__global__ __launch_bounds__(RSQC_SORT_THREADS) void sort_scan_sum_kernel(const uint32_t *data, uint64_t m, unsigned long long *chunk_sum) {
    const uint64_t first = (uint64_t)blockIdx.x * RSQC_SCAN_CHUNK + (uint64_t)threadIdx.x * RSQC_SCAN_ITEMS;
    unsigned long long s = 0;
    for (int k = 0; k < RSQC_SCAN_ITEMS; ++k) if (first + k < m) s += data[first + k];
    unsigned long long total;
    (void)sort_block_scan(s, total);
    if (threadIdx.x == 0) chunk_sum[blockIdx.x] = total;
}
__global__ __launch_bounds__(RSQC_SORT_THREADS) void sort_scan_top_kernel(unsigned long long *chunk_sum, uint64_t n_chunks, unsigned long long *total_out) {
    unsigned long long carry = 0;
    for (uint64_t j0 = 0; j0 < n_chunks; j0 += RSQC_SORT_THREADS) {
        const uint64_t j = j0 + threadIdx.x;
        const unsigned long long v = j < n_chunks ? chunk_sum[j] : 0ull;
        unsigned long long total;
        const unsigned long long ex = sort_block_scan(v, total);
        if (j < n_chunks) chunk_sum[j] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) total_out[0] = carry;
}
__global__ __launch_bounds__(RSQC_SORT_THREADS) void sort_scan_apply_kernel(uint32_t *data, uint64_t m, const unsigned long long *chunk_sum) {
    const uint64_t first = (uint64_t)blockIdx.x * RSQC_SCAN_CHUNK + (uint64_t)threadIdx.x * RSQC_SCAN_ITEMS;
    uint32_t v[RSQC_SCAN_ITEMS];
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < RSQC_SCAN_ITEMS; ++k) { v[k] = first + k < m ? data[first + k] : 0u; s += v[k]; }
    unsigned long long total;
    unsigned long long run = chunk_sum[blockIdx.x] + sort_block_scan(s, total);
#pragma unroll
    for (int k = 0; k < RSQC_SCAN_ITEMS; ++k) { if (first + k < m) data[first + k] = (uint32_t)run; run += v[k]; }
}

__global__ __launch_bounds__(RSQC_SORT_THREADS) void sort_scatter_kernel(const uint64_t *key_in, const uint32_t *idx_in, uint64_t *key_out, uint32_t *idx_out, uint64_t n, int shift,
                                                                          const uint32_t *slot /* the scanned table */, uint32_t n_tiles) {
    __shared__ uint32_t s_count[RSQC_SORT_THREADS / 64][256];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    for (uint32_t k = 0; k < RSQC_SORT_THREADS / 64; ++k) s_count[k][threadIdx.x] = 0u;
    __syncthreads();
    // wave w owns keys [w * 64 * ROUNDS, (w + 1) * 64 * ROUNDS) of the tile, a round is 64 consecutive keys
    const uint64_t first = (uint64_t)blockIdx.x * RSQC_SORT_TILE + (uint64_t)w * (64 * RSQC_SORT_ROUNDS) + lane;
    uint64_t key[RSQC_SORT_ROUNDS]; uint32_t idx[RSQC_SORT_ROUNDS], rank[RSQC_SORT_ROUNDS];
#pragma unroll
    for (int r = 0; r < RSQC_SORT_ROUNDS; ++r) {
        const uint64_t i = first + (uint64_t)r * 64;
        const bool valid = i < n;
        key[r] = valid ? key_in[i] : ~0ull; idx[r] = valid ? idx_in[i] : 0u;
        const uint32_t d = (uint32_t)(key[r] >> shift) & 255u;
        unsigned long long same = __ballot(valid);     // the lanes of this round that hold the digit d
#pragma unroll
        for (int b = 0; b < 8; ++b) { const bool bit = (d >> b) & 1u; const unsigned long long m = __ballot(bit); same &= bit ? m : ~m; }
        const uint32_t below = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        const uint32_t before = valid ? s_count[w][d] : 0u;             // ... and the ones of the wave's earlier rounds
        __builtin_amdgcn_wave_barrier();               // (every lane has read the counter before the first lane of a digit moves it on)
        if (valid && below == 0u) s_count[w][d] = before + (uint32_t)__popcll(same);
        __builtin_amdgcn_wave_barrier();
        rank[r] = before + below;
    }
    __syncthreads();
    {   // lane d: the waves' counts of digit d become each wave's first slot
        uint32_t at = slot[(uint64_t)threadIdx.x * n_tiles + blockIdx.x];
        for (uint32_t k = 0; k < RSQC_SORT_THREADS / 64; ++k) { const uint32_t c = s_count[k][threadIdx.x]; s_count[k][threadIdx.x] = at; at += c; }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RSQC_SORT_ROUNDS; ++r) {
        if (first + (uint64_t)r * 64 >= n) continue;
        const uint64_t p = (uint64_t)s_count[w][(uint32_t)(key[r] >> shift) & 255u] + rank[r];
        if (p < n) { key_out[p] = key[r]; idx_out[p] = idx[r]; }       // (p < n always; a store is never let out of the arrays)
    }
}

// ---- gathering ranks [r0, r0 + n) of the sorted order into one output batch ----------------------------------------------------
// the wide entry of collection record ci, or n_wide when it has none
__device__ inline uint64_t sort_wide_entry(const SortCollection &C, uint64_t ci) {
    const uint64_t k = sort_lower_bound(C.wide_index, C.n_wide, ci);
    return (k < C.n_wide && C.wide_index[k] == ci) ? k : C.n_wide;
}
__device__ inline bool sort_is_wide(const rsqc_rec_aux &a) { return a.n_cigar == RSQC_NCIGAR_ESCAPE || a.nm == RSQC_NM_ESCAPE || a.l_qseq == RSQC_LQSEQ_ESCAPE; }

// step 1, one lane per record: its operations, whether a contig segment starts at it, whether it has a wide entry (three columns for
// three prefix sums), and per workgroup how many records are not where they were collected
__global__ __launch_bounds__(RSQC_SORT_THREADS) void sort_gather_count_kernel(SortCollection C, const uint64_t *key, const uint32_t *idx, uint64_t r0, uint32_t n,
                                                                               uint32_t *n_ops, uint32_t *seg_mark, uint32_t *wide_mark, uint32_t *moved_part) {
    const uint32_t j = blockIdx.x * RSQC_SORT_THREADS + threadIdx.x;
    unsigned long long moved = 0;
    if (j < n) {
        const uint64_t ci = idx[r0 + j];
        const rsqc_rec_aux a = C.aux[ci];
        uint32_t ops = a.n_cigar, wide = 0u;
        if (sort_is_wide(a)) {
            const uint64_t k = sort_wide_entry(C, ci);
            wide = k < C.n_wide ? 1u : 0u;             // (an escape value without an entry stays one: the per-read kernels report it)
            if (a.n_cigar == RSQC_NCIGAR_ESCAPE) ops = wide ? C.wide_n_cigar[k] : 0u;
        }
        n_ops[j] = ops; wide_mark[j] = wide;
        seg_mark[j] = (j == 0 || sort_key_tid(key[r0 + j]) != sort_key_tid(key[r0 + j - 1])) ? 1u : 0u;
        moved = ci != r0 + j ? 1ull : 0ull;
    }
    unsigned long long total;
    (void)sort_block_scan(moved, total);
    if (threadIdx.x == 0) moved_part[blockIdx.x] = (uint32_t)total;
}
// step 2 (after the three prefix sums), one lane per record: the record's halves with cigar_off rewritten to the batch's compact pool,
// its operations, its segment and wide entries.  total_ops / n_seg: the sums of the marks (read back by the host)
__global__ __launch_bounds__(RSQC_SORT_THREADS) void sort_gather_kernel(SortCollection C, const uint64_t *key, const uint32_t *idx, uint64_t r0, uint32_t n,
                                                                         const uint32_t *ops_at, const uint32_t *seg_at, const uint32_t *wide_at, uint32_t total_ops, uint32_t n_seg, SortOutput O) {
    const uint32_t j = blockIdx.x * RSQC_SORT_THREADS + threadIdx.x;
    if (j >= n) return;
    const uint64_t ci = idx[r0 + j];
    rsqc_rec_core c = C.core[ci];
    const rsqc_rec_aux a = C.aux[ci];
    // the input batch of the record: the last one that starts at or before it
    uint32_t lo = 0, hi = C.n_batches;
    while (hi - lo > 1) { const uint32_t m = (lo + hi) >> 1; if (C.batch_rec0[m] <= ci) lo = m; else hi = m; }
    const uint64_t src = C.batch_pool0[lo] + c.cigar_off;
    const uint32_t at = ops_at[j], ops = (j + 1 < n ? ops_at[j + 1] : total_ops) - at;
    c.cigar_off = at;
    O.core[j] = c; O.aux[j] = a;
    if (C.qhash2) O.qhash2[j] = C.qhash2[ci];
    for (uint32_t k = 0; k < ops; ++k) O.cigar[at + k] = src + k < C.n_ops ? C.cigar[src + k] : 0u;
    const int32_t tid = sort_key_tid(key[r0 + j]);
    if (j == 0 || tid != sort_key_tid(key[r0 + j - 1])) { O.seg_tid[seg_at[j]] = tid; O.seg_start[seg_at[j]] = j; }
    if (j == 0) O.seg_start[n_seg] = n;
    if (sort_is_wide(a)) {
        const uint64_t k = sort_wide_entry(C, ci);
        if (k < C.n_wide) { const uint32_t wslot = wide_at[j]; O.wide_index[wslot] = j; O.wide_nm[wslot] = C.wide_nm[k]; O.wide_l_qseq[wslot] = C.wide_l_qseq[k]; O.wide_n_cigar[wslot] = C.wide_n_cigar[k]; }
    }
}

#endif

#if !defined(RSQC_WAVE_EMU)
// launchers (rsqc_sort.hip)
void launch_sort_append(hipStream_t s, const rsqc_rec_core *core, uint64_t n, const int32_t *seg_tid, const uint64_t *seg_start, uint32_t n_seg, uint64_t *key_out, uint64_t rec0,
                        const uint64_t *wide_index, const int32_t *wide_nm, const int32_t *wide_lq, const uint32_t *wide_nc, uint32_t n_wide,
                        uint64_t *c_wide_index, int32_t *c_wide_nm, int32_t *c_wide_lq, uint32_t *c_wide_nc);
void launch_sort_prepare(hipStream_t s, const uint64_t *key, uint64_t n, uint32_t *idx, unsigned long long *part, uint32_t grid);
// exclusive prefix sum of data[0, m) in place; chunk_sum: ceil(m / RSQC_SCAN_CHUNK) words of scratch; total_out[0] = the sum
void launch_sort_scan(hipStream_t s, uint32_t *data, uint64_t m, unsigned long long *chunk_sum, unsigned long long *total_out);
// one stable pass on the digit at `shift`; hist: 256 * ceil(n / RSQC_SORT_TILE) words
void launch_sort_pass(hipStream_t s, const uint64_t *key_in, const uint32_t *idx_in, uint64_t *key_out, uint32_t *idx_out, uint64_t n, int shift,
                      uint32_t *hist, unsigned long long *chunk_sum, unsigned long long *total_out);
void launch_sort_gather_count(hipStream_t s, const SortCollection &C, const uint64_t *key, const uint32_t *idx, uint64_t r0, uint32_t n,
                              uint32_t *n_ops, uint32_t *seg_mark, uint32_t *wide_mark, uint32_t *moved_part);
void launch_sort_gather(hipStream_t s, const SortCollection &C, const uint64_t *key, const uint32_t *idx, uint64_t r0, uint32_t n,
                        const uint32_t *ops_at, const uint32_t *seg_at, const uint32_t *wide_at, uint32_t total_ops, uint32_t n_seg, const SortOutput &O);
#endif

}  // namespace rsqc
