// rsqc_track.h -- the kernels of --bedgraph (rsqc_track_begin / rsqc_track_end / rsqc_track_rows / rsqc_track_text): the per-base
// coverage track of a pass as bedGraph rows.  Written like rsqc_junction.h against the HIP wave intrinsics only (__ballot, __shfl*,
// LDS): the same source runs under the 64-lane emulation of tests/hostemu/wavemu.h (tests/hostemu/track_emu.cpp) against a plain
// restatement of the contract (tests/track_ref.py).  No rocPRIM.
//
// The contract, in integers:
//   contigs      the track covers the n contigs handed to rsqc_track_begin (the header's @SQ entries in order) with their lengths,
//                each at most 2^31 - 1; names are optional (needed only for text) and at most 255 bytes each
//   population   a record contributes iff (flag & (0x4 | 0x100 | 0x200 | 0x800)) == 0 and its segment's tid is in [0, n): the
//                population of --junctions.  Nothing else gates it: not -q, the tag filters, --exclude-chimeric, --legacy,
//                --unpaired, --stranded, nor the duplicate flag.  The two mates of a pair are two records: where they overlap the
//                depth is 2
//   walk         p = pos, in 64 bits; the operations in order (a wide record's true count, clamped to the batch's pool): M = X of
//                length L >= 1 cover [p, p + L) and advance p; D and N advance p and cover nothing; I S H P do neither; an operation
//                of length 0 does nothing.  The part of an interval outside [0, length[tid]) is counted in no depth: its bases are
//                summed in clipped_bases, the bases inside in aligned_bases
//   depth        of a position: the number of covering intervals, exact up to 2^32 - 1 (32-bit modular arithmetic)
//   rows         a row is a maximal run of positions of ONE contig with equal, non-zero depth: (tid, start, end, depth), start
//                0-based, end exclusive, ascending by (tid, start).  A run never crosses a contig boundary.  The sum of
//                (end - start) * depth over the rows is aligned_bases.  The table does not depend on the order of the records or
//                on how they are cut into batches
//   text         each row is name<TAB>start<TAB>end<TAB>depth<LF> in decimal; no header or track line; no rows, no bytes
//
// Layout: ONE uint32_t difference array over all contigs.  Contig t starts at off[t] = sum over u < t of (length[u] + 1); its slot
// length[t] is a pad.  An interval clipped to [a, b), a < b <= length, adds +1 at off + a and -1 at off + b (b == length: the pad),
// so every contig's slots sum to zero, ONE prefix sum over the whole array gives the depths and every pad reads 0 -- which is why
// runs end at contig boundaries by themselves.  Indices are 64-bit.  The prefix sum is rsqc_sort.h's exclusive scan over total + 1
// slots: the depth of slot i is then read at i + 1.
//
//   track_events_kernel    per batch, one lane per record: the population test, the segment, the wide table and the pool clamp of
//                          junction_extract_kernel; one walk over the CIGAR that joins M = X operations which only I S H P or
//                          empty operations separate into one interval; non-returning atomicAdds.  Event ordinal 0 (the first
//                          interval's start) is merged across the wave: lanes that hold the same address are contiguous in a sorted
//                          file, a ballot of heads cuts the wave into runs and a run's last lane adds the run's length.  MERGE_LATER:
//                          the same for every later ordinal (in lock-step), else plain per-lane atomics.  The two base sums and
//                          the population: a workgroup reduction, then one atomic each per workgroup
//   track_count_kernel     heads per chunk of RSQC_TRACK_CHUNK slots (a head: non-zero depth that differs from its predecessor's)
//   track_rows_kernel      ranks the heads and the tails (non-zero depth that differs from its successor's) of a chunk -- ballot,
//                          popcount, the waves' counts through LDS -- and writes row k's tid / start / depth at the k-th head and its
//                          end at the k-th tail: the tails in front of a wave are the heads in front of it minus one if a run is open
//                          at the wave's first slot.  No second full-length array
//   track_linelen_kernel   bytes of every row's line in a window: the name + three digit counts + 4
//   track_format_kernel    every row writes its line at its offset (the exclusive scan of the lengths)
#pragma once

#if !defined(RSQC_WAVE_EMU)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "../../include/rnaseqc_amd.h"

#define RSQC_TRACK_THREADS 256
#define RSQC_TRACK_ROUNDS 16
#define RSQC_TRACK_WAVE_SPAN (64 * RSQC_TRACK_ROUNDS)                            /* slots one wave of the row kernels owns */
#define RSQC_TRACK_CHUNK ((RSQC_TRACK_THREADS / 64) * RSQC_TRACK_WAVE_SPAN)      /* 4096 slots per workgroup */
#define RSQC_TRACK_WINDOW 4194304ull            /* most rows of one rsqc_track_text call: 289 bytes a line at most, below 2^32 */
#define RSQC_TRACK_MAX_ROWS 0xFFFFFFF0ull       /* rows of one pass: fewer than this */
#define RSQC_TRACK_NAME_MAX 255
#define RSQC_TRACK_MERGE_LATER_DEFAULT true     /* events behind the first: merged like it (environment: RSQC_TRACK_MERGE) */
#define RSQC_TRACK_EXCLUDED (RSQC_FUNMAP | RSQC_FSECONDARY | RSQC_FQCFAIL | RSQC_FSUPP)

namespace rsqc {

// what the events kernel reads of one batch (device pointers; the columns of DevBatch)
struct TrackBatch {
    const rsqc_rec_core *core; const rsqc_rec_aux *aux; const uint32_t *cigar; uint64_t n, n_ops;
    const int32_t *seg_tid; const uint64_t *seg_start; uint32_t n_seg;
    const uint64_t *wide_index; const uint32_t *wide_n_cigar; uint32_t n_wide;
};
// the difference array: off[n + 1] (off[n] = all slots), length[n]; sums: [0] population, [1] aligned bases, [2] clipped bases
struct TrackArray { uint32_t *diff; const uint64_t *off; const uint32_t *length; int32_t n; unsigned long long *sums; };
// the table's columns (device pointers)
struct TrackRows { int32_t *tid; uint32_t *start, *end, *depth; };

#if defined(RSQC_TRACK_KERNELS) || defined(RSQC_WAVE_EMU)      /* the kernels: rsqc_track.hip and the emulation only */
__device__ inline int track_top_bit(unsigned long long x) {          // index of the highest set bit, x != 0
#if defined(RSQC_WAVE_EMU)
    return 63 - __builtin_clzll(x);
#else
    return 63 - __clzll((long long)x);
#endif
}
// the sum of v over the 256 lanes of a workgroup (every lane calls)
__device__ inline unsigned long long track_block_sum(unsigned long long v) {
    __shared__ unsigned long long s_wave[RSQC_TRACK_THREADS / 64];
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long tot = 0;
    for (uint32_t k = 0; k < RSQC_TRACK_THREADS / 64; ++k) tot += s_wave[k];
    __syncthreads();                                   // (the next call writes s_wave again)
    return tot;
}

// One event of every lane that has one (every lane of the wave calls): lanes that hold the same address one behind the other are a
// run, and the run's last lane adds val * the run's length.  The same address in two runs of a wave is two atomics: still the sum.
__device__ inline void track_merged_add(uint32_t *diff, bool has, uint64_t addr, uint32_t val) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long prev = __shfl_up((unsigned long long)addr, 1, 64);
    const unsigned long long vmask = __ballot(has);
    const bool head = has && (lane == 0 || !((vmask >> (lane - 1u)) & 1ull) || prev != addr);
    const unsigned long long hmask = __ballot(head);
    if (!has) return;
    const unsigned long long upto = (2ull << lane) - 1ull;            // bits [0, lane]  (lane 63: 2 << 63 wraps to 0, minus 1 = all)
    const uint32_t run_lo = (uint32_t)track_top_bit(hmask & upto);    // (a lane with an event has a head at or below it)
    const unsigned long long stop = (hmask | ~vmask) & ~upto;         // the next head, or the next lane without an event
    const uint32_t run_hi = stop ? (uint32_t)__ffsll(stop) - 2u : 63u;
    if (lane == run_hi) atomicAdd(&diff[addr], val * (run_hi - run_lo + 1u));
}

// The walk over one record's operations, one interval at a time.
struct TrackWalk {
    const uint32_t *ops; uint32_t n_ops, k; long long p;
};
// the next interval [s, e) of the walk (e > s), or false at the record's end
__device__ inline bool track_next_interval(TrackWalk &w, long long &s, long long &e) {
    bool open = false;
    while (w.k < w.n_ops) {
        const uint32_t op = w.ops[w.k], len = op >> 4, code = op & 15u;
        if (len != 0u) {
            if (code == 0u || code == 7u || code == 8u) {              // M = X
                if (!open) { s = w.p; open = true; }
                w.p += len; e = w.p;
            } else if (code == 2u || code == 3u) {                     // D N
                if (open) return true;                                 // (this operation is seen again by the next call, with nothing open)
                w.p += len;
            }
        }
        ++w.k;
    }
    return open;
}
// the next interval with bases inside [0, length): clipped to [a, b); the bases of every interval inside and outside are summed
__device__ inline bool track_next_clipped(TrackWalk &w, long long length, uint64_t &a, uint64_t &b, unsigned long long &aligned, unsigned long long &clipped) {
    long long s = 0, e = 0;
    while (track_next_interval(w, s, e)) {
        const long long lo = s < 0 ? 0 : s, hi = e > length ? length : e;
        const long long in = hi > lo ? hi - lo : 0;
        aligned += (unsigned long long)in; clipped += (unsigned long long)(e - s - in);
        if (in) { a = (uint64_t)lo; b = (uint64_t)hi; return true; }
    }
    return false;
}

template <bool MERGE_LATER>
__global__ __launch_bounds__(RSQC_TRACK_THREADS) void track_events_kernel(TrackBatch B, TrackArray A) {
    const uint64_t i = (uint64_t)blockIdx.x * RSQC_TRACK_THREADS + threadIdx.x;
    TrackWalk w{B.cigar, 0u, 0u, 0};
    unsigned long long member = 0, aligned = 0, clipped = 0;
    uint64_t base = 0; long long length = 0;
    if (i < B.n && B.n_seg) {
        const rsqc_rec_aux a = B.aux[i];
        // the segment of record i: the last one that starts at or before it (empty segments share a start: the last of them holds the record)
        uint32_t lo = 0, hi = B.n_seg;
        while (hi - lo > 1) { const uint32_t m = (lo + hi) >> 1; if (B.seg_start[m] <= i) lo = m; else hi = m; }
        const int32_t tid = B.seg_tid[lo];
        if ((a.flag & RSQC_TRACK_EXCLUDED) == 0 && tid >= 0 && tid < A.n) {
            member = 1;
            const rsqc_rec_core c = B.core[i];
            uint32_t n_ops = a.n_cigar;
            if (a.n_cigar == RSQC_NCIGAR_ESCAPE) {     // the true count is in the wide table (an escape value without an entry: no operations)
                uint32_t wl = 0, wh = B.n_wide;
                while (wl < wh) { const uint32_t m = (wl + wh) >> 1; if (B.wide_index[m] < i) wl = m + 1; else wh = m; }
                n_ops = (wl < B.n_wide && B.wide_index[wl] == i) ? B.wide_n_cigar[wl] : 0u;
            }
            // (no record reads past the batch's pool, whatever it claims)
            if ((uint64_t)c.cigar_off >= B.n_ops) n_ops = 0u; else if ((uint64_t)n_ops > B.n_ops - c.cigar_off) n_ops = (uint32_t)(B.n_ops - c.cigar_off);
            w.ops = B.cigar + c.cigar_off; w.n_ops = n_ops; w.p = c.pos;
            base = A.off[tid]; length = (long long)A.length[tid];
        }
    }
    // ordinal 0, merged; the later ones in lock-step and merged, or lane by lane.  base + b <= base + length: the contig's pad at most
    uint64_t a = 0, b = 0;
    bool has = track_next_clipped(w, length, a, b, aligned, clipped);
    track_merged_add(A.diff, has, base + a, 1u);
    if (MERGE_LATER) {
        for (;;) {
            track_merged_add(A.diff, has, base + b, 0xFFFFFFFFu);
            if (has) has = track_next_clipped(w, length, a, b, aligned, clipped);
            if (__ballot(has) == 0ull) break;
            track_merged_add(A.diff, has, base + a, 1u);
        }
    } else {
        while (has) {
            atomicAdd(&A.diff[base + b], 0xFFFFFFFFu);
            has = track_next_clipped(w, length, a, b, aligned, clipped);
            if (has) atomicAdd(&A.diff[base + a], 1u);
        }
    }
    member = track_block_sum(member); aligned = track_block_sum(aligned); clipped = track_block_sum(clipped);
    if (threadIdx.x == 0) {
        if (member) atomicAdd(&A.sums[0], member);
        if (aligned) atomicAdd(&A.sums[1], aligned);
        if (clipped) atomicAdd(&A.sums[2], clipped);
    }
}

// S: the exclusive prefix sum of the difference array, total + 1 entries: the depth of slot i, 0 outside [0, total)
__device__ inline uint32_t track_depth(const uint32_t *S, uint64_t total, long long i) { return (i >= 0 && (uint64_t)i < total) ? S[i + 1] : 0u; }

// heads of one wave's span, counted (every lane of the wave calls)
__device__ inline uint32_t track_wave_heads(const uint32_t *S, uint64_t total, uint64_t first) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t heads = 0;
    for (uint32_t r = 0; r < RSQC_TRACK_ROUNDS; ++r) {
        const long long i = (long long)(first + (uint64_t)r * 64u + lane);
        const uint32_t d = track_depth(S, total, i);
        heads += (uint32_t)__popcll(__ballot(d != 0u && d != track_depth(S, total, i - 1)));
    }
    return heads;
}

__global__ __launch_bounds__(RSQC_TRACK_THREADS) void track_count_kernel(const uint32_t *S, uint64_t total, uint32_t *count) {
    __shared__ uint32_t s_heads[RSQC_TRACK_THREADS / 64];
    const uint32_t wv = threadIdx.x >> 6;
    const uint32_t heads = track_wave_heads(S, total, (uint64_t)blockIdx.x * RSQC_TRACK_CHUNK + (uint64_t)wv * RSQC_TRACK_WAVE_SPAN);
    if ((threadIdx.x & 63u) == 0) s_heads[wv] = heads;
    __syncthreads();
    if (threadIdx.x == 0) { uint32_t t = 0; for (uint32_t k = 0; k < RSQC_TRACK_THREADS / 64; ++k) t += s_heads[k]; count[blockIdx.x] = t; }
}

// heads_before: the exclusive prefix sum of track_count_kernel's counts; n_rows: their sum (no rank reaches it)
__global__ __launch_bounds__(RSQC_TRACK_THREADS) void track_rows_kernel(const uint32_t *S, uint64_t total, const uint32_t *heads_before, const uint64_t *off, int32_t n_contigs,
                                                                        uint64_t n_rows, TrackRows R) {
    __shared__ uint32_t s_heads[RSQC_TRACK_THREADS / 64];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t first = (uint64_t)blockIdx.x * RSQC_TRACK_CHUNK + (uint64_t)wv * RSQC_TRACK_WAVE_SPAN;
    const uint32_t mine = track_wave_heads(S, total, first);
    if (lane == 0) s_heads[wv] = mine;
    __syncthreads();
    uint64_t h_rank = heads_before[blockIdx.x];
    for (uint32_t k = 0; k < wv; ++k) h_rank += s_heads[k];
    // a run is open at this wave's first slot when the slot in front of it is inside a run that it does not end
    const uint32_t d_in_front = track_depth(S, total, (long long)first - 1);
    uint64_t t_rank = h_rank - ((d_in_front != 0u && d_in_front == track_depth(S, total, (long long)first)) ? 1u : 0u);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t r = 0; r < RSQC_TRACK_ROUNDS; ++r) {
        const long long i = (long long)(first + (uint64_t)r * 64u + lane);
        const uint32_t d = track_depth(S, total, i);
        const bool head = d != 0u && d != track_depth(S, total, i - 1), tail = d != 0u && d != track_depth(S, total, i + 1);
        const unsigned long long hmask = __ballot(head), tmask = __ballot(tail);
        if (head || tail) {
            int32_t lo = 0, hi = n_contigs;                // the contig of slot i: the last one that starts at or before it
            while (hi - lo > 1) { const int32_t m = (lo + hi) >> 1; if (off[m] <= (uint64_t)i) lo = m; else hi = m; }
            const uint32_t at = (uint32_t)((uint64_t)i - off[lo]);
            if (head) { const uint64_t k = h_rank + (uint32_t)__popcll(hmask & below); if (k < n_rows) { R.tid[k] = lo; R.start[k] = at; R.depth[k] = d; } }
            if (tail) { const uint64_t k = t_rank + (uint32_t)__popcll(tmask & below); if (k < n_rows) R.end[k] = at + 1u; }
        }
        h_rank += (uint32_t)__popcll(hmask); t_rank += (uint32_t)__popcll(tmask);
    }
}

__device__ inline uint32_t track_digits(uint32_t x) {
    return x < 10u ? 1u : x < 100u ? 2u : x < 1000u ? 3u : x < 10000u ? 4u : x < 100000u ? 5u : x < 1000000u ? 6u : x < 10000000u ? 7u : x < 100000000u ? 8u : x < 1000000000u ? 9u : 10u;
}
// writes x in decimal, `digits` bytes ending in front of `end`
__device__ inline void track_put(char *end, uint32_t x, uint32_t digits) {
    for (uint32_t k = 0; k < digits; ++k) { *--end = (char)('0' + x % 10u); x /= 10u; }
}
// rows [first, first + n) of the table: name_off[n_contigs + 1] into the names' bytes
__global__ __launch_bounds__(RSQC_TRACK_THREADS) void track_linelen_kernel(TrackRows R, uint64_t first, uint32_t n, const uint32_t *name_off, uint32_t *len) {
    const uint64_t k = (uint64_t)blockIdx.x * RSQC_TRACK_THREADS + threadIdx.x;
    if (k >= n) return;
    const int32_t t = R.tid[first + k];
    len[k] = (name_off[t + 1] - name_off[t]) + track_digits(R.start[first + k]) + track_digits(R.end[first + k]) + track_digits(R.depth[first + k]) + 4u;
}
// at: the exclusive prefix sum of the lengths
__global__ __launch_bounds__(RSQC_TRACK_THREADS) void track_format_kernel(TrackRows R, uint64_t first, uint32_t n, const uint32_t *name_off, const char *names, const uint32_t *at, char *text) {
    const uint64_t k = (uint64_t)blockIdx.x * RSQC_TRACK_THREADS + threadIdx.x;
    if (k >= n) return;
    const int32_t t = R.tid[first + k];
    const uint32_t s = R.start[first + k], e = R.end[first + k], d = R.depth[first + k];
    char *q = text + at[k];
    for (uint32_t j = name_off[t]; j < name_off[t + 1]; ++j) *q++ = names[j];
    *q++ = '\t';
    uint32_t g = track_digits(s); q += g; track_put(q, s, g); *q++ = '\t';
    g = track_digits(e); q += g; track_put(q, e, g); *q++ = '\t';
    g = track_digits(d); q += g; track_put(q, d, g); *q++ = '\n';
}
#endif

#if !defined(RSQC_WAVE_EMU)
// launchers (rsqc_track.hip)
void launch_track_events(hipStream_t s, const TrackBatch &B, const TrackArray &A, bool merge_later);
void launch_track_count(hipStream_t s, const uint32_t *S, uint64_t total, uint32_t *count);
void launch_track_rows(hipStream_t s, const uint32_t *S, uint64_t total, const uint32_t *heads_before, const uint64_t *off, int32_t n_contigs, uint64_t n_rows, const TrackRows &R);
void launch_track_linelen(hipStream_t s, const TrackRows &R, uint64_t first, uint32_t n, const uint32_t *name_off, uint32_t *len);
void launch_track_format(hipStream_t s, const TrackRows &R, uint64_t first, uint32_t n, const uint32_t *name_off, const char *names, const uint32_t *at, char *text);
#endif

}  // namespace rsqc
