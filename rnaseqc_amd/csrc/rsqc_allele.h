// rsqc_allele.h -- base counts at known variant sites (--alleles, rsqc_alleles_*; the contract: include/rnaseqc_amd.h), written once as
// __host__ __device__ code like rsqc_mismatch.h: the device kernels (rsqc_allele.hip), the host reader (host/bam.cpp) and the emulation
// harnesses (tests/hostemu/allele_emu.cpp, allele_fuzz.cpp) run this one definition of
//   the site table as the accessor mismatch_class asks its second question of, the lower bound over a contig's sites, and the walk of a
//   record's operations over them (allele_walk: one body, one worker per record),
// then the record as the host counts it (allele_count_bam / allele_count_sam: one thread, a [site][7] table) and as the device counts it
// (allele_block: a LANE per record, [site][8] cells, an observation one no-return 64-bit global atomic or merged across the wave first).
// The class of a record is mismatch_class, the record sources are MismatchBamSrc / MismatchSamSrc (rsqc_mismatch.h), the base and quality
// codes are rsqc_cycle.h's: one definition for all three stages.
#pragma once

#include <stdint.h>
#include "rsqc_mismatch.h"

namespace rsqc {

constexpr uint32_t AL_COLS = RSQC_ALLELE_COLS;
// the columns of a site: 0..3 the base codes, then
constexpr uint32_t AL_OTHER = 4, AL_DELETED = 5, AL_LOW_BASEQ = 6;
// the device's cells: [site][AL_STRIDE], a site's seven counters in one 64-byte line (the eighth cell is never touched)
constexpr uint32_t AL_STRIDE = 8;
// the scalar words in front of the cells.  1..5 are the classes at mismatch_class's own numbers (MM_S_NO_REF: tid outside the contigs)
constexpr uint32_t AL_S_OFF_CONTIG = MM_S_NO_REF, AL_S_LOW_MAPQ = MM_S_LOW_MAPQ, AL_S_NO_SEQ = MM_S_NO_SEQ, AL_S_INCONSISTENT = MM_S_INCONSISTENT,
                   AL_S_RECORDS = MM_S_RECORDS, AL_S_NO_QUAL = 6, AL_S_HIT = 7, AL_S_OBS = 8, AL_S_WORDS = 16;

// ---- the sites --------------------------------------------------------------------------------------------------------------------------
// pos[n_sites] ascending within a contig; the sites of tid are [first[tid], first[tid + 1]).  As a reference accessor: contig() answers
// whether tid is one of the n contigs
struct AlleleSites {
    const int32_t *pos; const uint32_t *first;
    int32_t n;
    struct Contig { uint32_t lo, hi; };
    RSQC_BAM_FN bool contig(int32_t tid, Contig &c) const {
        if (tid < 0 || tid >= n) return false;
        c.lo = first[tid]; c.hi = first[tid + 1];
        return true;
    }
};
// the first site of [lo, hi) at or behind p
RSQC_BAM_FN uint32_t allele_lower_bound(const int32_t *pos, uint32_t lo, uint32_t hi, int64_t p) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if ((int64_t)pos[mid] < p) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// ---- the walk of a record of class `records` (so the query-consuming lengths add up to L: q + n <= L at every operation) --------------
// p only grows, so the cursor `cur` -- the first site of the contig at or behind p -- only moves forward: site by site under M = X and D,
// by a second lower bound over the rest behind an N.  The walk is ONE body written as a resumable cursor: next() hands out the record's
// observations one at a time.  One thread and a lane of the plain kernel drain it in a loop of their own; the lanes of the merging kernel
// take one step each per wave-uniform round, so that the wave can add up the lanes that meet on one cell before it touches memory
template <bool TEXT, class Ops> struct AlleleCursor {
    const uint8_t *seq, *qual; const int32_t *spos;
    Ops ops;
    uint32_t have_q, min_baseq, n_ops, hi;
    uint32_t o, q, cur, n, code;                  // the operation in turn; n, code: the M = X or D being walked while in_op
    int64_t p, end;
    bool in_op;
    RSQC_BAM_FN void begin(const uint8_t *seq_, const uint8_t *qual_, uint32_t have_q_, int32_t pos, const int32_t *spos_, const AlleleSites::Contig &ct, const Ops &ops_,
                           uint32_t n_ops_, uint32_t min_baseq_) {
        seq = seq_; qual = qual_; spos = spos_; ops = ops_; have_q = have_q_; min_baseq = min_baseq_; n_ops = n_ops_; hi = ct.hi;
        o = 0; q = 0; n = 0; code = 0; p = pos; end = pos; in_op = false;
        cur = allele_lower_bound(spos, ct.lo, ct.hi, p);
    }
    // the next observation (site, column); false: the record has no more
    RSQC_BAM_FN bool next(uint32_t &site, uint32_t &col) {
        for (;;) {
            if (in_op) {
                if (cur < hi && (int64_t)spos[cur] < end) {
                    site = cur;
                    if (code == 2u) col = AL_DELETED;                                   // D
                    else {                                                              // M = X
                        const uint32_t i = q + (uint32_t)((int64_t)spos[cur] - p);
                        uint32_t b;
                        if (TEXT) b = cycle_base_text(seq[i]);
                        else { const uint32_t two = seq[i >> 1]; b = cycle_base_nibble((i & 1u) ? (two & 15u) : (two >> 4)); }
                        col = (have_q && cycle_qual_at<TEXT>(qual, i) < min_baseq) ? AL_LOW_BASEQ : b;      // (b = 4 is AL_OTHER)
                    }
                    ++cur;
                    return true;
                }
                if (code != 2u) q += n;
                p = end; in_op = false; ++o;
            }
            if (o >= n_ops || cur >= hi) return false;                                  // (behind the contig's last site nothing counts)
            const uint32_t op = ops(o);
            code = op & 15u; n = op >> 4;
            if (n != 0u && (code == 0u || code == 7u || code == 8u || code == 2u)) { end = p + (int64_t)n; in_op = true; continue; }
            if (n != 0u && (code == 1u || code == 4u)) q += n;                          // I S
            else if (n != 0u && code == 3u) {                                           // N  (H, P and the codes above 8 do nothing)
                p += (int64_t)n;
                cur = allele_lower_bound(spos, cur, hi, p);
            }
            ++o;
        }
    }
};
// the sink takes the observations: obs(site, column)
template <bool TEXT, class Ops, class Sink>
RSQC_BAM_FN void allele_walk(const uint8_t *seq, const uint8_t *qual, uint32_t have_q, int32_t pos, const int32_t *spos, const AlleleSites::Contig &ct, const Ops &ops,
                             uint32_t n_ops, uint32_t min_baseq, Sink &sink) {
    AlleleCursor<TEXT, Ops> c;
    c.begin(seq, qual, have_q, pos, spos, ct, ops, n_ops, min_baseq);
    uint32_t site, col;
    while (c.next(site, col)) sink.obs(site, col);
}

// ---- one thread: the host reader, and what the tests hold the kernels against -------------------------------------------------------
// Cells: add(site, column) into a [site][AL_COLS] table
struct AlleleHostCells {
    uint64_t *counts;
    RSQC_BAM_FN void add(uint32_t site, uint32_t col) const { counts[(size_t)site * AL_COLS + col] += 1; }
};
template <class Cells> struct AlleleCounts {
    Cells cells;
    uint64_t s[AL_S_WORDS];
};
template <class Cells> struct AlleleHostSink {
    const Cells &cells; uint64_t n;
    RSQC_BAM_FN void obs(uint32_t site, uint32_t col) { cells.add(site, col); ++n; }
};
template <bool TEXT, class Ops, class Cells>
RSQC_BAM_FN void allele_count_record(const uint8_t *seq, const uint8_t *qual, uint32_t L, uint32_t have_q, uint32_t flag, int32_t tid, int32_t pos, uint32_t mapq, const Ops &ops,
                                     uint32_t n_ops, const AlleleSites &sites, uint32_t min_mapq, uint32_t min_baseq, AlleleCounts<Cells> &C) {
    const uint32_t cls = mismatch_class(flag, tid, mapq, L, sites, min_mapq, ops, n_ops);
    if (cls == MM_S_EXCLUDED) return;
    C.s[cls] += 1;
    if (cls != MM_S_RECORDS) return;
    if (!have_q) C.s[AL_S_NO_QUAL] += 1;
    AlleleSites::Contig ct;
    (void)sites.contig(tid, ct);
    AlleleHostSink<Cells> sink{C.cells, 0};
    allele_walk<TEXT>(seq, qual, have_q, pos, sites.pos, ct, ops, n_ops, min_baseq, sink);
    if (sink.n) { C.s[AL_S_HIT] += 1; C.s[AL_S_OBS] += sink.n; }
}
// a BAM record (rec at its block_size field); false: it contributes nothing (its fixed part does not fit, or l_read_name is 0)
template <class Cells>
RSQC_BAM_FN bool allele_count_bam(const uint8_t *rec, uint32_t block_size, const AlleleSites &sites, uint32_t min_mapq, uint32_t min_baseq, AlleleCounts<Cells> &C) {
    uint32_t so, qo, L, n_ops, ops_off;
    if (!cycle_bam_layout(rec, block_size, so, qo, L) || !bam_record_ops(rec, block_size, n_ops, ops_off)) return false;
    const uint8_t *r = rec + 4;
    allele_count_record<false>(rec + so, rec + qo, L, (L && rec[qo] != 0xFFu) ? 1u : 0u, bam_ld16(r + 14), (int32_t)bam_ld32(r), (int32_t)bam_ld32(r + 4), r[9],
                               MismatchOpsBytes{rec + ops_off}, n_ops, sites, min_mapq, min_baseq, C);
    return true;
}
// a SAM line with its fields and what the parser made of RNAME, POS (0-based), MAPQ, FLAG and the CIGAR
template <class Cells>
RSQC_BAM_FN bool allele_count_sam(const uint8_t *s, uint32_t len, const uint32_t f[12], uint32_t flag, int32_t tid, int32_t pos, uint32_t mapq, const uint32_t *ops,
                                  uint32_t n_ops, const AlleleSites &sites, uint32_t min_mapq, uint32_t min_baseq, AlleleCounts<Cells> &C) {
    uint32_t so, qo, L, hq;
    if (!cycle_sam_layout(s, len, f, so, qo, L, hq)) return false;
    allele_count_record<true>(s + so, s + qo, L, hq, flag, tid, pos, mapq, MismatchOpsWords{ops}, n_ops, sites, min_mapq, min_baseq, C);
    return true;
}

// ---- the device's form ----------------------------------------------------------------------------------------------------------------
// A lane per record: it locates its record, classes it and walks it alone -- 64 independent load chains per wave, with work only where a
// site lies under an aligned block.  Most records meet no site: they cost the locate, the class (one pass over the operations) and one
// lower bound.  The class counts, hit_records and the observations stay in registers; at the end a lane adds its non-zero words to LDS
// and the workgroup adds each non-zero word with one global atomic.  A 20 000-base record over a dense panel keeps one lane busy for
// thousands of steps while its 63 neighbours idle; accepted.
// Two forms of what an observation does to memory (RSQC_ALLELE_MERGE chooses, rsqc_allele_api.cpp):
//   plain   the lane drains its cursor; an observation is one no-return 64-bit global atomic on the site's line
//   merge   the wave takes its records' observations a step at a time -- every lane its next one, or none -- and before it touches
//           memory the lanes that meet on one cell are counted with a ballot: the first of them adds the count.  On a deep pile the
//           neighbouring records of a coordinate-sorted window observe the same cell in the same step.  At most AL_MERGE_ROUNDS cells a
//           step are merged, and the merging of a step ends at the second leader that nobody shares its cell with; what is left goes
//           lane by lane.  Every branch around a collective is wave-uniform
constexpr uint32_t AL_THREADS = 256, AL_MERGE_ROUNDS = 8;
#define RSQC_ALLELE_MERGE_DEFAULT true         /* environment: RSQC_ALLELE_MERGE; it measured faster on all three inputs */

struct AlleleTables { unsigned long long *scal, *cells; };        // device: AL_S_WORDS, n_sites * AL_STRIDE

#if defined(__HIPCC__) || defined(RSQC_WAVE_EMU)
// Src: n records; locate(j, rec) -> false: record j contributes nothing; bytes(); ops(at) -> the operations at a located ops_at; TEXT
template <bool MERGE, class Src>
__device__ __forceinline__ void allele_block(const Src &src, uint32_t n, const AlleleSites &sites, uint32_t min_mapq, uint32_t min_baseq, const AlleleTables &T, uint32_t block,
                                             uint32_t n_blocks) {
    __shared__ unsigned long long s_scal[AL_S_WORDS];
    const uint32_t t = threadIdx.x, lane = t & 63u;
    if (t < AL_S_WORDS) s_scal[t] = 0ull;
    __syncthreads();
    const uint8_t *bytes = src.bytes();
    uint32_t n_class[MM_S_RECORDS + 1u] = {0u, 0u, 0u, 0u, 0u, 0u}, n_noqual = 0, n_hit = 0;          // this lane's share of the scalars
    unsigned long long n_obs = 0;
    const uint32_t stride = n_blocks * AL_THREADS;
    for (uint32_t first = block * AL_THREADS + (t - lane); first < n; first += stride) {              // (wave-uniform; n < 2^26, at most 2^19 threads: no wrap)
        const uint32_t j = first + lane;
        MismatchRec r{};
        AlleleSites::Contig ct{0u, 0u};
        bool walk = false;
        if (j < n && src.locate(j, r)) {
            const uint32_t cls = mismatch_class(r.flag, r.tid, r.mapq, r.L, sites, min_mapq, src.ops(r.ops_at), r.n_ops);
            for (uint32_t k = MM_S_NO_REF; k <= MM_S_RECORDS; ++k) n_class[k] += cls == k ? 1u : 0u;  // (no dynamic index: the counts stay in registers)
            if (cls == MM_S_RECORDS) {
                if (!r.have_q) ++n_noqual;
                walk = sites.contig(r.tid, ct);                                                       // (true: the class says it is one)
            }
        }
        AlleleCursor<Src::TEXT, decltype(src.ops(0u))> c;
        if (walk) c.begin(bytes + r.seq_at, bytes + r.qual_at, r.have_q, r.pos, sites.pos, ct, src.ops(r.ops_at), r.n_ops, min_baseq);
        uint32_t mine = 0, site = 0, col = 0;                      // (a record observes under 2^32 sites: there are no more)
        if (!MERGE) {
            while (walk && c.next(site, col)) { atomicAdd(&T.cells[(size_t)site * AL_STRIDE + col], 1ull); ++mine; }
        } else {
            for (;;) {
                walk = walk && c.next(site, col);
                unsigned long long todo = __ballot(walk);
                if (!todo) break;
                const unsigned long long key = (unsigned long long)site * AL_STRIDE + col;
                bool pending = walk;
                if (walk) ++mine;
                for (uint32_t round = 0, lonely = 0; round < AL_MERGE_ROUNDS && todo; ++round) {
                    const int leader = __ffsll(todo) - 1;
                    const unsigned long long k = __shfl(key, leader, 64);
                    const unsigned long long same = __ballot(pending && key == k);
                    todo &= ~same;
                    const uint32_t cnt = (uint32_t)__popcll(same);
                    if (cnt < 2u) { if (++lonely == 2u) break; continue; }                            // (the leader stays pending: its own atomic below)
                    if (lane == (uint32_t)leader) atomicAdd(&T.cells[k], (unsigned long long)cnt);
                    if (key == k) pending = false;
                }
                if (pending) atomicAdd(&T.cells[key], 1ull);
            }
        }
        if (mine) { ++n_hit; n_obs += mine; }
    }
    if (n_class[AL_S_OFF_CONTIG]) atomicAdd(&s_scal[AL_S_OFF_CONTIG], (unsigned long long)n_class[AL_S_OFF_CONTIG]);
    if (n_class[AL_S_LOW_MAPQ]) atomicAdd(&s_scal[AL_S_LOW_MAPQ], (unsigned long long)n_class[AL_S_LOW_MAPQ]);
    if (n_class[AL_S_NO_SEQ]) atomicAdd(&s_scal[AL_S_NO_SEQ], (unsigned long long)n_class[AL_S_NO_SEQ]);
    if (n_class[AL_S_INCONSISTENT]) atomicAdd(&s_scal[AL_S_INCONSISTENT], (unsigned long long)n_class[AL_S_INCONSISTENT]);
    if (n_class[AL_S_RECORDS]) atomicAdd(&s_scal[AL_S_RECORDS], (unsigned long long)n_class[AL_S_RECORDS]);
    if (n_noqual) atomicAdd(&s_scal[AL_S_NO_QUAL], (unsigned long long)n_noqual);
    if (n_hit) atomicAdd(&s_scal[AL_S_HIT], (unsigned long long)n_hit);
    if (n_obs) atomicAdd(&s_scal[AL_S_OBS], n_obs);
    __syncthreads();
    if (t < AL_S_WORDS && s_scal[t]) atomicAdd(&T.scal[t], s_scal[t]);
}
#endif

#if defined(__HIPCC__)
// rsqc_allele.hip: the stage of one window behind its parse stage on the same stream
void launch_allele_bam(hipStream_t s, const DecodeWindow &W, const AlleleSites &sites, uint32_t min_mapq, uint32_t min_baseq, const AlleleTables &T, bool merge);
void launch_allele_sam(hipStream_t s, const SamWindow &S, const AlleleSites &sites, uint32_t min_mapq, uint32_t min_baseq, const AlleleTables &T, bool merge);
#endif

}  // namespace rsqc
