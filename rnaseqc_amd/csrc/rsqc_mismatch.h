// rsqc_mismatch.h -- errors by read cycle against the reference (--mismatches, rsqc_mismatch_*; the contract: include/rnaseqc_amd.h),
// written once as __host__ __device__ code like rsqc_cycle.h: the device kernels (rsqc_mismatch.hip), the host reader (host/bam.cpp) and
// the emulation harnesses (tests/hostemu/mismatch_emu.cpp, mismatch_fuzz.cpp) run this one definition of
//   the reference code of a FASTA byte and the packed word of eight of them, the class of a record, and the walk of its operations over
//   SEQ, QUAL and the reference (mismatch_walk: one body, run by one thread with stride 1 and by the 64 lanes of a wave with stride 64),
// then the record as the host counts it (mismatch_count_bam / mismatch_count_sam: one thread, 64-bit tables) and as the device counts it
// (mismatch_block: a wave per record, the whole cycle table as 32-bit cells in LDS, flushed once per workgroup).
// The end of a flag, the cycle of an index, the base and quality codes and the clamp are rsqc_cycle.h's: one definition for both stages.
#pragma once

#include <stdint.h>
#include "rsqc_cycle.h"

namespace rsqc {

constexpr uint32_t MM_ENDS = RSQC_CYCLE_ENDS, MM_MAX = RSQC_CYCLE_MAX, MM_COLS = RSQC_MISMATCH_COLS, MM_QBINS = RSQC_CYCLE_QBINS;
// the columns of a cycle
constexpr uint32_t MM_COMPARED = 0, MM_MISMATCH = 1, MM_UNCOMPARED = 2, MM_INSERTED = 3, MM_CLIPPED = 4, MM_DELETIONS = 5;
constexpr uint32_t MM_CYC_CELLS = MM_ENDS * MM_MAX * MM_COLS, MM_SUBST_CELLS = MM_ENDS * 16u, MM_BYQ_CELLS = MM_QBINS * 2u;
// the scalar words behind the tables.  The first six are the classes in the order they are tested (MM_S_EXCLUDED is never stored: such a
// record is counted nowhere but in seen_records); LEN_SUM is the sum of L over `records`, what the columns are checked against
constexpr uint32_t MM_S_EXCLUDED = 0, MM_S_NO_REF = 1, MM_S_LOW_MAPQ = 2, MM_S_NO_SEQ = 3, MM_S_INCONSISTENT = 4, MM_S_RECORDS = 5, MM_S_NO_QUAL = 6,
                   MM_S_BEYOND = 7, MM_S_CLAMPED = 8, MM_S_INS_EVENTS = 9, MM_S_DEL_EVENTS = 10, MM_S_DEL_BASES = 11, MM_S_LEN_SUM = 12, MM_S_WORDS = 16;
constexpr uint32_t MM_TABLE_WORDS = MM_CYC_CELLS + MM_SUBST_CELLS + MM_BYQ_CELLS + MM_S_WORDS;      // cyc | subst | byq | scalars, 64 bits each
constexpr uint32_t MM_FLAG_EXCLUDED = RSQC_FUNMAP | RSQC_FSECONDARY | RSQC_FQCFAIL | RSQC_FSUPP;

// ---- the reference ------------------------------------------------------------------------------------------------------------------
// code of a FASTA byte: A C G T in either case 0..3, every other byte 4 (cycle_base_text); eight codes per 32-bit word, base 8 w + k in
// bits [4 k, 4 k + 4).  The places of a last word behind the contig's end hold 4
RSQC_BAM_FN uint32_t mismatch_pack_word(const uint8_t *ascii, uint64_t len, uint64_t w) {
    uint32_t x = 0;
    for (uint32_t k = 0; k < 8u; ++k) {
        const uint64_t i = w * 8u + k;
        x |= (i < len ? cycle_base_text(ascii[i]) : 4u) << (4u * k);
    }
    return x;
}
// A reference accessor answers contig(tid, view) -- false: tid outside [0, n) or a contig without sequence -- and the view the code at a
// position inside [0, length).  Packed words on the device ...
struct MismatchPackedRef {
    const uint32_t *words; const unsigned long long *off, *len;      // off[tid]: first word of the contig, ~0: the FASTA lacks it
    int32_t n;
    struct Contig {
        const uint32_t *w; uint64_t length;
        RSQC_BAM_FN uint32_t code(uint64_t p) const { return (w[p >> 3] >> (4u * ((uint32_t)p & 7u))) & 15u; }
    };
    RSQC_BAM_FN bool contig(int32_t tid, Contig &c) const {
        if (tid < 0 || tid >= n || off[tid] == ~0ull) return false;
        c.w = words + off[tid]; c.length = len[tid];
        return true;
    }
};
// ... and the FASTA strings the host reader keeps
struct MismatchTextRef {
    const char *const *seq; const uint64_t *len;
    int32_t n;
    struct Contig {
        const char *s; uint64_t length;
        RSQC_BAM_FN uint32_t code(uint64_t p) const { return cycle_base_text((uint8_t)s[p]); }
    };
    RSQC_BAM_FN bool contig(int32_t tid, Contig &c) const {
        if (tid < 0 || tid >= n || !seq[tid]) return false;
        c.s = seq[tid]; c.length = len[tid];
        return true;
    }
};

// ---- the operations of a record -----------------------------------------------------------------------------------------------------
// in the record's own bytes (BAM: any alignment) or in a parsed column (SAM)
struct MismatchOpsBytes { const uint8_t *p; RSQC_BAM_FN uint32_t operator()(uint32_t k) const { return bam_ld32(p + 4ull * k); } };
struct MismatchOpsWords { const uint32_t *p; RSQC_BAM_FN uint32_t operator()(uint32_t k) const { return p[k]; } };
RSQC_BAM_FN bool mismatch_op_takes_query(uint32_t code) { return code == 0u || code == 1u || code == 4u || code == 7u || code == 8u; }   // M I S = X

// ---- the classes: every record is in exactly one, tested in this order; the answer is the scalar word it counts in -----------------
template <class Ref, class Ops>
RSQC_BAM_FN uint32_t mismatch_class(uint32_t flag, int32_t tid, uint32_t mapq, uint32_t L, const Ref &ref, uint32_t min_mapq, const Ops &ops, uint32_t n_ops) {
    if (flag & MM_FLAG_EXCLUDED) return MM_S_EXCLUDED;
    typename Ref::Contig ct;
    if (!ref.contig(tid, ct)) return MM_S_NO_REF;
    if (mapq < min_mapq) return MM_S_LOW_MAPQ;
    if (L == 0) return MM_S_NO_SEQ;
    uint64_t qsum = 0;                                                // (at most 2^32 operations of under 2^28: no wrap)
    for (uint32_t k = 0; k < n_ops; ++k) { const uint32_t op = ops(k); if (mismatch_op_takes_query(op & 15u)) qsum += op >> 4; }
    return qsum == (uint64_t)L ? MM_S_RECORDS : MM_S_INCONSISTENT;
}

// ---- the walk of a record of class MM_S_RECORDS (so the query-consuming lengths add up to L: q + n <= L at every operation) ---------
// `lane` of `stride` workers share the record: the bases of an operation are dealt out k = lane, lane + stride, ...; what happens once per
// operation (a deletion, the events) is worker 0's.  One thread: lane 0 of stride 1.  The sink takes the counts:
//   cell(e, column, c)  subst(e, R, B)  byq(v, mismatched)  beyond()  clamped()  insertion()  deletion(n)
template <bool TEXT, class Ref, class Ops, class Sink>
RSQC_BAM_FN void mismatch_walk(const uint8_t *seq, const uint8_t *qual, uint32_t L, uint32_t have_q, uint32_t flag, int32_t pos, const typename Ref::Contig &ct,
                               const Ops &ops, uint32_t n_ops, uint32_t lane, uint32_t stride, Sink &sink) {
    const uint32_t e = cycle_end(flag);
    uint32_t q = 0;
    int64_t p = pos;
    for (uint32_t o = 0; o < n_ops; ++o) {
        const uint32_t op = ops(o), code = op & 15u, n = op >> 4;
        if (n == 0) continue;
        if (code == 0u || code == 7u || code == 8u) {                                   // M = X
            for (uint32_t k = lane; k < n; k += stride) {
                const uint32_t i = q + k, c = cycle_of_index(i, L, flag);
                if (c >= MM_MAX) { sink.beyond(); continue; }
                uint32_t b;
                if (TEXT) b = cycle_base_text(seq[i]);
                else { const uint32_t two = seq[i >> 1]; b = cycle_base_nibble((i & 1u) ? (two & 15u) : (two >> 4)); }
                const int64_t pp = p + (int64_t)k;
                const uint32_t r = (pp < 0 || (uint64_t)pp >= ct.length) ? 4u : ct.code((uint64_t)pp);
                if (b < 4u && r < 4u) {
                    const bool mm = b != r;
                    sink.cell(e, MM_COMPARED, c);
                    if (flag & 0x10u) sink.subst(e, 3u - r, 3u - b); else sink.subst(e, r, b);
                    if (mm) sink.cell(e, MM_MISMATCH, c);
                    if (have_q) {
                        uint32_t clamped;
                        const uint32_t v = cycle_qual_clamp(cycle_qual_at<TEXT>(qual, i), clamped);
                        if (clamped) sink.clamped();
                        sink.byq(v, mm);
                    }
                } else sink.cell(e, MM_UNCOMPARED, c);
            }
            q += n; p += n;
        } else if (code == 1u || code == 4u) {                                          // I S
            for (uint32_t k = lane; k < n; k += stride) {
                const uint32_t c = cycle_of_index(q + k, L, flag);
                if (c >= MM_MAX) sink.beyond(); else sink.cell(e, code == 1u ? MM_INSERTED : MM_CLIPPED, c);
            }
            if (code == 1u && lane == 0) sink.insertion();
            q += n;
        } else if (code == 2u) {                                                        // D: one event at the query index behind it
            if (lane == 0) {
                const uint32_t c = cycle_of_index(q < L - 1u ? q : L - 1u, L, flag);
                if (c < MM_MAX) sink.cell(e, MM_DELETIONS, c);
                sink.deletion(n);
            }
            p += n;
        } else if (code == 3u) p += n;                                                  // N  (H, P and the codes above 8 do nothing)
    }
}

// ---- one thread, 64-bit tables: the host reader, and what the tests hold the kernels against ----------------------------------------
struct MismatchCounts {
    uint64_t *cyc, *subst, *byq;         // [2][512][6], [2][4][4], [64][2]
    uint64_t s[MM_S_WORDS];
};
struct MismatchHostSink {
    MismatchCounts &C;
    RSQC_BAM_FN void cell(uint32_t e, uint32_t col, uint32_t c) { C.cyc[(e * MM_MAX + c) * MM_COLS + col] += 1; }
    RSQC_BAM_FN void subst(uint32_t e, uint32_t R, uint32_t B) { C.subst[e * 16u + R * 4u + B] += 1; }
    RSQC_BAM_FN void byq(uint32_t v, bool mm) { C.byq[v * 2u] += 1; if (mm) C.byq[v * 2u + 1u] += 1; }
    RSQC_BAM_FN void beyond() { C.s[MM_S_BEYOND] += 1; }
    RSQC_BAM_FN void clamped() { C.s[MM_S_CLAMPED] += 1; }
    RSQC_BAM_FN void insertion() { C.s[MM_S_INS_EVENTS] += 1; }
    RSQC_BAM_FN void deletion(uint32_t n) { C.s[MM_S_DEL_EVENTS] += 1; C.s[MM_S_DEL_BASES] += n; }
};
template <bool TEXT, class Ref, class Ops>
RSQC_BAM_FN void mismatch_count_record(const uint8_t *seq, const uint8_t *qual, uint32_t L, uint32_t have_q, uint32_t flag, int32_t tid, int32_t pos, uint32_t mapq,
                                       const Ops &ops, uint32_t n_ops, const Ref &ref, uint32_t min_mapq, MismatchCounts &C) {
    const uint32_t cls = mismatch_class(flag, tid, mapq, L, ref, min_mapq, ops, n_ops);
    if (cls == MM_S_EXCLUDED) return;
    C.s[cls] += 1;
    if (cls != MM_S_RECORDS) return;
    C.s[MM_S_LEN_SUM] += L;
    if (!have_q) C.s[MM_S_NO_QUAL] += 1;
    typename Ref::Contig ct;
    (void)ref.contig(tid, ct);
    MismatchHostSink sink{C};
    mismatch_walk<TEXT, Ref>(seq, qual, L, have_q, flag, pos, ct, ops, n_ops, 0u, 1u, sink);
}
// a BAM record (rec at its block_size field); false: it contributes nothing (its fixed part does not fit, or l_read_name is 0)
template <class Ref>
RSQC_BAM_FN bool mismatch_count_bam(const uint8_t *rec, uint32_t block_size, const Ref &ref, uint32_t min_mapq, MismatchCounts &C) {
    uint32_t so, qo, L, n_ops, ops_off;
    if (!cycle_bam_layout(rec, block_size, so, qo, L) || !bam_record_ops(rec, block_size, n_ops, ops_off)) return false;
    const uint8_t *r = rec + 4;
    mismatch_count_record<false>(rec + so, rec + qo, L, (L && rec[qo] != 0xFFu) ? 1u : 0u, bam_ld16(r + 14), (int32_t)bam_ld32(r), (int32_t)bam_ld32(r + 4), r[9],
                                 MismatchOpsBytes{rec + ops_off}, n_ops, ref, min_mapq, C);
    return true;
}
// a SAM line with its fields and what the parser made of RNAME, POS (0-based), MAPQ, FLAG and the CIGAR
template <class Ref>
RSQC_BAM_FN bool mismatch_count_sam(const uint8_t *s, uint32_t len, const uint32_t f[12], uint32_t flag, int32_t tid, int32_t pos, uint32_t mapq, const uint32_t *ops,
                                    uint32_t n_ops, const Ref &ref, uint32_t min_mapq, MismatchCounts &C) {
    uint32_t so, qo, L, hq;
    if (!cycle_sam_layout(s, len, f, so, qo, L, hq)) return false;
    mismatch_count_record<true>(s + so, s + qo, L, hq, flag, tid, pos, mapq, MismatchOpsWords{ops}, n_ops, ref, min_mapq, C);
    return true;
}

// ---- the device's form ----------------------------------------------------------------------------------------------------------------
// A workgroup of MM_WAVES waves holds the WHOLE cycle table (both ends, six columns, 512 cycles) as 32-bit cells in LDS, 24 KB, beside
// subst (128 B) and MM_BYQ_COPIES copies of byq (8 KB): no tiles, every record is visited once.  The lanes of a wave first locate 64
// records, one each: the class (with the sum of the query-consuming operations), where SEQ, QUAL and the operations lie, L, pos, tid and
// flag; they add their share of the class counts in registers.  The wave then takes the records of class `records` one at a time
// (mismatch_walk with stride 64): the operation loop is wave-uniform, the lanes stride over an operation's bases, so QUAL is read
// coalesced, two lanes share a SEQ byte and eight a reference word, and no two lanes of one instruction hit one cycle.  The cells are laid
// out [end][column][cycle]: the 64 lanes of an instruction fall into different banks.  Binned qualities put most lanes of an instruction on
// one value: a lane adds to copy lane & 15 of byq, the copies are summed at the flush.  A record of many one-base operations leaves 63
// lanes idle per step; accepted.
// No 32-bit cell can wrap inside a launch: every count is one query base (at least 1.5 bytes of a BAM record, one of a SAM line) or one D
// operation (4 bytes, 2 of text), and a window holds under 2^31 bytes.  The sums that are no counts (deleted bases, L) are 64-bit.
// At the end the workgroup adds its non-zero cells to the 64-bit tables with one global atomic each and its scalars with one per word.
constexpr uint32_t MM_WAVES = 16, MM_THREADS = 64 * MM_WAVES, MM_BYQ_COPIES = 16;
constexpr uint32_t MM_LDS_CYC = MM_ENDS * MM_COLS * MM_MAX, MM_LDS_BYQ = MM_BYQ_COPIES * MM_BYQ_CELLS;

struct MismatchTables { unsigned long long *cyc, *subst, *byq, *scal; };      // device: MM_CYC_CELLS, MM_SUBST_CELLS, MM_BYQ_CELLS, MM_S_WORDS

// what a lane knows of the record it located
struct MismatchRec { uint32_t flag, L, have_q, seq_at, qual_at, ops_at, n_ops, mapq; int32_t tid, pos; };

#if defined(__HIPCC__) || defined(RSQC_WAVE_EMU)
struct MismatchLdsSink {
    uint32_t *cyc, *sub, *byq_copy;                         // (byq_copy: this lane's copy)
    uint32_t n_beyond, n_clamped, n_ins, n_del;
    unsigned long long n_del_bases;
    __device__ __forceinline__ void cell(uint32_t e, uint32_t col, uint32_t c) { atomicAdd(&cyc[(e * MM_COLS + col) * MM_MAX + c], 1u); }
    __device__ __forceinline__ void subst(uint32_t e, uint32_t R, uint32_t B) { atomicAdd(&sub[e * 16u + R * 4u + B], 1u); }
    __device__ __forceinline__ void byq(uint32_t v, bool mm) { atomicAdd(&byq_copy[v * 2u], 1u); if (mm) atomicAdd(&byq_copy[v * 2u + 1u], 1u); }
    __device__ __forceinline__ void beyond() { ++n_beyond; }
    __device__ __forceinline__ void clamped() { ++n_clamped; }
    __device__ __forceinline__ void insertion() { ++n_ins; }
    __device__ __forceinline__ void deletion(uint32_t n) { ++n_del; n_del_bases += n; }
};

// Src: n records; locate(j, rec) -> false: record j contributes nothing; bytes(); ops(at) -> the operations at a located ops_at; TEXT
template <class Src>
__device__ __forceinline__ void mismatch_block(const Src &src, uint32_t n, const MismatchPackedRef &ref, uint32_t min_mapq, const MismatchTables &T, uint32_t block,
                                               uint32_t n_blocks) {
    __shared__ uint32_t s_cyc[MM_LDS_CYC];
    __shared__ uint32_t s_byq[MM_LDS_BYQ];
    __shared__ uint32_t s_sub[MM_SUBST_CELLS];
    __shared__ unsigned long long s_scal[MM_S_WORDS];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    for (uint32_t k = t; k < MM_LDS_CYC; k += MM_THREADS) s_cyc[k] = 0u;
    for (uint32_t k = t; k < MM_LDS_BYQ; k += MM_THREADS) s_byq[k] = 0u;
    if (t < MM_SUBST_CELLS) s_sub[t] = 0u;
    if (t < MM_S_WORDS) s_scal[t] = 0ull;
    __syncthreads();
    const uint8_t *bytes = src.bytes();
    MismatchLdsSink sink{s_cyc, s_sub, s_byq + (lane & (MM_BYQ_COPIES - 1u)) * MM_BYQ_CELLS, 0u, 0u, 0u, 0u, 0ull};
    uint32_t n_class[MM_S_RECORDS + 1u] = {0u, 0u, 0u, 0u, 0u, 0u}, n_noqual = 0;                     // this lane's share of the scalars
    unsigned long long n_len = 0;
    const uint32_t stride = n_blocks * MM_WAVES * 64u;
    for (uint32_t first = (block * MM_WAVES + wave) * 64u; first < n; first += stride) {             // (wave-uniform: n < 2^26, no wrap)
        const uint32_t j = first + lane;
        MismatchRec r{};
        uint32_t cls = MM_S_EXCLUDED;
        if (j < n && src.locate(j, r)) {
            cls = mismatch_class(r.flag, r.tid, r.mapq, r.L, ref, min_mapq, src.ops(r.ops_at), r.n_ops);
            for (uint32_t k = MM_S_NO_REF; k <= MM_S_RECORDS; ++k) n_class[k] += cls == k ? 1u : 0u;  // (no dynamic index: the counts stay in registers)
            if (cls == MM_S_RECORDS) { n_len += r.L; if (!r.have_q) ++n_noqual; }
        }
        unsigned long long todo = __ballot(cls == MM_S_RECORDS);
        while (todo) {
            const int k = __ffsll(todo) - 1;
            todo &= todo - 1ull;
            // (the record's words travel in four)
            const unsigned long long w0 = __shfl((unsigned long long)r.L | (unsigned long long)r.flag << 32 | (unsigned long long)r.have_q << 48, k, 64);
            const unsigned long long w1 = __shfl((unsigned long long)r.seq_at | (unsigned long long)r.qual_at << 32, k, 64);
            const unsigned long long w2 = __shfl((unsigned long long)r.ops_at | (unsigned long long)r.n_ops << 32, k, 64);
            const unsigned long long w3 = __shfl((unsigned long long)(uint32_t)r.tid | (unsigned long long)(uint32_t)r.pos << 32, k, 64);
            MismatchPackedRef::Contig ct;
            if (!ref.contig((int32_t)(uint32_t)w3, ct)) continue;                                    // (cannot be: the class says it has one)
            mismatch_walk<Src::TEXT, MismatchPackedRef>(bytes + (uint32_t)w1, bytes + (uint32_t)(w1 >> 32), (uint32_t)w0, (uint32_t)(w0 >> 48), (uint32_t)(w0 >> 32) & 0xFFFFu,
                                                        (int32_t)(uint32_t)(w3 >> 32), ct, src.ops((uint32_t)w2), (uint32_t)(w2 >> 32), lane, 64u, sink);
        }
    }
    if (n_class[MM_S_NO_REF]) atomicAdd(&s_scal[MM_S_NO_REF], (unsigned long long)n_class[MM_S_NO_REF]);
    if (n_class[MM_S_LOW_MAPQ]) atomicAdd(&s_scal[MM_S_LOW_MAPQ], (unsigned long long)n_class[MM_S_LOW_MAPQ]);
    if (n_class[MM_S_NO_SEQ]) atomicAdd(&s_scal[MM_S_NO_SEQ], (unsigned long long)n_class[MM_S_NO_SEQ]);
    if (n_class[MM_S_INCONSISTENT]) atomicAdd(&s_scal[MM_S_INCONSISTENT], (unsigned long long)n_class[MM_S_INCONSISTENT]);
    if (n_class[MM_S_RECORDS]) atomicAdd(&s_scal[MM_S_RECORDS], (unsigned long long)n_class[MM_S_RECORDS]);
    if (n_noqual) atomicAdd(&s_scal[MM_S_NO_QUAL], (unsigned long long)n_noqual);
    if (n_len) atomicAdd(&s_scal[MM_S_LEN_SUM], n_len);
    if (sink.n_beyond) atomicAdd(&s_scal[MM_S_BEYOND], (unsigned long long)sink.n_beyond);
    if (sink.n_clamped) atomicAdd(&s_scal[MM_S_CLAMPED], (unsigned long long)sink.n_clamped);
    if (sink.n_ins) atomicAdd(&s_scal[MM_S_INS_EVENTS], (unsigned long long)sink.n_ins);
    if (sink.n_del) atomicAdd(&s_scal[MM_S_DEL_EVENTS], (unsigned long long)sink.n_del);
    if (sink.n_del_bases) atomicAdd(&s_scal[MM_S_DEL_BASES], sink.n_del_bases);
    __syncthreads();
    for (uint32_t k = t; k < MM_LDS_CYC; k += MM_THREADS) {
        const uint32_t v = s_cyc[k];
        if (!v) continue;
        const uint32_t c = k % MM_MAX, col = (k / MM_MAX) % MM_COLS, e = k / (MM_MAX * MM_COLS);
        atomicAdd(&T.cyc[(e * MM_MAX + c) * MM_COLS + col], (unsigned long long)v);
    }
    for (uint32_t k = t; k < MM_BYQ_CELLS; k += MM_THREADS) {
        unsigned long long v = 0;
        for (uint32_t copy = 0; copy < MM_BYQ_COPIES; ++copy) v += s_byq[copy * MM_BYQ_CELLS + k];
        if (v) atomicAdd(&T.byq[k], v);
    }
    if (t < MM_SUBST_CELLS && s_sub[t]) atomicAdd(&T.subst[t], (unsigned long long)s_sub[t]);
    if (t < MM_S_WORDS && s_scal[t]) atomicAdd(&T.scal[t], s_scal[t]);
}
#endif

}  // namespace rsqc

#if defined(__HIPCC__) || defined(RSQC_WAVE_EMU)
namespace rsqc {

// the records of a parsed BAM window: tid at rec + 4, pos, mapq and flag from the parsed columns, the operations through bam_record_ops
// from the record's own bytes (a wide record's true count, a CG:B,I CIGAR's real one).  Nothing outside [rec, rec + 4 + block_size) is read
struct MismatchBamSrc {
    static constexpr bool TEXT = false;
    DecodeWindow W;
    RSQC_BAM_FN const uint8_t *bytes() const { return W.buf; }
    RSQC_BAM_FN MismatchOpsBytes ops(uint32_t at) const { return MismatchOpsBytes{W.buf + at}; }
    RSQC_BAM_FN bool locate(uint32_t j, MismatchRec &r) const {
        const uint32_t at = W.rec_off[j];
        const uint8_t *rec = W.buf + at;
        const uint32_t bs = bam_ld32(rec);
        uint32_t so, qo, oo;
        if (!cycle_bam_layout(rec, bs, so, qo, r.L) || !bam_record_ops(rec, bs, r.n_ops, oo)) return false;
        const rsqc_rec_aux a = W.aux[j];
        r.flag = a.flag; r.mapq = a.mapq; r.pos = W.core[j].pos; r.tid = (int32_t)bam_ld32(rec + 4);
        r.seq_at = at + so; r.qual_at = at + qo; r.ops_at = at + oo;
        r.have_q = (r.L && rec[qo] != 0xFFu) ? 1u : 0u;
        return true;
    }
};
// the record lines of a parsed SAM window: S.rtid, W.core.pos, W.aux, SEQ / QUAL through the tab bitmap, the operations from the parsed
// column W.cigar at W.ops_at[j], S.nops[j] of them (what the parse stage wrote there)
struct MismatchSamSrc {
    static constexpr bool TEXT = true;
    SamWindow S;
    RSQC_BAM_FN const uint8_t *bytes() const { return S.W.buf; }
    RSQC_BAM_FN MismatchOpsWords ops(uint32_t at) const { return MismatchOpsWords{S.W.cigar + at}; }
    RSQC_BAM_FN bool locate(uint32_t j, MismatchRec &r) const {
        uint32_t ls, le, f[12], so, qo;
        sam_line_bounds(S, S.st->hdr + j, ls, le);
        if (!sam_fields_bitmap(S.tbits, S.base, ls, le, f)) return false;
        if (!cycle_sam_layout(S.W.buf + ls, le - ls, f, so, qo, r.L, r.have_q)) return false;
        r.ops_at = S.W.ops_at[j]; r.n_ops = S.nops[j];
        if ((uint64_t)r.ops_at + r.n_ops > S.cigar_cap) return false;                 // (the parse stage refuses such a window)
        const rsqc_rec_aux a = S.W.aux[j];
        r.flag = a.flag; r.mapq = a.mapq; r.pos = S.W.core[j].pos; r.tid = S.rtid[j];
        r.seq_at = ls + so; r.qual_at = ls + qo;
        return true;
    }
};

#if defined(__HIPCC__)
// rsqc_mismatch.hip: the reference packed, and the stage of one window behind its parse stage on the same stream
void launch_mismatch_pack(hipStream_t s, const uint8_t *ascii, uint64_t len, uint32_t *words);
void launch_mismatch_bam(hipStream_t s, const DecodeWindow &W, const MismatchPackedRef &ref, uint32_t min_mapq, const MismatchTables &T);
void launch_mismatch_sam(hipStream_t s, const SamWindow &S, const MismatchPackedRef &ref, uint32_t min_mapq, const MismatchTables &T);
#endif

}  // namespace rsqc
#endif
