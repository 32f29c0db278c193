// rsqc_cycle.h -- base quality and composition by read cycle (--cycles, rsqc_cycles_*; the contract: include/rnaseqc_amd.h), written
// once as __host__ __device__ code like rsqc_umi.h: the device kernels (rsqc_cycle.hip), the host reader (host/bam.cpp) and the
// emulation harnesses (tests/hostemu/cycle_emu.cpp, cycle_fuzz.cpp) run this one definition of
//   the population and the end of a flag, the cycle of a query index, the base code of a BAM nibble and of a SAM byte, the quality
//   value of a BAM and of a SAM byte and its clamp,
// then the record as the host counts it (cycle_count_bam / cycle_count_sam: one thread, 64-bit tables) and as the device counts it
// (cycle_block: a wave per record, 32-bit tables of one tile of cycles in LDS, flushed once per workgroup).
#pragma once

#include <stdint.h>
#include "rsqc_bamrec.h"

namespace rsqc {

constexpr uint32_t CYC_MAX = RSQC_CYCLE_MAX, CYC_QBINS = RSQC_CYCLE_QBINS, CYC_ENDS = RSQC_CYCLE_ENDS, CYC_BASES = RSQC_CYCLE_BASES;
constexpr uint32_t CYC_BASE_CELLS = CYC_ENDS * CYC_MAX * CYC_BASES, CYC_QUAL_CELLS = CYC_ENDS * CYC_MAX * CYC_QBINS;
// the scalar words behind the tables; LEN_SUM is the sum of L over the population, what bases + beyond_bases is checked against
constexpr uint32_t CYC_S_RECORDS = 0, CYC_S_NO_SEQ = 1, CYC_S_NO_QUAL = 2, CYC_S_BEYOND = 3, CYC_S_CLAMPED = 4, CYC_S_LEN_SUM = 5, CYC_S_WORDS = 8;
constexpr uint32_t CYC_TABLE_WORDS = CYC_BASE_CELLS + CYC_QUAL_CELLS + CYC_S_WORDS;     // base | qual | scalars, 64 bits each

RSQC_BAM_FN bool cycle_counted(uint32_t flag) { return (flag & (RSQC_FSECONDARY | RSQC_FQCFAIL | RSQC_FSUPP)) == 0; }
RSQC_BAM_FN uint32_t cycle_end(uint32_t flag) { return ((flag & 0x1u) && (flag & 0x80u) && !(flag & 0x40u)) ? 1u : 0u; }
RSQC_BAM_FN uint32_t cycle_of_index(uint32_t i, uint32_t L, uint32_t flag) { return (flag & 0x10u) ? L - 1u - i : i; }   // (its own inverse)
RSQC_BAM_FN uint32_t cycle_base_nibble(uint32_t nib) { return nib == 1u ? 0u : nib == 2u ? 1u : nib == 4u ? 2u : nib == 8u ? 3u : 4u; }
RSQC_BAM_FN uint32_t cycle_base_text(uint32_t byte) {
    switch (byte | 0x20u) {                           // (only the letter's two cases give its lower case with this bit set)
    case 'a': return 0u;
    case 'c': return 1u;
    case 'g': return 2u;
    case 't': return 3u;
    default: return 4u;
    }
}
RSQC_BAM_FN uint32_t cycle_base_strand(uint32_t b, uint32_t flag) { return ((flag & 0x10u) && b < 4u) ? 3u - b : b; }
RSQC_BAM_FN uint32_t cycle_qual_text(uint32_t byte) { return byte < 33u ? 0u : byte - 33u; }
RSQC_BAM_FN uint32_t cycle_qual_clamp(uint32_t q, uint32_t &clamped) { clamped = q >= CYC_QBINS ? 1u : 0u; return clamped ? CYC_QBINS - 1u : q; }

// base code (strand applied) and quality value of query index i.  TEXT: SEQ / QUAL are SAM text, else BAM nibbles / bytes
template <bool TEXT> RSQC_BAM_FN uint32_t cycle_base_at(const uint8_t *seq, uint32_t i, uint32_t flag) {
    uint32_t b;
    if (TEXT) b = cycle_base_text(seq[i]);
    else { const uint32_t two = seq[i >> 1]; b = cycle_base_nibble((i & 1u) ? (two & 15u) : (two >> 4)); }
    return cycle_base_strand(b, flag);
}
template <bool TEXT> RSQC_BAM_FN uint32_t cycle_qual_at(const uint8_t *qual, uint32_t i) { return TEXT ? cycle_qual_text(qual[i]) : (uint32_t)qual[i]; }

// SEQ and QUAL of a SAM line s[0, len) with the fields f of sam_fields_bytes / sam_fields_bitmap: offsets from s, L (0 for *) and whether
// QUAL is there.  false: a field lies outside the line, is empty, or QUAL is neither * nor as long as SEQ (sam_parse_fields refuses
// the same lines: such a record contributes nothing)
RSQC_BAM_FN bool cycle_sam_layout(const uint8_t *s, uint32_t len, const uint32_t f[12], uint32_t &seq_off, uint32_t &qual_off, uint32_t &L, uint32_t &have_q) {
    if (f[9] >= f[10] || f[10] >= f[11] || (uint64_t)f[11] > (uint64_t)len + 1u) return false;
    const uint32_t sqlen = f[10] - 1u - f[9], qulen = f[11] - 1u - f[10];
    if (sqlen == 0 || qulen == 0) return false;
    L = (sqlen == 1u && s[f[9]] == '*') ? 0u : sqlen;
    have_q = (qulen == 1u && s[f[10]] == '*') ? 0u : 1u;
    if (have_q && qulen != L) return false;
    seq_off = f[9]; qual_off = f[10];
    return true;
}

// ---- one thread, 64-bit tables: the host reader, and what the tests hold the kernels against ------------------------------------
struct CycleCounts {
    uint64_t *base, *qual;               // [CYC_BASE_CELLS], [CYC_QUAL_CELLS]
    uint64_t s[CYC_S_WORDS];
};
template <bool TEXT> RSQC_BAM_FN void cycle_count_record(const uint8_t *seq, const uint8_t *qual, uint32_t L, uint32_t have_q, uint32_t flag, CycleCounts &C) {
    if (L == 0) { C.s[CYC_S_NO_SEQ] += 1; return; }
    C.s[CYC_S_RECORDS] += 1; C.s[CYC_S_LEN_SUM] += L;
    if (!have_q) C.s[CYC_S_NO_QUAL] += 1;
    const uint32_t e = cycle_end(flag);
    for (uint32_t i = 0; i < L; ++i) {
        const uint32_t c = cycle_of_index(i, L, flag);
        if (c >= CYC_MAX) { C.s[CYC_S_BEYOND] += 1; continue; }
        C.base[(e * CYC_MAX + c) * CYC_BASES + cycle_base_at<TEXT>(seq, i, flag)] += 1;
        if (!have_q) continue;
        uint32_t clamped;
        const uint32_t q = cycle_qual_clamp(cycle_qual_at<TEXT>(qual, i), clamped);
        C.s[CYC_S_CLAMPED] += clamped;
        C.qual[(e * CYC_MAX + c) * CYC_QBINS + q] += 1;
    }
}
// the parsed length column (rsqc_rec_aux.l_qseq: l_seq, or the escape of a wide record) says that the record has no cycle c0 or beyond.
// Only the tiles behind the first ask (c0 > 0): the first tile looks at every record, it counts the records' scalars
RSQC_BAM_FN bool cycle_ends_before(uint32_t l_qseq, uint32_t c0) { return c0 > 0 && l_qseq != RSQC_LQSEQ_ESCAPE && l_qseq <= c0; }
// SEQ and QUAL of a BAM record (rec at its block_size field): bam_seq_layout's bound, and a read name (l_read_name counts its NUL: no
// record has 0).  false: the record contributes nothing
RSQC_BAM_FN bool cycle_bam_layout(const uint8_t *rec, uint32_t block_size, uint32_t &seq_off, uint32_t &qual_off, uint32_t &L) {
    return bam_seq_layout(rec, block_size, seq_off, qual_off, L) && rec[4 + 8] != 0;
}
// a BAM record; false: it contributes nothing (not of the population, or its fixed part does not fit)
RSQC_BAM_FN bool cycle_count_bam(const uint8_t *rec, uint32_t block_size, CycleCounts &C) {
    uint32_t so, qo, L;
    if (!cycle_bam_layout(rec, block_size, so, qo, L)) return false;
    const uint32_t flag = bam_ld16(rec + 4 + 14);
    if (!cycle_counted(flag)) return false;
    cycle_count_record<false>(rec + so, rec + qo, L, (L && rec[qo] != 0xFFu) ? 1u : 0u, flag, C);
    return true;
}
// a SAM line with its fields and its parsed flag
RSQC_BAM_FN bool cycle_count_sam(const uint8_t *s, uint32_t len, const uint32_t f[12], uint32_t flag, CycleCounts &C) {
    uint32_t so, qo, L, hq;
    if (!cycle_counted(flag) || !cycle_sam_layout(s, len, f, so, qo, L, hq)) return false;
    cycle_count_record<true>(s + so, s + qo, L, hq, flag, C);
    return true;
}

// ---- the device's form ------------------------------------------------------------------------------------------------------------
// A workgroup of CYC_WAVES waves (sixteen: the LDS of a CU holds two tiles, so this is what hides the latency of a record's loads) owns ONE tile of CYC_TILE cycles (both ends) as 32-bit cells in LDS and walks its share of the
// window's records.  The lanes of a wave first locate 64 records, one each (flag, SEQ / QUAL position, L, first quality byte); the
// wave then takes the located records that reach into the tile one at a time: lane l counts cycles c0 + l, c0 + l + 64 of the tile, so
// QUAL is read coalesced (forward or backward), two lanes share a SEQ byte, and no two lanes of one instruction hit one cycle.  The LDS
// cells are laid out [end][value][cycle]: the 64 lanes of an instruction then fall into 64 different banks whatever their values are
// ([cycle][value] would put equal qualities -- the common case -- into one bank).  A window holds fewer than 2^26 records, so a cell
// cannot wrap inside a launch.  At the end the workgroup adds its non-zero cells to the 64-bit tables with one global atomic each, and
// its scalars with one atomic per word: no global atomic per record.
constexpr uint32_t CYC_TILE = 128, CYC_TILES = CYC_MAX / CYC_TILE, CYC_WAVES = 16, CYC_THREADS = 64 * CYC_WAVES;
constexpr uint32_t CYC_LDS_QUAL = CYC_ENDS * CYC_QBINS * CYC_TILE, CYC_LDS_BASE = CYC_ENDS * CYC_BASES * CYC_TILE;

struct CycleTables { unsigned long long *base, *qual, *scal; };      // device: CYC_BASE_CELLS, CYC_QUAL_CELLS, CYC_S_WORDS

#if defined(__HIPCC__) || defined(RSQC_WAVE_EMU)
// Src: n records; locate(j, c0, flag, seq_at, qual_at, L, have_q) -> does record j count, and where its bytes lie in bytes() -- it may
// answer no without looking at the record when the parsed length column says that the record ends in front of cycle c0 > 0; TEXT
template <class Src>
__device__ __forceinline__ void cycle_block(const Src &src, uint32_t n, const CycleTables &T, uint32_t tile, uint32_t block, uint32_t n_blocks) {
    __shared__ uint32_t s_qual[CYC_LDS_QUAL];
    __shared__ uint32_t s_base[CYC_LDS_BASE];
    __shared__ uint32_t s_scal[CYC_S_WORDS];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    for (uint32_t k = t; k < CYC_LDS_QUAL; k += CYC_THREADS) s_qual[k] = 0u;
    for (uint32_t k = t; k < CYC_LDS_BASE; k += CYC_THREADS) s_base[k] = 0u;
    if (t < CYC_S_WORDS) s_scal[t] = 0u;
    __syncthreads();
    const uint32_t c0 = tile * CYC_TILE;
    const uint8_t *bytes = src.bytes();
    uint32_t n_rec = 0, n_noseq = 0, n_noqual = 0, n_beyond = 0, n_clamped = 0, n_len = 0;       // this lane's share of the scalars
    const uint32_t stride = n_blocks * CYC_WAVES * 64u;
    for (uint32_t first = (block * CYC_WAVES + wave) * 64u; first < n; first += stride) {       // (wave-uniform: n < 2^26, no wrap)
        const uint32_t j = first + lane;
        uint32_t flag = 0, seq_at = 0, qual_at = 0, L = 0, have_q = 0;
        const bool in = j < n && src.locate(j, c0, flag, seq_at, qual_at, L, have_q);
        if (in && tile == 0) {                                                                   // the scalars of a record are counted once: by tile 0
            if (L == 0) ++n_noseq;
            else { ++n_rec; n_len += L; if (!have_q) ++n_noqual; if (L > CYC_MAX) n_beyond += L - CYC_MAX; }
        }
        unsigned long long todo = __ballot(in && L > c0);                                        // records with a cycle in this tile
        while (todo) {
            const int k = __ffsll(todo) - 1;
            todo &= todo - 1ull;
            // (the record's five words travel in two: L | flag << 32 | have_q << 48 and seq_at | qual_at << 32)
            const unsigned long long w0 = __shfl((unsigned long long)L | (unsigned long long)flag << 32 | (unsigned long long)have_q << 48, k, 64);
            const unsigned long long w1 = __shfl((unsigned long long)seq_at | (unsigned long long)qual_at << 32, k, 64);
            const uint32_t rL = (uint32_t)w0, rflag = (uint32_t)(w0 >> 32) & 0xFFFFu, rhq = (uint32_t)(w0 >> 48);
            const uint8_t *seq = bytes + (uint32_t)w1, *qual = bytes + (uint32_t)(w1 >> 32);
            const uint32_t e = cycle_end(rflag);
            const uint32_t c1 = rL < c0 + CYC_TILE ? rL : c0 + CYC_TILE;
            for (uint32_t c = c0 + lane; c < c1; c += 64u) {
                const uint32_t i = cycle_of_index(c, rL, rflag);
                atomicAdd(&s_base[(e * CYC_BASES + cycle_base_at<Src::TEXT>(seq, i, rflag)) * CYC_TILE + (c - c0)], 1u);
                if (rhq) {
                    uint32_t clamped;
                    const uint32_t q = cycle_qual_clamp(cycle_qual_at<Src::TEXT>(qual, i), clamped);
                    n_clamped += clamped;
                    atomicAdd(&s_qual[(e * CYC_QBINS + q) * CYC_TILE + (c - c0)], 1u);
                }
            }
        }
    }
    if (n_rec) atomicAdd(&s_scal[CYC_S_RECORDS], n_rec);
    if (n_noseq) atomicAdd(&s_scal[CYC_S_NO_SEQ], n_noseq);
    if (n_noqual) atomicAdd(&s_scal[CYC_S_NO_QUAL], n_noqual);
    if (n_beyond) atomicAdd(&s_scal[CYC_S_BEYOND], n_beyond);                                    // (a window is under 2^31 bytes: the sums fit 32 bits)
    if (n_clamped) atomicAdd(&s_scal[CYC_S_CLAMPED], n_clamped);
    if (n_len) atomicAdd(&s_scal[CYC_S_LEN_SUM], n_len);
    __syncthreads();
    for (uint32_t k = t; k < CYC_LDS_QUAL; k += CYC_THREADS) {
        const uint32_t v = s_qual[k];
        if (!v) continue;
        const uint32_t cc = k % CYC_TILE, q = (k / CYC_TILE) % CYC_QBINS, e = k / (CYC_TILE * CYC_QBINS);
        atomicAdd(&T.qual[(e * CYC_MAX + c0 + cc) * CYC_QBINS + q], (unsigned long long)v);
    }
    for (uint32_t k = t; k < CYC_LDS_BASE; k += CYC_THREADS) {
        const uint32_t v = s_base[k];
        if (!v) continue;
        const uint32_t cc = k % CYC_TILE, b = (k / CYC_TILE) % CYC_BASES, e = k / (CYC_TILE * CYC_BASES);
        atomicAdd(&T.base[(e * CYC_MAX + c0 + cc) * CYC_BASES + b], (unsigned long long)v);
    }
    if (t < CYC_S_WORDS && s_scal[t]) atomicAdd(&T.scal[t], (unsigned long long)s_scal[t]);
}
#endif

}  // namespace rsqc

#if defined(__HIPCC__) || defined(RSQC_WAVE_EMU)
#include "rsqc_sam.h"

namespace rsqc {

// the records of a parsed BAM window: buf, rec_off[0, n_rec) and the flag column.  Nothing outside [rec, rec + 4 + block_size) is read
struct CycleBamSrc {
    static constexpr bool TEXT = false;
    DecodeWindow W;
    RSQC_BAM_FN const uint8_t *bytes() const { return W.buf; }
    RSQC_BAM_FN bool locate(uint32_t j, uint32_t c0, uint32_t &flag, uint32_t &seq_at, uint32_t &qual_at, uint32_t &L, uint32_t &have_q) const {
        const rsqc_rec_aux a = W.aux[j];
        flag = a.flag;
        if (!cycle_counted(flag) || cycle_ends_before(a.l_qseq, c0)) return false;
        const uint32_t at = W.rec_off[j];
        const uint8_t *rec = W.buf + at;
        uint32_t so, qo;
        if (!cycle_bam_layout(rec, bam_ld32(rec), so, qo, L)) return false;
        seq_at = at + so; qual_at = at + qo;
        have_q = (L && rec[qo] != 0xFFu) ? 1u : 0u;
        return true;
    }
};
// the record lines of a parsed SAM window (the header lines in front are skipped as the other stages skip them): f[9] / f[10] from the
// tab bitmap, the flag from the parsed column
struct CycleSamSrc {
    static constexpr bool TEXT = true;
    SamWindow S;
    RSQC_BAM_FN const uint8_t *bytes() const { return S.W.buf; }
    RSQC_BAM_FN bool locate(uint32_t j, uint32_t c0, uint32_t &flag, uint32_t &seq_at, uint32_t &qual_at, uint32_t &L, uint32_t &have_q) const {
        const rsqc_rec_aux a = S.W.aux[j];
        flag = a.flag;
        if (!cycle_counted(flag) || cycle_ends_before(a.l_qseq, c0)) return false;
        uint32_t ls, le, f[12], so, qo;
        sam_line_bounds(S, S.st->hdr + j, ls, le);
        if (!sam_fields_bitmap(S.tbits, S.base, ls, le, f)) return false;
        if (!cycle_sam_layout(S.W.buf + ls, le - ls, f, so, qo, L, have_q)) return false;
        seq_at = ls + so; qual_at = ls + qo;
        return true;
    }
};

#if defined(__HIPCC__)
// rsqc_cycle.hip: the stage of one window, behind its parse stage on the same stream
void launch_cycle_bam(hipStream_t s, const DecodeWindow &W, const CycleTables &T);
void launch_cycle_sam(hipStream_t s, const SamWindow &S, const CycleTables &T);
#endif

}  // namespace rsqc
#endif
