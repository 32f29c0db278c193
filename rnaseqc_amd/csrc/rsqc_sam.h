// rsqc_sam.h -- device-side SAM text decode: what one window of text goes through (plain SAM copied up, or BGZF-compressed
// SAM after the inflate kernel) before the per-read kernels, as per-lane bodies shared by the HIP kernels (rsqc_sam.hip)
// and the host emulation of the tests (tests/hostemu/sam_emu.cpp).  The output is that of rsqc_decode.h: the same
// DecodeWindow columns and DecodeSummary, so everything after the decode is the BAM path's.
//
//   bitmap   one lane per 64 bytes: a bit per byte for '\t' and for the '\n' that ends a record line (blank lines are
//            not records); per 256 words (16 KiB) the count of record lines
//   lines    exclusive sums of the counts, then one lane per word writes the position of every record line's '\n'
//   header   while the stream has had no record: the '@' lines in front of the first record are the header's
//   fields   one lane per line: its 11 fields from the tab bitmap (SEQ and QUAL are hopped a word at a time), the CIGAR's
//            operator count; exclusive sums of the counts give every line's first operation slot
//   parse    one lane per line: sam_parse_fields -> core / aux / qhash2 / operations / RefID column
//   marks    one lane per line: contig change / wide / unrecognised-RefID marks, the unsorted-input test
//   lists    the marks in record order -> the batch's segment and wide tables (rsqc_decode.h's counts, a SAM write step)
#pragma once

#include "rsqc_samrec.h"
#include "rsqc_decode.h"

namespace rsqc {

// ---- capacities: what the C ABI allocates (rsqc_decode_api.cpp reserve_columns) for a window buffer of buf_bytes, and what a window may
// use of it.  The host emulation of the tests sizes its arrays with the same functions.
struct SamCaps { uint32_t rec_alloc, cigar_alloc; };
inline SamCaps sam_caps(size_t buf_bytes) {
    const size_t rec = buf_bytes / SAM_MIN_LINE + 4;                    // a record line is at least SAM_MIN_LINE bytes
    return SamCaps{(uint32_t)(rec < 0xFFFFFFF0u ? rec : 0xFFFFFFF0u),
                   (uint32_t)(buf_bytes / 2 + 64)};                     // an operation is at least 2 bytes of text ("1M")
}
// record slots of a window of window_bytes: until the stream has had records, header lines (shorter than SAM_MIN_LINE) may fill it
inline uint32_t sam_window_rec_cap(uint32_t rec_alloc, uint32_t window_bytes, bool records_before) {
    const uint32_t w = window_bytes / SAM_MIN_LINE + 1u;
    return records_before && w < rec_alloc ? w : rec_alloc;
}

constexpr uint32_t SAM_SEG_WORDS = 256;              // words of 64 bytes per segment (one workgroup of the bitmap stage)
constexpr uint32_t SAM_NONE = 0xFFFFFFFFu;

struct SamStatus {                                   // per window (cleared by the host before the stages)
    uint32_t n_lines;                                // record lines (header lines included) in the window
    uint32_t n_nl;                                   // every '\n' of the window (blank and header lines included)
    uint32_t last_nl1;                               // one past the window's last '\n' (0: none)
    uint32_t hdr_end;                                // first line that is not a header line (SAM_NONE: none)
    uint32_t hdr;                                    // header lines in front of the window's records
    uint32_t first_bad;                              // first malformed record (SAM_NONE: none), its code
    uint32_t bad_code;
    uint32_t overflow;                               // more lines than the window's record slots (short, i.e. malformed, lines)
};
struct SamCarry { uint32_t records_seen; };          // the stream has had a record: '@' lines are malformed from here on

struct SamWindow {
    DecodeWindow W;                                  // rec_off[i] = position of the '\n' that ends line i
    uint64_t *ebits, *tbits;                         // record-line ends, tabs: bit b of word w <-> byte base + 64 w + b
    uint32_t base, n_words, n_seg, rec_cap;
    uint32_t cigar_cap;                              // operation slots of W.cigar
    uint32_t *seg_cnt, *seg_k0;                      // record lines per segment, their exclusive sums
    int32_t *rtid; uint32_t *nops;                   // per record: RefID, operations
    SamRefTable refs;
    SamStatus *st; SamCarry *sc;
};

// ---- bitmap ----------------------------------------------------------------------------------------------------------
// the bytes of x (8 of them) equal to c, as 8 bits
RSQC_BAM_FN uint32_t sam_eq8(uint64_t x, uint32_t c) {
    const uint64_t t = x ^ (0x0101010101010101ull * c);
    const uint64_t hi = ~(((t & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | t) & 0x8080808080808080ull;
    return (uint32_t)(((hi >> 7) * 0x0102040810204080ull) >> 56);
}
struct SamWordCounts { uint32_t rec, nl, last_nl1; };
RSQC_BAM_FN SamWordCounts sam_bitmap_word(const SamWindow &S, uint32_t w) {
    const DecodeWindow &W = S.W;
    const uint32_t p = S.base + (w << 6);
    uint64_t nl = 0, tb = 0, cr = 0;
    for (uint32_t q = 0; q < 8u; ++q) {
        uint64_t x; __builtin_memcpy(&x, W.buf + p + 8u * q, 8);
        nl |= (uint64_t)sam_eq8(x, '\n') << (8u * q); tb |= (uint64_t)sam_eq8(x, '\t') << (8u * q); cr |= (uint64_t)sam_eq8(x, '\r') << (8u * q);
    }
    uint64_t vm = ~0ull;
    if (W.start > p) vm = W.start - p >= 64u ? 0ull : vm << (W.start - p);
    if (W.end < p + 64u) vm &= W.end <= p ? 0ull : (1ull << (W.end - p)) - 1ull;
    nl &= vm; tb &= vm; cr &= vm;
    // line starts: behind every '\n', and the window's first byte
    auto is_ls = [&](uint32_t a) { return a == W.start || (a > W.start && W.buf[a - 1] == '\n'); };
    uint64_t ls = nl << 1;
    if (p >= W.start && is_ls(p)) ls |= 1ull;
    if (W.start > p && W.start - p < 64u) ls |= 1ull << (W.start - p);
    uint64_t blank = nl & (ls | ((cr & ls) << 1));       // "\n" or "\r\n" on its own
    if (p >= W.start + 1u && W.buf[p - 1] == '\r' && is_ls(p - 1)) blank |= nl & 1ull;
    const uint64_t e = nl & ~blank;
    S.ebits[w] = e; S.tbits[w] = tb;
    return SamWordCounts{(uint32_t)__builtin_popcountll(e), (uint32_t)__builtin_popcountll(nl), nl ? p + 64u - (uint32_t)__builtin_clzll(nl) : 0u};
}
// lines: the record lines ending in word w, numbered from k0
RSQC_BAM_FN void sam_lines_word(const SamWindow &S, uint32_t w, uint32_t k0) {
    uint64_t e = S.ebits[w];
    const uint32_t p = S.base + (w << 6);
    for (uint32_t k = k0; e; ++k) {
        const uint32_t b = (uint32_t)__builtin_ctzll(e);
        e &= e - 1;
        if (k < S.rec_cap) S.W.rec_off[k] = p + b;
        else S.st->overflow = 1;
    }
}
// bytes of line i (record lines, header included): [ls, le), without blank lines in front, '\n' and a trailing '\r'
RSQC_BAM_FN void sam_line_bounds(const SamWindow &S, uint32_t i, uint32_t &ls, uint32_t &le) {
    const uint8_t *b = S.W.buf;
    le = S.W.rec_off[i];
    ls = i ? S.W.rec_off[i - 1] + 1u : S.W.start;
    while (ls < le && (b[ls] == '\n' || (b[ls] == '\r' && b[ls + 1] == '\n'))) ++ls;
    if (le > ls && b[le - 1] == '\r') --le;
}
RSQC_BAM_FN bool sam_is_header_line(const SamWindow &S, uint32_t i) {
    uint32_t ls, le;
    sam_line_bounds(S, i, ls, le);
    return le > ls && S.W.buf[ls] == '@';
}
// ---- fields: operations of record j -----------------------------------------------------------------------------------
RSQC_BAM_FN uint32_t sam_fields_one(const SamWindow &S, uint32_t j) {
    uint32_t ls, le, f[12];
    sam_line_bounds(S, S.st->hdr + j, ls, le);
    if (!sam_fields_bitmap(S.tbits, S.base, ls, le, f)) return 0;
    return sam_count_ops(S.W.buf + ls + f[5], f[6] - 1 - f[5]);
}
// record j parsed; cigar_out null = no operations written.  Returns SAM_OK or SAM_ERR_*.
RSQC_BAM_FN uint32_t sam_record(const SamWindow &S, uint32_t j, BamRecOut &o, uint32_t *cigar_out, uint32_t max_ops) {
    uint32_t ls, le, f[12];
    sam_line_bounds(S, S.st->hdr + j, ls, le);
    if (!sam_fields_bitmap(S.tbits, S.base, ls, le, f)) return SAM_ERR_FIELDS;
    return sam_parse_fields(S.W.buf + ls, le - ls, f, S.W.tags, S.refs, o, cigar_out, max_ops);
}
// ---- parse: record j into the columns; returns SAM_OK or the code -----------------------------------------------------
RSQC_BAM_FN uint32_t sam_parse_one(const SamWindow &S, uint32_t j) {
    const DecodeWindow &W = S.W;
    const uint32_t at = W.ops_at[j];
    // (valid lines always fit: their operations take 2 bytes of text each.  Operator counts of malformed lines can push the
    //  slots of later lines past the column: refused here, and the host then names the malformed line)
    if ((uint64_t)at + S.nops[j] > S.cigar_cap) return SAM_ERR_CIGAR;
    BamRecOut o;
    const uint32_t rc = sam_record(S, j, o, W.cigar + at, S.nops[j]);
    if (rc != SAM_OK) return rc;
    o.core.cigar_off = at;
    W.core[j] = o.core; W.aux[j] = o.aux; W.qh2[j] = o.qhash2;
    if (W.umi) W.umi[j] = o.umi;
    S.rtid[j] = o.tid;
    return SAM_OK;
}
// ---- marks: decode_parse_one's marks and unsorted test, on the parsed columns -----------------------------------------
RSQC_BAM_FN bool sam_aux_wide(const rsqc_rec_aux &a) {
    return a.l_qseq == RSQC_LQSEQ_ESCAPE || a.nm == RSQC_NM_ESCAPE || a.n_cigar == RSQC_NCIGAR_ESCAPE;
}
RSQC_BAM_FN void sam_mark_one(const SamWindow &S, uint32_t j, bool &unsorted) {
    const DecodeWindow &W = S.W;
    const int32_t tid = S.rtid[j];
    const rsqc_rec_aux a = W.aux[j];
    uint32_t m = 0;
    if (j == 0 || S.rtid[j - 1] != tid) m |= DEC_MARK_SEG;
    if (sam_aux_wide(a)) m |= DEC_MARK_WIDE;
    if (bam_flag_judged(a.flag)) {
        if (tid < 0 || tid >= W.tags.n_ref) m |= DEC_MARK_BADREF;
        else {
            m |= DEC_MARK_JUDGED;
            bool found = false; int32_t ptid = 0, ppos = 0;
            for (uint32_t k = j; k-- > 0;) {
                const int32_t t = S.rtid[k];
                if (!bam_flag_judged(W.aux[k].flag) || t < 0 || t >= W.tags.n_ref) continue;
                found = true; ptid = t; ppos = W.core[k].pos;
                break;
            }
            if (!found && W.carry->have_q) { found = true; ptid = W.carry->q_tid; ppos = W.carry->q_pos; }
            if (found && ptid == tid && ppos > W.core[j].pos) unsorted = true;
        }
    }
    W.mark[j] = (uint8_t)m;
}
// ---- lists: decode_lists_count counts the marks; the writes and the totals take tid / wide values from the SAM columns --
RSQC_BAM_FN void sam_lists_write(const SamWindow &S, uint32_t lo, uint32_t hi, DecodeListCounts base) {
    const DecodeWindow &W = S.W;
    for (uint32_t j = lo; j < hi; ++j) {
        const uint32_t m = W.mark[j];
        if (!(m & 7u)) continue;
        if (m & DEC_MARK_SEG) { W.seg_tid[base.seg] = S.rtid[j]; W.seg_start[base.seg] = j; ++base.seg; }
        if (m & DEC_MARK_WIDE) {
            BamRecOut o;
            (void)sam_record(S, j, o, nullptr, 0);
            W.wide_index[base.wide] = j; W.wide_nm[base.wide] = o.nm; W.wide_lq[base.wide] = o.l_seq; W.wide_nc[base.wide] = o.n_ops;
            ++base.wide;
        }
        if (m & DEC_MARK_BADREF) {
            if (base.bad < DEC_MAX_BAD) { uint32_t ls, le; sam_line_bounds(S, S.st->hdr + j, ls, le); W.sum->bad_off[base.bad] = ls; }
            ++base.bad;
        }
    }
}
RSQC_BAM_FN void sam_lists_finish(const SamWindow &S, uint32_t n, DecodeListCounts total) {
    const DecodeWindow &W = S.W;
    W.seg_start[total.seg] = n;
    W.sum->n_seg = total.seg; W.sum->n_wide = total.wide; W.sum->n_bad = total.bad;
    if (total.last_judged >= 0) { W.carry->have_q = 1; W.carry->q_tid = S.rtid[total.last_judged]; W.carry->q_pos = W.core[total.last_judged].pos; }
}
// after the header stage (one thread): the window's record count, where its unconsumed tail starts
RSQC_BAM_FN void sam_settle(const SamWindow &S) {
    SamStatus &st = *S.st;
    const uint32_t n_lines = st.n_lines < S.rec_cap ? st.n_lines : S.rec_cap;
    const uint32_t hdr = S.sc->records_seen ? 0u : (st.hdr_end < n_lines ? st.hdr_end : n_lines);
    st.hdr = hdr;
    S.W.sum->n_rec = n_lines - hdr;
    if (n_lines > hdr) S.sc->records_seen = 1;
    S.W.sum->consumed_end = st.last_nl1 ? st.last_nl1 : S.W.start;
    if (st.overflow || st.n_lines > S.rec_cap) { st.overflow = 1; S.W.sum->status |= DEC_ST_BAD_RECORD; S.W.sum->n_rec = 0; }
}

// host: the first malformed line of a window's text t[0, n) the stages refused, and its line number (line0 = the number of the
// window's first line; seen = the stream has had a record, so '@' lines are no longer header lines).  The same functions as the
// device.  false = no malformed line among the window's complete lines.
inline bool sam_find_bad_line(const uint8_t *t, size_t n, bool seen, const BamTagSpec &tags, uint64_t line0, uint64_t &line, uint32_t &code) {
    line = line0;
    for (size_t a = 0; a < n; ++line) {
        size_t b = a;
        while (b < n && t[b] != '\n') ++b;
        if (b == n) break;                                              // (an incomplete last line is the next window's)
        size_t len = b - a;
        if (len && t[a + len - 1] == '\r') --len;
        if (len) {
            if (!seen && t[a] == '@') { a = b + 1; continue; }
            seen = true;
            BamRecOut o;
            code = len > 0xFFFFFFF0u ? SAM_ERR_FIELDS : sam_parse_line(t + a, (uint32_t)len, tags, SamRefTable{nullptr, nullptr, 0, 0}, o, nullptr, 0);
            if (code != SAM_OK) return true;
        }
        a = b + 1;
    }
    return false;
}
inline const char *sam_error_text(uint32_t code) {
    switch (code) {
    case SAM_ERR_NUMBER: return "a number that does not parse or overflows its column";
    case SAM_ERR_CIGAR: return "a malformed CIGAR";
    case SAM_ERR_SEQ_CIGAR: return "CIGAR and query sequence are of different length";
    case SAM_ERR_QUAL: return "SEQ and QUAL are of different length";
    case SAM_ERR_HEADER: return "a header line after the first alignment";
    case SAM_ERR_QNAME: return "QNAME empty or longer than 254 characters";
    default: return "fewer than 11 fields or a malformed optional field";
    }
}

// words of scratch launch_sam_window needs for a window of rec_cap record slots and n_seg segments
inline size_t sam_scratch_words(uint32_t rec_cap, uint32_t n_seg) {
    return 16 + ((size_t)rec_cap + 255) / 256 + 1024 + ((size_t)n_seg + 255) / 256 + 1024 + 4 * (((size_t)rec_cap + 8191) / 8192 + 4);
}
#if defined(__HIPCC__)
// rsqc_sam.hip
void launch_sam_window(hipStream_t s, const SamWindow &S, uint32_t *scratch);
#endif

}  // namespace rsqc
