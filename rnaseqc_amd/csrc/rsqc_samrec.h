// rsqc_samrec.h -- SAM text alignment lines (SAM spec 1.6 section 1.4) to the boundary's batch columns, written once as
// __host__ __device__ code like rsqc_bamrec.h: the device SAM stages (rsqc_sam.hip), the host side of the C ABI (the line
// number of a malformed line) and tests/hostemu/sam_emu.cpp run the same functions.
//
// For any alignment, sam_parse_fields on its SAM line and bam_parse_record on its BAM record fill the same BamRecOut
// (core, aux incl. qhash / tagbits, qhash2, nm, l_seq, n_ops, wide) and the same operations.  The reference reads SAM
// through SeqLib -> htslib's sam_parse1; where a rule below is htslib's, it is marked "htslib" ("SAM text":
// recalled, not pinned against an htslib build).  SEQ and QUAL are never read, only their lengths are taken.
#pragma once

#include <stdint.h>
#include "rsqc_bamrec.h"

namespace rsqc {

// sam_parse_fields results (0 = a record)
constexpr uint32_t SAM_OK = 0, SAM_ERR_FIELDS = 1, SAM_ERR_NUMBER = 2, SAM_ERR_CIGAR = 3, SAM_ERR_SEQ_CIGAR = 4,
                   SAM_ERR_QUAL = 5, SAM_ERR_HEADER = 6, SAM_ERR_QNAME = 7;
constexpr uint32_t SAM_MIN_LINE = 22;          // the shortest valid line, '\n' included: 11 one-byte fields and 10 tabs

// ---- @SQ names: an open-addressed table keyed on bam_qname_hash of the name, the bytes compared on a hit ----------------
struct SamRefSlot { uint64_t hash; uint32_t off, len; int32_t idx, pad; };   // idx -1 = empty
struct SamRefTable {
    const SamRefSlot *slot; const uint8_t *names;
    uint32_t mask;                             // slots - 1 (a power of two, at least twice the names)
    int32_t n_ref;
};
RSQC_BAM_FN int32_t sam_ref_lookup(const SamRefTable &T, const uint8_t *s, uint32_t len) {
    if (T.n_ref <= 0) return -1;
    const uint64_t h = bam_qname_hash(s, len);
    for (uint32_t k = (uint32_t)h & T.mask;; k = (k + 1) & T.mask) {
        const SamRefSlot e = T.slot[k];
        if (e.idx < 0) return -1;
        if (e.hash == h && e.len == len) {
            uint32_t i = 0;
            while (i < len && T.names[e.off + i] == s[i]) ++i;
            if (i == len) return e.idx;
        }
    }
}

// ---- the rule for records whose reference is not a placed one (htslib sam_parse1, as recalled) ------------------------
// RNAME "*" -> tid -1, the flag as written.  A name that the header's @SQ lines do not define -> tid -1 AND the unmapped bit
// ("unrecognized reference name; treated as unmapped").  A record with a known RNAME and POS 0 -> tid -1 AND the unmapped
// bit ("mapped query cannot have zero coordinate; treated as unmapped").  One function, so that the rule is in one place.
RSQC_BAM_FN void sam_place(bool rname_star, int32_t found_tid, int32_t pos, int32_t &tid, uint32_t &flag) {
    if (rname_star) { tid = -1; return; }
    tid = found_tid;
    if (tid < 0) { flag |= RSQC_FUNMAP; return; }
    if (pos < 0) { tid = -1; flag |= RSQC_FUNMAP; }
}

// ---- numbers: decimal digits only ("+" / leading blanks are not numbers), no overflow of `max` --------------------------
RSQC_BAM_FN bool sam_udec(const uint8_t *s, uint32_t len, uint64_t max, uint64_t &v) {
    if (len == 0 || len > 20) return false;
    uint64_t x = 0;
    for (uint32_t i = 0; i < len; ++i) {
        const uint32_t d = (uint32_t)s[i] - '0';
        if (d > 9) return false;
        if (x > (max - d) / 10) return false;
        x = x * 10 + d;
    }
    v = x; return true;
}
RSQC_BAM_FN bool sam_sdec(const uint8_t *s, uint32_t len, int64_t lo, int64_t hi, int64_t &v) {
    const bool neg = len && s[0] == '-';
    uint64_t u;
    if (!sam_udec(s + (neg ? 1 : 0), len - (neg ? 1 : 0), neg ? (uint64_t)(-lo) : (uint64_t)hi, u)) return false;
    v = neg ? -(int64_t)u : (int64_t)u; return true;
}
// FLAG: decimal, or 0x / 0X hexadecimal as htslib reads it
RSQC_BAM_FN bool sam_flag(const uint8_t *s, uint32_t len, uint32_t &flag) {
    uint64_t v;
    if (len > 2 && s[0] == '0' && (s[1] == 'x' || s[1] == 'X')) {
        if (len > 2 + 4) return false;
        v = 0;
        for (uint32_t i = 2; i < len; ++i) {
            const uint32_t c = s[i];
            const uint32_t d = (c >= '0' && c <= '9') ? c - '0' : (c >= 'a' && c <= 'f') ? c - 'a' + 10 : (c >= 'A' && c <= 'F') ? c - 'A' + 10 : 99u;
            if (d > 15) return false;
            v = v * 16 + d;
        }
    } else if (!sam_udec(s, len, 0xFFFF, v)) return false;
    flag = (uint32_t)v; return true;
}

// the BAM code of a CIGAR operator letter, or -1
RSQC_BAM_FN int sam_cigar_code(uint32_t c) {
    switch (c) {
    case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
    case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8;
    default: return -1;
    }
}
// operations of a CIGAR field as the parse will write them: the bytes that are not digits ("*" -> 0)
RSQC_BAM_FN uint32_t sam_count_ops(const uint8_t *s, uint32_t len) {
    if (len == 1 && s[0] == '*') return 0;
    uint32_t n = 0;
    for (uint32_t i = 0; i < len; ++i) n += ((uint32_t)s[i] - '0' > 9u) ? 1u : 0u;
    return n;
}

// ---- fields of a line: f[k] = first byte of field k (k < 11), f[11] = one past the end of QUAL (a tab or the line's end).
// s[0, len) is the line without its '\n' and without a trailing '\r'.  false = fewer than 11 fields.
RSQC_BAM_FN bool sam_fields_bytes(const uint8_t *s, uint32_t len, uint32_t f[12]) {
    uint32_t k = 1; f[0] = 0;
    for (uint32_t i = 0; i < len && k < 12; ++i) if (s[i] == '\t') f[k++] = i + 1;
    if (k < 11) return false;
    if (k == 11) f[11] = len + 1;               // no optional fields
    return true;
}
// the same from a bitmap of the tabs (bit b of word w <-> byte `base + 64 w + b` of the window buffer): the lane hops a 64-byte
// word at a time over SEQ and QUAL.  ls / le: the line's bytes in the window buffer.
RSQC_BAM_FN bool sam_fields_bitmap(const uint64_t *tabs, uint32_t base, uint32_t ls, uint32_t le, uint32_t f[12]) {
    uint32_t k = 1; f[0] = 0;
    uint32_t w = (ls - base) >> 6;
    uint64_t m = tabs[w] & (~0ull << ((ls - base) & 63u));
    for (;;) {
        const uint32_t word_at = base + (w << 6);
        if (word_at >= le) break;
        if (le - word_at < 64u) m &= (1ull << (le - word_at)) - 1ull;
        while (m && k < 12) {
            const uint32_t b = (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            f[k++] = word_at + b + 1 - ls;
        }
        if (k == 12) break;
        m = tabs[++w];
    }
    if (k < 11) return false;
    if (k == 11) f[11] = le - ls + 1;
    return true;
}

// ---- one line -> BamRecOut (+ its operations into cigar_out when not null, at most max_ops of them) ---------------------
// s[0, len): the line without '\n' / trailing '\r'; f: its fields.  Returns SAM_OK or a SAM_ERR_*.
RSQC_BAM_FN uint32_t sam_parse_fields(const uint8_t *s, uint32_t len, const uint32_t f[12], const BamTagSpec &tags, const SamRefTable &refs,
                                      BamRecOut &o, uint32_t *cigar_out, uint32_t max_ops) {
    if (len && s[0] == '@') return SAM_ERR_HEADER;
    auto flen = [&](uint32_t k) { return f[k + 1] - 1 - f[k]; };
    // QNAME: 1-254 bytes (the BAM record's l_read_name is a byte, NUL included), hashed as bam_parse_record hashes it
    const uint32_t qlen = flen(0);
    if (qlen == 0 || qlen > 254) return SAM_ERR_QNAME;
    uint64_t qh = 0xCBF29CE484222325ull;
    uint32_t qh2 = BAM_QH2_SEED;
    for (uint32_t i = 0; i < qlen; ++i) { const uint32_t b = s[i]; qh ^= b; qh *= 0x100000001B3ull; qh2 = bam_qh2_step(qh2, b); }
    qh ^= qh >> 33; qh *= 0xFF51AFD7ED558CCDull; qh ^= qh >> 33; qh *= 0xC4CEB9FE1A85EC53ull; qh ^= qh >> 33;
    uint32_t flag;
    if (!sam_flag(s + f[1], flen(1), flag)) return SAM_ERR_NUMBER;
    // RNAME, POS
    const bool rstar = flen(2) == 1 && s[f[2]] == '*';
    const int32_t found = rstar ? -1 : sam_ref_lookup(refs, s + f[2], flen(2));
    uint64_t u;
    if (!sam_udec(s + f[3], flen(3), 0x7FFFFFFFull, u)) return SAM_ERR_NUMBER;
    const int32_t pos = (int32_t)u - 1;
    int32_t tid;
    sam_place(rstar, found, pos, tid, flag);
    if (!sam_udec(s + f[4], flen(4), 255, u)) return SAM_ERR_NUMBER;
    const uint32_t mapq = (uint32_t)u;
    // CIGAR
    const uint8_t *cg = s + f[5];
    const uint32_t cglen = flen(5);
    uint32_t n_ops = 0; uint64_t qlen_cigar = 0;
    if (!(cglen == 1 && cg[0] == '*')) {
        if (cglen == 0) return SAM_ERR_CIGAR;
        uint64_t x = 0; uint32_t nd = 0;
        for (uint32_t i = 0; i < cglen; ++i) {
            const uint32_t c = cg[i], d = c - '0';
            if (d <= 9) { x = x * 10 + d; if (x >= (1ull << 28)) return SAM_ERR_CIGAR; ++nd; continue; }
            const int code = sam_cigar_code(c);
            if (code < 0 || nd == 0) return SAM_ERR_CIGAR;
            if (cigar_out) { if (n_ops >= max_ops) return SAM_ERR_CIGAR; cigar_out[n_ops] = (uint32_t)(x << 4) | (uint32_t)code; }
            if (code == 0 || code == 1 || code == 4 || code == 7 || code == 8) qlen_cigar += x;
            ++n_ops; x = 0; nd = 0;
        }
        if (nd) return SAM_ERR_CIGAR;                          // digits without an operator
    }
    // RNEXT, PNEXT, TLEN
    int32_t mtid;
    const uint32_t rnlen = flen(6);
    if (rnlen == 1 && s[f[6]] == '=') mtid = tid;
    else if (rnlen == 1 && s[f[6]] == '*') mtid = -1;
    else mtid = sam_ref_lookup(refs, s + f[6], rnlen);
    if (!sam_udec(s + f[7], flen(7), 0x7FFFFFFFull, u)) return SAM_ERR_NUMBER;
    const int32_t mpos = (int32_t)u - 1;
    int64_t isize;
    if (!sam_sdec(s + f[8], flen(8), -0x7FFFFFFFll - 1, 0x7FFFFFFFll, isize)) return SAM_ERR_NUMBER;
    // SEQ, QUAL: lengths only
    const uint32_t sqlen = flen(9), qulen = flen(10);
    if (sqlen == 0 || qulen == 0) return SAM_ERR_FIELDS;
    const bool seq_star = sqlen == 1 && s[f[9]] == '*';
    const int32_t l_seq = seq_star ? 0 : (int32_t)sqlen;
    if (n_ops && !seq_star && qlen_cigar != (uint64_t)l_seq) return SAM_ERR_SEQ_CIGAR;
    if (!(qulen == 1 && s[f[10]] == '*') && qulen != (uint32_t)l_seq) return SAM_ERR_QUAL;
    // optional fields TG:T:value; the last occurrence of a tag decides, as in bam_parse_record
    uint32_t tagbits = (tid == mtid) ? RSQC_TB_MTID_SAME : 0;
    int32_t nm = 0;
    uint64_t umi = tags.umi_src == RSQC_UMI_QNAME ? umi_from_qname(s, qlen, tags.umi_sep) : 0ull;
    bool umi_open = tags.umi_src == RSQC_UMI_TAG;                              // the first field of that name counts, as in bam_parse_record
    for (uint32_t a = f[11]; a < len;) {
        uint32_t b = a;
        while (b < len && s[b] != '\t') ++b;
        const uint32_t fl = b - a;
        if (fl < 5 || s[a + 2] != ':' || s[a + 4] != ':') return SAM_ERR_FIELDS;
        const char t0 = (char)s[a], t1 = (char)s[a + 1], type = (char)s[a + 3];
        const uint8_t *v = s + a + 5; const uint32_t vl = fl - 5;
        int64_t iv = 0;
        const bool is_int = type == 'i';
        if (is_int && !sam_sdec(v, vl, -0x7FFFFFFFll - 1, 0xFFFFFFFFll, iv)) return SAM_ERR_NUMBER;
        if (t0 == 'N' && t1 == 'M') {                          // bam_aux_int: an integer tag only; (uint32 values stored as 'I', read as int32)
            if (is_int) { nm = (int32_t)(uint32_t)(uint64_t)iv; tagbits |= RSQC_TB_HAS_NM; }
        }
        if (tags.have_ch && t0 == (char)tags.ch0 && t1 == (char)tags.ch1) {     // readStringTag: Z, or a non-NUL A
            if (type == 'Z' || (type == 'A' && vl > 0)) tagbits |= RSQC_TB_HAS_CH;
        }
        for (uint32_t fi = 0; fi < tags.n_filter; ++fi)                         // GetTag: Z, integer or float
            if (t0 == (char)tags.f0[fi] && t1 == (char)tags.f1[fi] && (type == 'Z' || type == 'f' || is_int)) tagbits |= (uint32_t)RSQC_TB_FILTER0 << fi;
        if (umi_open && t0 == (char)tags.umi_t0 && t1 == (char)tags.umi_t1) {
            umi_open = false;
            if (type == 'Z') umi = umi_pack(v, vl);
        }
        a = b + 1;
    }
    o.qname_len = qlen; o.qhash2 = bam_qh2_finish(qh2, qlen); o.umi = umi;
    o.core.pos = pos; o.core.mpos = mpos; o.core.isize = (int32_t)isize; o.core.cigar_off = 0;
    o.aux.qhash = qh; o.aux.flag = (uint16_t)flag; o.aux.mapq = (uint8_t)mapq;
    o.tid = tid; o.n_ops = n_ops; o.ops_off = 0;
    const bool wide = l_seq >= RSQC_LQSEQ_ESCAPE || nm >= RSQC_NM_ESCAPE || nm < 0 || n_ops >= RSQC_NCIGAR_ESCAPE;
    o.aux.l_qseq = l_seq >= RSQC_LQSEQ_ESCAPE ? (uint16_t)RSQC_LQSEQ_ESCAPE : (uint16_t)l_seq;
    o.aux.nm = (nm >= RSQC_NM_ESCAPE || nm < 0) ? (uint8_t)RSQC_NM_ESCAPE : (uint8_t)nm;
    o.aux.n_cigar = n_ops >= RSQC_NCIGAR_ESCAPE ? (uint8_t)RSQC_NCIGAR_ESCAPE : (uint8_t)n_ops;
    o.aux.tagbits = (uint8_t)tagbits;
    o.nm = nm; o.l_seq = l_seq; o.wide = wide ? 1u : 0u;
    return SAM_OK;
}
// a whole line (host: tests, and the host side's search for the first malformed line)
RSQC_BAM_FN uint32_t sam_parse_line(const uint8_t *s, uint32_t len, const BamTagSpec &tags, const SamRefTable &refs,
                                    BamRecOut &o, uint32_t *cigar_out, uint32_t max_ops) {
    uint32_t f[12];
    if (len && s[len - 1] == '\r') --len;
    if (len && s[0] == '@') return SAM_ERR_HEADER;
    if (!sam_fields_bytes(s, len, f)) return SAM_ERR_FIELDS;
    return sam_parse_fields(s, len, f, tags, refs, o, cigar_out, max_ops);
}

}  // namespace rsqc
