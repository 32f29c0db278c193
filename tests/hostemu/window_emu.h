// window_emu.h -- TEST HARNESS ONLY: what cycle_emu.cpp, mismatch_emu.cpp and allele_emu.cpp restate of the decode in front of their
// kernel bodies, over buffers of exactly the window's size (a read outside one is a heap overflow under the sanitizers):
//   BamWindow   a BAM window as the decode leaves it: the record offsets, the flag, mapq and l_qseq columns, core.pos, the summary
//   SamLines    a SAM window's bitmap words, line ends and header count, from the product's own steps (rsqc_sam.h)
//   SamParsed   ... and its parse columns, the operations in an arena of exactly their number
//   Names       the RNAME table of a SAM stream
//   host_bam_records / host_sam_lines   the records the one-thread forms are handed, one after the other
// The windows hold pointers into their own vectors: they are filled once and neither copied nor moved.
#pragma once
#include "wavemu.h"

#include "../../rnaseqc_amd/csrc/rsqc_cycle.h"

namespace window_emu {

using namespace rsqc;

// `bytes` complete records one behind the other, placed `front` bytes into the window buffer (record starts at every alignment)
struct BamWindow {
    std::vector<uint8_t> buf;
    std::vector<uint32_t> rec_off;
    std::vector<rsqc_rec_aux> aux;
    std::vector<rsqc_rec_core> core;
    DecodeSummary sum{};
    DecodeWindow W{};
    // false: the bytes are no chain of records
    bool frame(const uint8_t *bytes, uint64_t n_bytes, uint32_t front) {
        buf.resize((size_t)front + n_bytes);
        if (n_bytes) memcpy(buf.data() + front, bytes, n_bytes);
        for (uint64_t p = front; p < buf.size();) {
            if (p + 4 > buf.size()) return false;
            const uint8_t *rec = buf.data() + p;
            const uint32_t bs = bam_ld32(rec);
            if (bs < 32 || p + 4 + (uint64_t)bs > buf.size()) return false;
            rsqc_rec_aux a{};
            rsqc_rec_core c{};
            a.flag = (uint16_t)bam_ld16(rec + 4 + 14); a.mapq = rec[4 + 9];                   // (the parse stage's columns)
            const int32_t l_seq = (int32_t)bam_ld32(rec + 4 + 16);
            a.l_qseq = (l_seq >= RSQC_LQSEQ_ESCAPE || l_seq < 0) ? (uint16_t)RSQC_LQSEQ_ESCAPE : (uint16_t)l_seq;
            c.pos = (int32_t)bam_ld32(rec + 4 + 4);
            rec_off.push_back((uint32_t)p); aux.push_back(a); core.push_back(c);
            p += 4 + (uint64_t)bs;
        }
        sum.n_rec = (uint32_t)rec_off.size();
        W.buf = buf.data(); W.start = front; W.end = (uint32_t)buf.size();
        W.rec_off = rec_off.data(); W.aux = aux.data(); W.core = core.data(); W.sum = &sum;
        return true;
    }
};

struct Names {
    std::vector<SamRefSlot> slots; std::vector<uint8_t> names; SamRefTable refs{};
    // the @SQ names in order
    void set(int32_t n_ref, const char *const *name) {
        slots.clear(); names.clear();
        uint32_t n_slots = 16;
        while (n_slots < 2u * (uint32_t)n_ref) n_slots <<= 1;
        slots.assign(n_slots, SamRefSlot{0, 0, 0, -1, 0});
        for (int32_t r = 0; r < n_ref; ++r) {
            const uint32_t len = (uint32_t)strlen(name[r]);
            const uint64_t h = bam_qname_hash((const uint8_t *)name[r], len);
            uint32_t k = (uint32_t)h & (n_slots - 1);
            while (slots[k].idx >= 0) k = (k + 1) & (n_slots - 1);
            slots[k] = SamRefSlot{h, (uint32_t)names.size(), len, r, 0};
            names.insert(names.end(), name[r], name[r] + len);
        }
        names.push_back(0);
        refs = SamRefTable{slots.data(), names.data(), n_slots - 1, n_ref};
    }
};

// text of complete lines ('\n'-ended), `front` bytes into the window buffer.  seen: the stream has had a record before this window ('@'
// lines in front are header lines only while it has not).  n: the record lines; the caller hands S.W the columns its source reads
struct SamLines {
    SamWindow S{};
    std::vector<uint8_t> buf;
    std::vector<uint64_t> ebits, tbits;
    std::vector<uint32_t> rec_off;
    SamStatus st{};
    DecodeSummary sum{};
    uint32_t n = 0;
    void frame(const uint8_t *text, uint64_t n_bytes, uint32_t front, int seen, const SamRefTable &refs) {
        S.base = front & ~63u;
        const uint32_t end = front + (uint32_t)n_bytes;
        S.n_words = (end - S.base + 63u) / 64u;
        buf.assign((size_t)S.base + (size_t)S.n_words * 64u, 0);                        // (the bitmap stage loads whole words)
        if (n_bytes) memcpy(buf.data() + front, text, n_bytes);
        ebits.assign(S.n_words + 1, 0); tbits.assign(S.n_words + 1, 0);
        S.W.buf = buf.data(); S.W.start = front; S.W.end = end;
        S.ebits = ebits.data(); S.tbits = tbits.data();
        S.refs = refs; S.W.tags.n_ref = refs.n_ref;
        uint32_t n_lines = 0;
        for (uint32_t w = 0; w < S.n_words; ++w) n_lines += sam_bitmap_word(S, w).rec;
        rec_off.assign((size_t)n_lines + 1, 0);
        S.W.rec_off = rec_off.data(); S.rec_cap = n_lines;
        S.st = &st;
        for (uint32_t w = 0, k = 0; w < S.n_words; ++w) { sam_lines_word(S, w, k); k += (uint32_t)__builtin_popcountll(ebits[w]); }
        uint32_t hdr = 0;
        if (!seen) while (hdr < n_lines && sam_is_header_line(S, hdr)) ++hdr;
        st.hdr = hdr; st.n_lines = n_lines;
        n = n_lines - hdr;
        sum.n_rec = n;
        S.W.sum = &sum;
    }
};

struct SamParsed : SamLines {
    std::vector<rsqc_rec_aux> aux;
    std::vector<rsqc_rec_core> core;
    std::vector<uint32_t> qh2, nops, ops_at, cigar;
    std::vector<int32_t> rtid;
    // (behind frame) false: a line the parser refuses
    bool parse() {
        aux.resize((size_t)n + 1); core.resize((size_t)n + 1);
        qh2.resize((size_t)n + 1); nops.resize((size_t)n + 1); ops_at.resize((size_t)n + 1); rtid.resize((size_t)n + 1);
        S.W.aux = aux.data(); S.W.core = core.data(); S.W.qh2 = qh2.data(); S.W.ops_at = ops_at.data(); S.nops = nops.data(); S.rtid = rtid.data();
        uint32_t total = 0;
        for (uint32_t j = 0; j < n; ++j) { nops[j] = sam_fields_one(S, j); ops_at[j] = total; total += nops[j]; }
        cigar.resize((size_t)total);                                                    // (exactly the operations: one more read is an overflow)
        S.W.cigar = cigar.data(); S.cigar_cap = total;
        for (uint32_t j = 0; j < n; ++j) if (sam_parse_one(S, j) != SAM_OK) return false;
        sum.n_ops = total;
        return true;
    }
};

// the records of a BAM stream: f(rec, block_size).  Returns their number, -1: the bytes are no chain of records
template <class F> long long host_bam_records(const uint8_t *bytes, uint64_t n_bytes, F f) {
    long long n = 0;
    for (uint64_t p = 0; p + 4 <= n_bytes; ++n) {
        const uint32_t bs = bam_ld32(bytes + p);
        if (bs < 32 || p + 4 + (uint64_t)bs > n_bytes) return -1;
        f(bytes + p, bs);
        p += 4 + (uint64_t)bs;
    }
    return n;
}
// the lines of a SAM text without header lines, each in a buffer of exactly the line and parsed by the product's line parser:
// f(line, length, fields, the parsed record, its operations).  Returns their number, -1: a line the parser refuses
template <class F> long long host_sam_lines(const uint8_t *text, uint64_t n_bytes, const SamRefTable &refs, F f) {
    BamTagSpec tags{};
    tags.n_ref = refs.n_ref;
    long long n = 0;
    for (uint64_t p = 0; p < n_bytes; ++n) {
        uint64_t e = p;
        while (e < n_bytes && text[e] != '\n') ++e;
        std::vector<uint8_t> line(text + p, text + e);
        std::vector<uint32_t> ops(sam_count_ops(line.data(), (uint32_t)line.size()) + 1u);
        BamRecOut o;
        uint32_t fields[12];
        if (!sam_fields_bytes(line.data(), (uint32_t)line.size(), fields) ||
            sam_parse_fields(line.data(), (uint32_t)line.size(), fields, tags, refs, o, ops.data(), (uint32_t)ops.size()) != SAM_OK) return -1;
        f(line.data(), (uint32_t)line.size(), fields, o, ops.data());
        p = e + 1;
    }
    return n;
}

}  // namespace window_emu
