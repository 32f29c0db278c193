// allele_emu.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// The kernel body of --alleles -- allele_block of rnaseqc_amd/csrc/rsqc_allele.h, unmodified, with the two record sources the kernels of
// rsqc_allele.hip hand it -- compiled for the host on top of the 64-lane fiber emulation of wavemu.h.  What the decode stages in front of
// it leave is restated over buffers of exactly the window's size, as in mismatch_emu.cpp.  The site table is held in vectors of exactly
// its length.  The cells ([site][8]) and the scalar words are ADDED to, as on the device.  The expected table is NOT computed here:
// tests/allele_ref.py restates the contract in Python and the test compares.
#include "wavemu.h"

#include <string>

#include "../../rnaseqc_amd/csrc/rsqc_allele.h"

using namespace rsqc;

#define EMU_API extern "C" __attribute__((visibility("default")))

namespace {

struct Sites {
    std::vector<int32_t> pos; std::vector<uint32_t> first;
    AlleleSites table() const { return AlleleSites{pos.data(), first.data(), (int32_t)first.size() - 1}; }
} g_sites;
bool g_merge = false;                              // which form of allele_block runs

struct Names { std::vector<SamRefSlot> slots; std::vector<uint8_t> names; SamRefTable refs{}; } g_names;

template <class Src> void launch(const Src &src, uint32_t n, uint32_t min_mapq, uint32_t min_baseq, const AlleleTables &T, uint32_t n_blocks) {
    const AlleleSites sites = g_sites.table();
    for (uint32_t b = 0; b < n_blocks; ++b)
        wavemu::run_block((int)AL_THREADS, [&]() { if (g_merge) allele_block<true>(src, n, sites, min_mapq, min_baseq, T, b, n_blocks); else allele_block<false>(src, n, sites, min_mapq, min_baseq, T, b, n_blocks); });
}
AlleleTables tables_of(uint64_t *scal, uint64_t *cells) { return AlleleTables{(unsigned long long *)scal, (unsigned long long *)cells}; }

}  // namespace

EMU_API void alemu_set_merge(int on) { g_merge = on != 0; }
EMU_API void alemu_set_schedule_seed(unsigned long long seed) { wavemu::set_seed(seed); }

// the sites of n_contigs contigs: pos[n_sites] and first[n_contigs + 1], copied into vectors of exactly those lengths
EMU_API void alemu_set_sites(int32_t n_contigs, uint32_t n_sites, const int32_t *pos, const uint32_t *first) {
    g_sites = Sites{};
    g_sites.pos.assign(pos, pos + n_sites); g_sites.pos.shrink_to_fit();
    g_sites.first.assign(first, first + n_contigs + 1);
}

// the RNAME table of a SAM stream (the @SQ names in order)
EMU_API void alemu_set_names(int32_t n_ref, const char *const *names) {
    Names &g = g_names;
    g = Names{};
    uint32_t slots = 16;
    while (slots < 2u * (uint32_t)n_ref) slots <<= 1;
    g.slots.assign(slots, SamRefSlot{0, 0, 0, -1, 0});
    for (int32_t r = 0; r < n_ref; ++r) {
        const uint32_t len = (uint32_t)strlen(names[r]);
        const uint64_t h = bam_qname_hash((const uint8_t *)names[r], len);
        uint32_t k = (uint32_t)h & (slots - 1);
        while (g.slots[k].idx >= 0) k = (k + 1) & (slots - 1);
        g.slots[k] = SamRefSlot{h, (uint32_t)g.names.size(), len, r, 0};
        g.names.insert(g.names.end(), names[r], names[r] + len);
    }
    g.names.push_back(0);
    g.refs = SamRefTable{g.slots.data(), g.names.data(), slots - 1, n_ref};
}

// A BAM window: `bytes` complete records one behind the other, placed `front` bytes into the window buffer (record starts at every
// alignment).  Returns the records framed, -1: the bytes are no chain of records
EMU_API long long alemu_bam(const uint8_t *bytes, uint64_t n_bytes, uint32_t front, uint32_t n_blocks, uint32_t min_mapq, uint32_t min_baseq, uint64_t *scal, uint64_t *cells) {
    std::vector<uint8_t> buf((size_t)front + n_bytes);
    if (n_bytes) memcpy(buf.data() + front, bytes, n_bytes);
    std::vector<uint32_t> rec_off;
    std::vector<rsqc_rec_aux> aux;
    std::vector<rsqc_rec_core> core;
    for (uint64_t p = front; p < buf.size();) {
        if (p + 4 > buf.size()) return -1;
        const uint32_t bs = bam_ld32(buf.data() + p);
        if (bs < 32 || p + 4 + (uint64_t)bs > buf.size()) return -1;
        rsqc_rec_aux a{};
        rsqc_rec_core c{};
        a.flag = (uint16_t)bam_ld16(buf.data() + p + 4 + 14); a.mapq = buf[p + 4 + 9];          // (the parse stage's columns)
        c.pos = (int32_t)bam_ld32(buf.data() + p + 4 + 4);
        rec_off.push_back((uint32_t)p); aux.push_back(a); core.push_back(c);
        p += 4 + (uint64_t)bs;
    }
    DecodeSummary sum{};
    sum.n_rec = (uint32_t)rec_off.size();
    MismatchBamSrc src{};
    src.W.buf = buf.data(); src.W.start = front; src.W.end = (uint32_t)buf.size();
    src.W.rec_off = rec_off.data(); src.W.aux = aux.data(); src.W.core = core.data(); src.W.sum = &sum;
    launch(src, sum.n_rec, min_mapq, min_baseq, tables_of(scal, cells), n_blocks);
    return (long long)rec_off.size();
}

// A SAM window: text of complete lines ('\n'-ended), `front` bytes into the window buffer.  seen: the stream has had a record before
// this window ('@' lines in front are header lines only while it has not).  Returns the record lines, -1: a line the parser refuses
EMU_API long long alemu_sam(const uint8_t *text, uint64_t n_bytes, uint32_t front, int seen, uint32_t n_blocks, uint32_t min_mapq, uint32_t min_baseq, uint64_t *scal, uint64_t *cells) {
    SamWindow S{};
    S.base = front & ~63u;
    const uint32_t end = front + (uint32_t)n_bytes;
    S.n_words = (end - S.base + 63u) / 64u;
    std::vector<uint8_t> buf((size_t)S.base + (size_t)S.n_words * 64u, 0);          // (the bitmap stage loads whole words)
    if (n_bytes) memcpy(buf.data() + front, text, n_bytes);
    std::vector<uint64_t> ebits(S.n_words + 1, 0), tbits(S.n_words + 1, 0);
    S.W.buf = buf.data(); S.W.start = front; S.W.end = end;
    S.ebits = ebits.data(); S.tbits = tbits.data();
    S.refs = g_names.refs; S.W.tags.n_ref = g_names.refs.n_ref;
    uint32_t n_lines = 0;
    for (uint32_t w = 0; w < S.n_words; ++w) n_lines += sam_bitmap_word(S, w).rec;
    std::vector<uint32_t> rec_off((size_t)n_lines + 1, 0);
    S.W.rec_off = rec_off.data(); S.rec_cap = n_lines;
    SamStatus st{};
    S.st = &st;
    for (uint32_t w = 0, k = 0; w < S.n_words; ++w) { sam_lines_word(S, w, k); k += (uint32_t)__builtin_popcountll(ebits[w]); }
    uint32_t hdr = 0;
    if (!seen) while (hdr < n_lines && sam_is_header_line(S, hdr)) ++hdr;
    st.hdr = hdr; st.n_lines = n_lines;
    const uint32_t n = n_lines - hdr;
    std::vector<rsqc_rec_aux> aux((size_t)n + 1);
    std::vector<rsqc_rec_core> core((size_t)n + 1);
    std::vector<uint32_t> qh2((size_t)n + 1), nops((size_t)n + 1), ops_at((size_t)n + 1);
    std::vector<int32_t> rtid((size_t)n + 1);
    S.W.aux = aux.data(); S.W.core = core.data(); S.W.qh2 = qh2.data(); S.W.ops_at = ops_at.data(); S.nops = nops.data(); S.rtid = rtid.data();
    uint32_t total = 0;
    for (uint32_t j = 0; j < n; ++j) { nops[j] = sam_fields_one(S, j); ops_at[j] = total; total += nops[j]; }
    std::vector<uint32_t> cigar((size_t)total);                                     // (exactly the operations: one more read is an overflow)
    S.W.cigar = cigar.data(); S.cigar_cap = total;
    for (uint32_t j = 0; j < n; ++j) if (sam_parse_one(S, j) != SAM_OK) return -1;
    DecodeSummary sum{};
    sum.n_rec = n; sum.n_ops = total;
    S.W.sum = &sum;
    MismatchSamSrc src{S};
    launch(src, n, min_mapq, min_baseq, tables_of(scal, cells), n_blocks);
    return (long long)n;
}

// the one-thread form (what the host reader runs) over the same bytes, into a [site][7] table: the records of a BAM stream
EMU_API long long alemu_host_bam(const uint8_t *bytes, uint64_t n_bytes, uint32_t min_mapq, uint32_t min_baseq, uint64_t *scal, uint64_t *counts) {
    AlleleCounts<AlleleHostCells> C{AlleleHostCells{counts}, {}};
    const AlleleSites sites = g_sites.table();
    long long n = 0;
    for (uint64_t p = 0; p + 4 <= n_bytes; ++n) {
        const uint32_t bs = bam_ld32(bytes + p);
        if (bs < 32 || p + 4 + (uint64_t)bs > n_bytes) return -1;
        (void)allele_count_bam(bytes + p, bs, sites, min_mapq, min_baseq, C);
        p += 4 + (uint64_t)bs;
    }
    for (uint32_t k = 0; k < AL_S_WORDS; ++k) scal[k] += C.s[k];
    return n;
}
// ... and the lines of a SAM text without header lines, each parsed by the product's line parser
EMU_API long long alemu_host_sam(const uint8_t *text, uint64_t n_bytes, uint32_t min_mapq, uint32_t min_baseq, uint64_t *scal, uint64_t *counts) {
    AlleleCounts<AlleleHostCells> C{AlleleHostCells{counts}, {}};
    const AlleleSites sites = g_sites.table();
    BamTagSpec tags{};
    tags.n_ref = g_names.refs.n_ref;
    long long n = 0;
    for (uint64_t p = 0; p < n_bytes; ++n) {
        uint64_t e = p;
        while (e < n_bytes && text[e] != '\n') ++e;
        std::vector<uint8_t> line(text + p, text + e);                                // (exactly the line)
        std::vector<uint32_t> ops(sam_count_ops(line.data(), (uint32_t)line.size()) + 1u);
        BamRecOut o;
        uint32_t f[12];
        if (!sam_fields_bytes(line.data(), (uint32_t)line.size(), f) || sam_parse_fields(line.data(), (uint32_t)line.size(), f, tags, g_names.refs, o, ops.data(), (uint32_t)ops.size()) != SAM_OK) return -1;
        (void)allele_count_sam(line.data(), (uint32_t)line.size(), f, o.aux.flag, o.tid, o.core.pos, o.aux.mapq, ops.data(), o.n_ops, sites, min_mapq, min_baseq, C);
        p = e + 1;
    }
    for (uint32_t k = 0; k < AL_S_WORDS; ++k) scal[k] += C.s[k];
    return n;
}
