// mismatch_emu.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// The kernel body of --mismatches -- mismatch_block of rnaseqc_amd/csrc/rsqc_mismatch.h, unmodified, with the two record sources the
// kernels of rsqc_mismatch.hip hand it -- compiled for the host on top of the 64-lane fiber emulation of wavemu.h.  What the decode
// stages in front of it leave is restated over buffers of exactly the window's size: for a BAM window the record offsets and the flag,
// mapq and pos columns; for a SAM window the product's own bitmap, line and parse steps (rsqc_sam.h) run one record after the other.  The
// reference is packed with mismatch_pack_word into words of exactly its size.  The tables are ADDED to, as on the device.  The expected
// tables are NOT computed here: tests/mismatch_ref.py restates the contract in Python and the test compares.
#include "wavemu.h"

#include <string>

#include "../../rnaseqc_amd/csrc/rsqc_mismatch.h"

using namespace rsqc;

#define EMU_API extern "C" __attribute__((visibility("default")))

namespace {

struct Reference {
    std::vector<std::string> text; std::vector<uint8_t> have;
    std::vector<const char *> seq; std::vector<uint64_t> len64;
    std::vector<uint32_t> words; std::vector<unsigned long long> off, len;
    MismatchPackedRef packed() const { return MismatchPackedRef{words.data(), off.data(), len.data(), (int32_t)off.size()}; }
    MismatchTextRef plain() const { return MismatchTextRef{seq.data(), len64.data(), (int32_t)seq.size()}; }
} g_ref;

struct Names { std::vector<SamRefSlot> slots; std::vector<uint8_t> names; SamRefTable refs{}; } g_names;

template <class Src> void launch(const Src &src, uint32_t n, uint32_t min_mapq, const MismatchTables &T, uint32_t n_blocks) {
    const MismatchPackedRef ref = g_ref.packed();
    for (uint32_t b = 0; b < n_blocks; ++b) wavemu::run_block((int)MM_THREADS, [&]() { mismatch_block(src, n, ref, min_mapq, T, b, n_blocks); });
}
MismatchTables tables_of(uint64_t *cyc, uint64_t *subst, uint64_t *byq, uint64_t *scal) {
    return MismatchTables{(unsigned long long *)cyc, (unsigned long long *)subst, (unsigned long long *)byq, (unsigned long long *)scal};
}

}  // namespace

EMU_API void mmemu_set_schedule_seed(unsigned long long seed) { wavemu::set_seed(seed); }

// n contigs; sequence[i] NULL: the FASTA lacks it
EMU_API void mmemu_set_reference(int32_t n, const uint64_t *length, const char *const *sequence) {
    g_ref = Reference{};
    for (int32_t i = 0; i < n; ++i) {
        g_ref.have.push_back(sequence[i] ? 1 : 0);
        g_ref.text.emplace_back(sequence[i] ? std::string(sequence[i], (size_t)length[i]) : std::string());
        g_ref.len.push_back(length[i]); g_ref.len64.push_back(length[i]);
        g_ref.off.push_back(sequence[i] ? (unsigned long long)g_ref.words.size() : ~0ull);
        if (!sequence[i]) continue;
        std::vector<uint8_t> exact(sequence[i], sequence[i] + length[i]);                          // (a read behind the contig's end is a heap overflow)
        for (uint64_t w = 0; w < (length[i] + 7) / 8; ++w) g_ref.words.push_back(mismatch_pack_word(exact.data(), length[i], w));
    }
    for (int32_t i = 0; i < n; ++i) g_ref.seq.push_back(g_ref.have[(size_t)i] ? g_ref.text[(size_t)i].data() : nullptr);
}

// the reference code of every byte value, through the packed word and its accessor
EMU_API void mmemu_pack_codes(uint32_t *code) {
    uint8_t all[256];
    for (uint32_t v = 0; v < 256u; ++v) all[v] = (uint8_t)v;
    uint32_t words[32];
    for (uint32_t w = 0; w < 32u; ++w) words[w] = mismatch_pack_word(all, 256, w);
    const MismatchPackedRef::Contig ct{words, 256};
    for (uint32_t v = 0; v < 256u; ++v) code[v] = ct.code(v);
}

// the RNAME table of a SAM stream (the @SQ names in order)
EMU_API void mmemu_set_names(int32_t n_ref, const char *const *names) {
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
EMU_API long long mmemu_bam(const uint8_t *bytes, uint64_t n_bytes, uint32_t front, uint32_t n_blocks, uint32_t min_mapq, uint64_t *cyc, uint64_t *subst, uint64_t *byq,
                            uint64_t *scal) {
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
    launch(src, sum.n_rec, min_mapq, tables_of(cyc, subst, byq, scal), n_blocks);
    return (long long)rec_off.size();
}

// A SAM window: text of complete lines ('\n'-ended), `front` bytes into the window buffer.  seen: the stream has had a record before
// this window ('@' lines in front are header lines only while it has not).  Returns the record lines, -1: a line the parser refuses
EMU_API long long mmemu_sam(const uint8_t *text, uint64_t n_bytes, uint32_t front, int seen, uint32_t n_blocks, uint32_t min_mapq, uint64_t *cyc, uint64_t *subst,
                            uint64_t *byq, uint64_t *scal) {
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
    launch(src, n, min_mapq, tables_of(cyc, subst, byq, scal), n_blocks);
    return (long long)n;
}

// the one-thread form (what the host reader runs) over the same bytes, against the reference's text: the records of a BAM stream
EMU_API long long mmemu_host_bam(const uint8_t *bytes, uint64_t n_bytes, uint32_t min_mapq, uint64_t *cyc, uint64_t *subst, uint64_t *byq, uint64_t *scal) {
    MismatchCounts C{cyc, subst, byq, {}};
    const MismatchTextRef ref = g_ref.plain();
    long long n = 0;
    for (uint64_t p = 0; p + 4 <= n_bytes; ++n) {
        const uint32_t bs = bam_ld32(bytes + p);
        if (bs < 32 || p + 4 + (uint64_t)bs > n_bytes) return -1;
        (void)mismatch_count_bam(bytes + p, bs, ref, min_mapq, C);
        p += 4 + (uint64_t)bs;
    }
    for (uint32_t k = 0; k < MM_S_WORDS; ++k) scal[k] += C.s[k];
    return n;
}
// ... and the lines of a SAM text without header lines, each parsed by the product's line parser
EMU_API long long mmemu_host_sam(const uint8_t *text, uint64_t n_bytes, uint32_t min_mapq, uint64_t *cyc, uint64_t *subst, uint64_t *byq, uint64_t *scal) {
    MismatchCounts C{cyc, subst, byq, {}};
    const MismatchTextRef ref = g_ref.plain();
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
        (void)mismatch_count_sam(line.data(), (uint32_t)line.size(), f, o.aux.flag, o.tid, o.core.pos, o.aux.mapq, ops.data(), o.n_ops, ref, min_mapq, C);
        p = e + 1;
    }
    for (uint32_t k = 0; k < MM_S_WORDS; ++k) scal[k] += C.s[k];
    return n;
}
