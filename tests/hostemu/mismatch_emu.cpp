// mismatch_emu.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// The kernel body of --mismatches -- mismatch_block of rnaseqc_amd/csrc/rsqc_mismatch.h, unmodified, with the two record sources the
// kernels of rsqc_mismatch.hip hand it -- compiled for the host on top of the 64-lane fiber emulation of wavemu.h.  What the decode
// stages in front of it leave is restated by window_emu.h over buffers of exactly the window's size.  The reference is packed with
// mismatch_pack_word into words of exactly its size.  The tables are ADDED to, as on the device.  The expected
// tables are NOT computed here: tests/mismatch_ref.py restates the contract in Python and the test compares.
#include "window_emu.h"

#include <string>

#include "../../rnaseqc_amd/csrc/rsqc_mismatch.h"

using namespace rsqc;
using namespace window_emu;

#define EMU_API extern "C" __attribute__((visibility("default")))

namespace {

struct Reference {
    std::vector<std::string> text; std::vector<uint8_t> have;
    std::vector<const char *> seq; std::vector<uint64_t> len64;
    std::vector<uint32_t> words; std::vector<unsigned long long> off, len;
    MismatchPackedRef packed() const { return MismatchPackedRef{words.data(), off.data(), len.data(), (int32_t)off.size()}; }
    MismatchTextRef plain() const { return MismatchTextRef{seq.data(), len64.data(), (int32_t)seq.size()}; }
} g_ref;

Names g_names;

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
EMU_API void mmemu_set_names(int32_t n_ref, const char *const *names) { g_names.set(n_ref, names); }

// A BAM window: `bytes` complete records one behind the other, placed `front` bytes into the window buffer (record starts at every
// alignment).  Returns the records framed, -1: the bytes are no chain of records
EMU_API long long mmemu_bam(const uint8_t *bytes, uint64_t n_bytes, uint32_t front, uint32_t n_blocks, uint32_t min_mapq, uint64_t *cyc, uint64_t *subst, uint64_t *byq,
                            uint64_t *scal) {
    BamWindow B;
    if (!B.frame(bytes, n_bytes, front)) return -1;
    launch(MismatchBamSrc{B.W}, B.sum.n_rec, min_mapq, tables_of(cyc, subst, byq, scal), n_blocks);
    return (long long)B.sum.n_rec;
}

// A SAM window: text of complete lines ('\n'-ended), `front` bytes into the window buffer.  seen: the stream has had a record before
// this window ('@' lines in front are header lines only while it has not).  Returns the record lines, -1: a line the parser refuses
EMU_API long long mmemu_sam(const uint8_t *text, uint64_t n_bytes, uint32_t front, int seen, uint32_t n_blocks, uint32_t min_mapq, uint64_t *cyc, uint64_t *subst,
                            uint64_t *byq, uint64_t *scal) {
    SamParsed P;
    P.frame(text, n_bytes, front, seen, g_names.refs);
    if (!P.parse()) return -1;
    launch(MismatchSamSrc{P.S}, P.n, min_mapq, tables_of(cyc, subst, byq, scal), n_blocks);
    return (long long)P.n;
}

// the one-thread form (what the host reader runs) over the same bytes, against the reference's text: the records of a BAM stream
EMU_API long long mmemu_host_bam(const uint8_t *bytes, uint64_t n_bytes, uint32_t min_mapq, uint64_t *cyc, uint64_t *subst, uint64_t *byq, uint64_t *scal) {
    MismatchCounts C{cyc, subst, byq, {}};
    const MismatchTextRef ref = g_ref.plain();
    const long long n = host_bam_records(bytes, n_bytes, [&](const uint8_t *rec, uint32_t bs) { (void)mismatch_count_bam(rec, bs, ref, min_mapq, C); });
    for (uint32_t k = 0; k < MM_S_WORDS; ++k) scal[k] += C.s[k];
    return n;
}
// ... and the lines of a SAM text without header lines, each parsed by the product's line parser
EMU_API long long mmemu_host_sam(const uint8_t *text, uint64_t n_bytes, uint32_t min_mapq, uint64_t *cyc, uint64_t *subst, uint64_t *byq, uint64_t *scal) {
    MismatchCounts C{cyc, subst, byq, {}};
    const MismatchTextRef ref = g_ref.plain();
    const long long n = host_sam_lines(text, n_bytes, g_names.refs, [&](const uint8_t *line, uint32_t len, const uint32_t *f, const BamRecOut &o, const uint32_t *ops) {
        (void)mismatch_count_sam(line, len, f, o.aux.flag, o.tid, o.core.pos, o.aux.mapq, ops, o.n_ops, ref, min_mapq, C);
    });
    for (uint32_t k = 0; k < MM_S_WORDS; ++k) scal[k] += C.s[k];
    return n;
}
