// allele_emu.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// The kernel body of --alleles -- allele_block of rnaseqc_amd/csrc/rsqc_allele.h, unmodified, with the two record sources the kernels of
// rsqc_allele.hip hand it -- compiled for the host on top of the 64-lane fiber emulation of wavemu.h.  What the decode stages in front of
// it leave is restated by window_emu.h over buffers of exactly the window's size.  The site table is held in vectors of exactly
// its length.  The cells ([site][8]) and the scalar words are ADDED to, as on the device.  The expected table is NOT computed here:
// tests/allele_ref.py restates the contract in Python and the test compares.
#include "window_emu.h"

#include <string>

#include "../../rnaseqc_amd/csrc/rsqc_allele.h"

using namespace rsqc;
using namespace window_emu;

#define EMU_API extern "C" __attribute__((visibility("default")))

namespace {

struct Sites {
    std::vector<int32_t> pos; std::vector<uint32_t> first;
    AlleleSites table() const { return AlleleSites{pos.data(), first.data(), (int32_t)first.size() - 1}; }
} g_sites;
bool g_merge = false;                              // which form of allele_block runs

Names g_names;

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
EMU_API void alemu_set_names(int32_t n_ref, const char *const *names) { g_names.set(n_ref, names); }

// A BAM window: `bytes` complete records one behind the other, placed `front` bytes into the window buffer (record starts at every
// alignment).  Returns the records framed, -1: the bytes are no chain of records
EMU_API long long alemu_bam(const uint8_t *bytes, uint64_t n_bytes, uint32_t front, uint32_t n_blocks, uint32_t min_mapq, uint32_t min_baseq, uint64_t *scal, uint64_t *cells) {
    BamWindow B;
    if (!B.frame(bytes, n_bytes, front)) return -1;
    launch(MismatchBamSrc{B.W}, B.sum.n_rec, min_mapq, min_baseq, tables_of(scal, cells), n_blocks);
    return (long long)B.sum.n_rec;
}

// A SAM window: text of complete lines ('\n'-ended), `front` bytes into the window buffer.  seen: the stream has had a record before
// this window ('@' lines in front are header lines only while it has not).  Returns the record lines, -1: a line the parser refuses
EMU_API long long alemu_sam(const uint8_t *text, uint64_t n_bytes, uint32_t front, int seen, uint32_t n_blocks, uint32_t min_mapq, uint32_t min_baseq, uint64_t *scal, uint64_t *cells) {
    SamParsed P;
    P.frame(text, n_bytes, front, seen, g_names.refs);
    if (!P.parse()) return -1;
    launch(MismatchSamSrc{P.S}, P.n, min_mapq, min_baseq, tables_of(scal, cells), n_blocks);
    return (long long)P.n;
}

// the one-thread form (what the host reader runs) over the same bytes, into a [site][7] table: the records of a BAM stream
EMU_API long long alemu_host_bam(const uint8_t *bytes, uint64_t n_bytes, uint32_t min_mapq, uint32_t min_baseq, uint64_t *scal, uint64_t *counts) {
    AlleleCounts<AlleleHostCells> C{AlleleHostCells{counts}, {}};
    const AlleleSites sites = g_sites.table();
    const long long n = host_bam_records(bytes, n_bytes, [&](const uint8_t *rec, uint32_t bs) { (void)allele_count_bam(rec, bs, sites, min_mapq, min_baseq, C); });
    for (uint32_t k = 0; k < AL_S_WORDS; ++k) scal[k] += C.s[k];
    return n;
}
// ... and the lines of a SAM text without header lines, each parsed by the product's line parser
EMU_API long long alemu_host_sam(const uint8_t *text, uint64_t n_bytes, uint32_t min_mapq, uint32_t min_baseq, uint64_t *scal, uint64_t *counts) {
    AlleleCounts<AlleleHostCells> C{AlleleHostCells{counts}, {}};
    const AlleleSites sites = g_sites.table();
    const long long n = host_sam_lines(text, n_bytes, g_names.refs, [&](const uint8_t *line, uint32_t len, const uint32_t *f, const BamRecOut &o, const uint32_t *ops) {
        (void)allele_count_sam(line, len, f, o.aux.flag, o.tid, o.core.pos, o.aux.mapq, ops, o.n_ops, sites, min_mapq, min_baseq, C);
    });
    for (uint32_t k = 0; k < AL_S_WORDS; ++k) scal[k] += C.s[k];
    return n;
}
