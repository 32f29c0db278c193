// cycle_emu.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// The kernel body of --cycles -- cycle_block of rnaseqc_amd/csrc/rsqc_cycle.h, unmodified, with the two record sources the kernels of
// rsqc_cycle.hip hand it -- compiled for the host on top of the 64-lane fiber emulation of wavemu.h.  What the decode stages in front
// of it leave is restated by window_emu.h over buffers of exactly the window's size; of a SAM window the stage reads the flag and the
// length column only, and this harness has no RNAME table for the full parse, so the two are filled by hand.  The tables are ADDED to, as on the device: a stream is emulated window by window into the same arrays.  The
// expected tables are NOT computed here: tests/cycle_ref.py restates the contract in Python and the test compares.
#include "window_emu.h"

#include <string>

#include "../../rnaseqc_amd/csrc/rsqc_cycle.h"

using namespace rsqc;
using namespace window_emu;

#define EMU_API extern "C" __attribute__((visibility("default")))

namespace {

template <class Src> void launch(const Src &src, uint32_t n, const CycleTables &T, uint32_t n_blocks) {
    for (uint32_t tile = 0; tile < CYC_TILES; ++tile)
        for (uint32_t b = 0; b < n_blocks; ++b)
            wavemu::run_block((int)CYC_THREADS, [&]() { cycle_block(src, n, T, tile, b, n_blocks); });
}
CycleTables tables_of(uint64_t *base, uint64_t *qual, uint64_t *scal) {
    return CycleTables{(unsigned long long *)base, (unsigned long long *)qual, (unsigned long long *)scal};
}

}  // namespace

EMU_API void cycemu_set_schedule_seed(unsigned long long seed) { wavemu::set_seed(seed); }

// A BAM window: `bytes` complete records one behind the other, placed `front` bytes into the window buffer (record starts at every
// alignment).  Returns the records framed, -1: the bytes are no chain of records
EMU_API long long cycemu_bam(const uint8_t *bytes, uint64_t n_bytes, uint32_t front, uint32_t n_blocks, uint64_t *base, uint64_t *qual, uint64_t *scal) {
    BamWindow B;
    if (!B.frame(bytes, n_bytes, front)) return -1;
    launch(CycleBamSrc{B.W}, B.sum.n_rec, tables_of(base, qual, scal), n_blocks);
    return (long long)B.sum.n_rec;
}

// A SAM window: text of complete lines ('\n'-ended), `front` bytes into the window buffer.  seen: the stream has had a record before
// this window ('@' lines in front are header lines only while it has not).  Returns the record lines, -1: a line without 11 fields
EMU_API long long cycemu_sam(const uint8_t *text, uint64_t n_bytes, uint32_t front, int seen, uint32_t n_blocks, uint64_t *base, uint64_t *qual, uint64_t *scal) {
    SamLines T;
    T.frame(text, n_bytes, front, seen, SamRefTable{});
    const SamWindow &S = T.S;
    const std::vector<uint8_t> &buf = T.buf;
    const uint32_t n = T.n;
    std::vector<rsqc_rec_aux> aux((size_t)n + 1);
    for (uint32_t j = 0; j < n; ++j) {
        uint32_t ls, le, f[12];
        sam_line_bounds(S, T.st.hdr + j, ls, le);
        if (!sam_fields_bitmap(S.tbits, S.base, ls, le, f)) return -1;
        uint32_t flag = 0;
        for (uint32_t p = ls + f[1]; p < ls + f[2] - 1u; ++p) flag = flag * 10u + (uint32_t)(buf[p] - '0');
        const uint32_t sqlen = f[10] - 1u - f[9], l_seq = (sqlen == 1u && buf[ls + f[9]] == '*') ? 0u : sqlen;
        aux[j] = rsqc_rec_aux{};
        aux[j].flag = (uint16_t)flag;
        aux[j].l_qseq = l_seq >= RSQC_LQSEQ_ESCAPE ? (uint16_t)RSQC_LQSEQ_ESCAPE : (uint16_t)l_seq;
    }
    T.S.W.aux = aux.data();
    launch(CycleSamSrc{T.S}, n, tables_of(base, qual, scal), n_blocks);
    return (long long)n;
}

// the one-thread form (what the host reader runs) over the same bytes: the records of a BAM stream
EMU_API long long cycemu_host_bam(const uint8_t *bytes, uint64_t n_bytes, uint64_t *base, uint64_t *qual, uint64_t *scal) {
    CycleCounts C{base, qual, {0, 0, 0, 0, 0, 0, 0, 0}};
    const long long n = host_bam_records(bytes, n_bytes, [&](const uint8_t *rec, uint32_t bs) { (void)cycle_count_bam(rec, bs, C); });
    for (uint32_t k = 0; k < CYC_S_WORDS; ++k) scal[k] += C.s[k];
    return n;
}
