// cycle_emu.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// The kernel body of --cycles -- cycle_block of rnaseqc_amd/csrc/rsqc_cycle.h, unmodified, with the two record sources the kernels of
// rsqc_cycle.hip hand it -- compiled for the host on top of the 64-lane fiber emulation of wavemu.h.  What the decode stages in front
// of it leave (the record offsets and the flag column of a BAM window; the line ends, the tab bitmap, the header count and the flag
// column of a SAM window) is restated with plain code over buffers of exactly the window's size: a read outside one is a heap overflow
// under the sanitizers.  The tables are ADDED to, as on the device: a stream is emulated window by window into the same arrays.  The
// expected tables are NOT computed here: tests/cycle_ref.py restates the contract in Python and the test compares.
#include "wavemu.h"

#include <string>

#include "../../rnaseqc_amd/csrc/rsqc_cycle.h"

using namespace rsqc;

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
    std::vector<uint8_t> buf((size_t)front + n_bytes);
    if (n_bytes) memcpy(buf.data() + front, bytes, n_bytes);
    std::vector<uint32_t> rec_off;
    std::vector<rsqc_rec_aux> aux;
    for (uint64_t p = front; p < buf.size();) {
        if (p + 4 > buf.size()) return -1;
        const uint32_t bs = bam_ld32(buf.data() + p);
        if (bs < 32 || p + 4 + (uint64_t)bs > buf.size()) return -1;
        rsqc_rec_aux a{};
        a.flag = (uint16_t)bam_ld16(buf.data() + p + 4 + 14);
        const int32_t l_seq = (int32_t)bam_ld32(buf.data() + p + 4 + 16);                   // (the parse stage's length column)
        a.l_qseq = (l_seq >= RSQC_LQSEQ_ESCAPE || l_seq < 0) ? (uint16_t)RSQC_LQSEQ_ESCAPE : (uint16_t)l_seq;
        rec_off.push_back((uint32_t)p); aux.push_back(a);
        p += 4 + (uint64_t)bs;
    }
    DecodeSummary sum{};
    sum.n_rec = (uint32_t)rec_off.size();
    CycleBamSrc src{};
    src.W.buf = buf.data(); src.W.start = front; src.W.end = (uint32_t)buf.size();
    src.W.rec_off = rec_off.data(); src.W.aux = aux.data(); src.W.sum = &sum;
    launch(src, sum.n_rec, tables_of(base, qual, scal), n_blocks);
    return (long long)rec_off.size();
}

// A SAM window: text of complete lines ('\n'-ended), `front` bytes into the window buffer.  seen: the stream has had a record before
// this window ('@' lines in front are header lines only while it has not).  Returns the record lines, -1: a line without 11 fields
EMU_API long long cycemu_sam(const uint8_t *text, uint64_t n_bytes, uint32_t front, int seen, uint32_t n_blocks, uint64_t *base, uint64_t *qual, uint64_t *scal) {
    SamWindow S{};
    S.base = front & ~63u;
    const uint32_t end = front + (uint32_t)n_bytes;
    S.n_words = (end - S.base + 63u) / 64u;
    std::vector<uint8_t> buf((size_t)S.base + (size_t)S.n_words * 64u, 0);          // (the bitmap stage loads whole words)
    if (n_bytes) memcpy(buf.data() + front, text, n_bytes);
    std::vector<uint64_t> ebits(S.n_words + 1, 0), tbits(S.n_words + 1, 0);
    S.W.buf = buf.data(); S.W.start = front; S.W.end = end;
    S.ebits = ebits.data(); S.tbits = tbits.data();
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
    for (uint32_t j = 0; j < n; ++j) {
        uint32_t ls, le, f[12];
        sam_line_bounds(S, hdr + j, ls, le);
        if (!sam_fields_bitmap(S.tbits, S.base, ls, le, f)) return -1;
        uint32_t flag = 0;
        for (uint32_t p = ls + f[1]; p < ls + f[2] - 1u; ++p) flag = flag * 10u + (uint32_t)(buf[p] - '0');
        const uint32_t sqlen = f[10] - 1u - f[9], l_seq = (sqlen == 1u && buf[ls + f[9]] == '*') ? 0u : sqlen;
        aux[j] = rsqc_rec_aux{};
        aux[j].flag = (uint16_t)flag;
        aux[j].l_qseq = l_seq >= RSQC_LQSEQ_ESCAPE ? (uint16_t)RSQC_LQSEQ_ESCAPE : (uint16_t)l_seq;
    }
    DecodeSummary sum{};
    sum.n_rec = n;
    S.W.aux = aux.data(); S.W.sum = &sum;
    CycleSamSrc src{S};
    launch(src, n, tables_of(base, qual, scal), n_blocks);
    return (long long)n;
}

// the one-thread form (what the host reader runs) over the same bytes: the records of a BAM stream
EMU_API long long cycemu_host_bam(const uint8_t *bytes, uint64_t n_bytes, uint64_t *base, uint64_t *qual, uint64_t *scal) {
    CycleCounts C{base, qual, {0, 0, 0, 0, 0, 0, 0, 0}};
    long long n = 0;
    for (uint64_t p = 0; p + 4 <= n_bytes; ++n) {
        const uint32_t bs = bam_ld32(bytes + p);
        if (bs < 32 || p + 4 + (uint64_t)bs > n_bytes) return -1;
        (void)cycle_count_bam(bytes + p, bs, C);
        p += 4 + (uint64_t)bs;
    }
    for (uint32_t k = 0; k < CYC_S_WORDS; ++k) scal[k] += C.s[k];
    return n;
}
