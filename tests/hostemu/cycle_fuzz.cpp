// cycle_fuzz.cpp -- TEST HARNESS ONLY: a stand-alone program (built with -fsanitize=address,undefined by tests/test_cycle_host.py and run
// as a child process) that hands bam_seq_layout and the per-record body of --cycles (rnaseqc_amd/csrc/rsqc_cycle.h) damaged records, each
// in a heap buffer of exactly its size: a read outside [rec, rec + 4 + block_size) is a heap overflow the sanitizer reports.
//   BAM   block_size short by 1..L bytes; l_seq 0x7FFFFFFF and negative; l_read_name 0; n_cigar at its maximum
//   SAM   the line cut at every length in front of the end of QUAL
// Every such record must count NOTHING; then random damage to the fixed part, where only the memory accesses are checked.
// Usage: cycle_fuzz [random cases] [seed].  Exit 0 and a line "cycle_fuzz: N cases, ..." -- or 1 with the case that counted.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../rnaseqc_amd/csrc/rsqc_cycle.h"
#include "../../rnaseqc_amd/csrc/rsqc_samrec.h"
#include "stage_fuzz.h"

using namespace rsqc;

namespace {

struct Counts {
    std::vector<uint64_t> base = std::vector<uint64_t>(CYC_BASE_CELLS, 0), qual = std::vector<uint64_t>(CYC_QUAL_CELLS, 0);
    CycleCounts c{base.data(), qual.data(), {0, 0, 0, 0, 0, 0, 0, 0}};
    bool empty() const {
        for (uint64_t v : base) if (v) return false;
        for (uint64_t v : qual) if (v) return false;
        for (uint64_t v : c.s) if (v) return false;
        return true;
    }
};

// (no tid or pos matters here: every operation is L M)
std::vector<uint8_t> make_record(uint32_t l_name, uint32_t n_cigar, uint32_t L, uint32_t flag) { return ::make_record(l_name, std::vector<uint32_t>(n_cigar, op(L, 0)), L, flag, 0, 100); }

// the record in a heap buffer of exactly `bytes` bytes; true: it counted something or the layout was accepted though it must not be
bool counts_something(const std::vector<uint8_t> &rec, size_t bytes, bool must_refuse) {
    Counts K;
    bool laid = false, counted = false;
    on_exact_heap(rec, bytes, [&](const uint8_t *heap, uint32_t bs) {
        uint32_t so, qo, L;
        laid = cycle_bam_layout(heap, bs, so, qo, L);
        counted = cycle_count_bam(heap, bs, K.c);
    });
    return must_refuse && (laid || counted || !K.empty());
}

int fail(const char *what, long long a, long long b) { printf("cycle_fuzz: COUNTED: %s (%lld, %lld)\n", what, a, b); return 1; }

}  // namespace

int main(int argc, char **argv) {
    const long n_random = argc > 1 ? atol(argv[1]) : 20000;
    seed_rnd(argc, argv);
    long long cases = 0;
    // a sound record counts (the harness would otherwise pass for the wrong reason)
    {
        const std::vector<uint8_t> r = make_record(5, 1, 37, 0);
        Counts K;
        if (!cycle_count_bam(r.data(), (uint32_t)r.size() - 4u, K.c) || K.c.s[CYC_S_RECORDS] != 1 || K.c.s[CYC_S_LEN_SUM] != 37) return fail("a sound record did not count", 0, 0);
    }
    const uint32_t Ls[] = {1, 2, 3, 17, 64, 65, 129, 700};
    for (uint32_t L : Ls)
        for (uint32_t l_name : {1u, 2u, 8u, 9u})
            for (uint32_t n_cigar : {0u, 1u, 3u}) {
                const std::vector<uint8_t> good = make_record(l_name, n_cigar, L, (L & 1u) ? 0x10u : 0x0u);
                const uint32_t bs = (uint32_t)good.size() - 4u;
                for (uint32_t d = 1; d <= L; ++d, ++cases) {                 // block_size short by d: the buffer ends where the record claims to
                    std::vector<uint8_t> r = good;
                    const uint32_t nbs = bs - d;
                    memcpy(r.data(), &nbs, 4);
                    if (counts_something(r, 4u + nbs, true)) return fail("block_size short", L, d);
                }
                for (int32_t l_seq : {0x7FFFFFFF, -1, -2, (int32_t)0x80000000, -(int32_t)L, 0x7FFFFFFE, (int32_t)(L + 1u)}) {
                    std::vector<uint8_t> r = good;
                    memcpy(r.data() + 20, &l_seq, 4);
                    ++cases;
                    if (counts_something(r, r.size(), true)) return fail("l_seq", L, l_seq);
                }
                {
                    std::vector<uint8_t> r = good;
                    r[12] = 0;                                               // l_read_name 0: no record has that
                    ++cases;
                    if (counts_something(r, r.size(), true)) return fail("l_read_name 0", L, l_name);
                }
                {
                    std::vector<uint8_t> r = good;
                    r[16] = r[17] = 0xFF;                                    // n_cigar 65535
                    ++cases;
                    if (counts_something(r, r.size(), true)) return fail("n_cigar", L, n_cigar);
                }
                {
                    std::vector<uint8_t> r = good;                           // block_size below the fixed part, the buffer as short
                    for (uint32_t nbs : {0u, 1u, 31u}) {
                        memcpy(r.data(), &nbs, 4);
                        ++cases;
                        if (counts_something(r, 36, true)) return fail("block_size below 32", L, nbs);
                    }
                }
            }
    // SAM: a line cut in front of the end of QUAL counts nothing
    for (uint32_t L : {1u, 2u, 5u, 64u, 130u})
        for (int star : {0, 1}) {
            std::string seq(L, 'A'), qual(L, 'I');
            for (uint32_t k = 0; k < L; ++k) { seq[k] = "ACGTN"[k % 5u]; qual[k] = (char)(33 + k % 60u); }
            const std::string head = "name\t16\tchrA\t101\t60\t" + std::to_string(L) + "M\t*\t0\t0\t";
            const std::string line = head + seq + "\t" + (star ? std::string("*") : qual);
            {
                uint32_t f[12];
                Counts K;
                if (!sam_fields_bytes((const uint8_t *)line.data(), (uint32_t)line.size(), f) || !cycle_count_sam((const uint8_t *)line.data(), (uint32_t)line.size(), f, 16, K.c) ||
                    K.c.s[CYC_S_RECORDS] != 1) return fail("a sound line did not count", L, star);
            }
            for (size_t len = 0; len < line.size(); ++len, ++cases) {
                uint8_t *heap = (uint8_t *)malloc(len ? len : 1);
                memcpy(heap, line.data(), len);
                uint32_t f[12];
                Counts K;
                bool counted = false;
                if (sam_fields_bytes(heap, (uint32_t)len, f)) counted = cycle_count_sam(heap, (uint32_t)len, f, 16, K.c);
                free(heap);
                // (a cut that leaves SEQ whole and QUAL as * or as long as SEQ is a line of its own right: there is none in front of the end)
                if (counted || !K.empty()) return fail("a cut SAM line", L, (long long)len);
            }
        }
    // random damage to the fixed part and the block size: only the accesses are checked
    long long refused = 0;
    for (long k = 0; k < n_random; ++k, ++cases) {
        std::vector<uint8_t> r = make_record(1u + rnd() % 12u, rnd() % 4u, rnd() % 300u, rnd() & 0xFFFu);
        const uint32_t hits = 1u + rnd() % 3u;
        for (uint32_t h = 0; h < hits; ++h) r[rnd() % 36u] = (uint8_t)rnd();
        const size_t bytes = clamp_block_size(r);
        Counts K;
        on_exact_heap(r, bytes, [&](const uint8_t *heap, uint32_t bs) { if (!cycle_count_bam(heap, bs, K.c)) ++refused; });
    }
    printf("cycle_fuzz: %lld cases, %lld of %ld random ones refused\n", cases, refused, n_random);
    return 0;
}
