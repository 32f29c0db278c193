// allele_fuzz.cpp -- TEST HARNESS ONLY: a stand-alone program (built with -fsanitize=address,undefined by tests/test_allele_host.py and run
// as a child process) that hands the one-thread form of --alleles (rnaseqc_amd/csrc/rsqc_allele.h) damaged records, each in a heap buffer
// of exactly its size, over a site table in heap buffers of exactly its length (pos[n_sites], first[n_contigs + 1], counts[n_sites][7]): a
// read outside [rec, rec + 4 + block_size) or outside the table is a heap overflow the sanitizer reports.
//   block_size short by 1..L bytes; l_seq 0x7FFFFFFF and negative; l_read_name 0; n_cigar at its maximum        -> contributes nothing
//   operations that run past L or stop short of it, none at all                                               -> inconsistent, no cell touched
//   pos near 2^31, negative, at and behind the last site; reference spans of 2^28 - 1 per operation           -> walked, nothing read outside
//   tid at the table's end, beyond it and negative                                                            -> off_contig, no cell touched
// then random damage to the fixed part and the operations, where only the memory accesses are checked.
// Usage: allele_fuzz [random cases] [seed].  Exit 0 and a line "allele_fuzz: N cases, ..." -- or 1 with the case that went wrong.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../rnaseqc_amd/csrc/rsqc_allele.h"
#include "stage_fuzz.h"

using namespace rsqc;

namespace {

// two contigs: sites at every third position of [0, 1002] and at the two ends of the range on contig 0, none on contig 1
struct Table {
    int32_t *pos; uint32_t *first; uint64_t *counts;
    uint32_t n;
    Table() {
        std::vector<int32_t> p;
        for (int32_t k = 0; k <= 1002; k += 3) p.push_back(k);
        p.push_back(0x7FFFFFFF - 9); p.push_back(0x7FFFFFFF - 1);
        n = (uint32_t)p.size();
        pos = (int32_t *)malloc((size_t)n * 4); memcpy(pos, p.data(), (size_t)n * 4);
        first = (uint32_t *)malloc(3 * 4); first[0] = 0; first[1] = n; first[2] = n;
        counts = (uint64_t *)calloc((size_t)n * AL_COLS, 8);
    }
    ~Table() { free(pos); free(first); free(counts); }
    AlleleSites sites() const { return AlleleSites{pos, first, 2}; }
    uint64_t sum() const { uint64_t s = 0; for (size_t k = 0; k < (size_t)n * AL_COLS; ++k) s += counts[k]; return s; }
    void clear() { memset(counts, 0, (size_t)n * AL_COLS * 8); }
};

struct Result { bool counted; uint64_t s[AL_S_WORDS]; uint64_t cells; };

// the record in a heap buffer of exactly `bytes` bytes, counted into a cleared table
Result count(const std::vector<uint8_t> &rec, size_t bytes, Table &T, uint32_t min_baseq = 0) {
    T.clear();
    AlleleCounts<AlleleHostCells> C{AlleleHostCells{T.counts}, {}};
    Result r{};
    on_exact_heap(rec, bytes, [&](const uint8_t *heap, uint32_t bs) { r.counted = allele_count_bam(heap, bs, T.sites(), 0, min_baseq, C); });
    memcpy(r.s, C.s, sizeof r.s);
    r.cells = T.sum();
    return r;
}
bool counts_something(const std::vector<uint8_t> &rec, size_t bytes, Table &T) {
    const Result r = count(rec, bytes, T);
    if (r.counted || r.cells) return true;
    for (uint64_t v : r.s) if (v) return true;
    return false;
}

int fail(const char *what, long long a, long long b) { printf("allele_fuzz: WRONG: %s (%lld, %lld)\n", what, a, b); return 1; }

}  // namespace

int main(int argc, char **argv) {
    const long n_random = argc > 1 ? atol(argv[1]) : 20000;
    seed_rnd(argc, argv);
    Table T;
    long long cases = 0;
    // a sound record counts (the harness would otherwise pass for the wrong reason): 30 M over [99, 129) meets 10 sites, the D of 3 one
    {
        const std::vector<uint8_t> r = make_record(5, {op(3, 4), op(30, 0), op(3, 2), op(4, 1)}, 37, 0, 0, 99);
        const Result k = count(r, r.size(), T);
        if (!k.counted || k.s[AL_S_RECORDS] != 1 || k.s[AL_S_HIT] != 1 || k.s[AL_S_OBS] != 11 || k.cells != 11) return fail("a sound record did not count", (long long)k.s[AL_S_OBS], (long long)k.cells);
    }
    const uint32_t Ls[] = {1, 2, 3, 17, 64, 65, 129, 700};
    for (uint32_t L : Ls)
        for (uint32_t l_name : {1u, 2u, 8u, 9u})
            for (uint32_t n_cigar : {1u, 3u}) {
                std::vector<uint32_t> ops = n_cigar == 1 ? std::vector<uint32_t>{op(L, 0)} : std::vector<uint32_t>{op(0, 4), op(L, 0), op(5, 3)};
                const std::vector<uint8_t> good = make_record(l_name, ops, L, (L & 1u) ? 0x10u : 0x0u, 0, 51);
                const uint32_t bs = (uint32_t)good.size() - 4u;
                const uint64_t under = (51 + L - 1) / 3 - 50 / 3;                               // the sites of [51, 51 + L)
                { const Result k = count(good, good.size(), T, 20); ++cases; if (!k.counted || k.s[AL_S_RECORDS] != 1 || k.cells != under || k.s[AL_S_OBS] != under) return fail("a sound record", L, (long long)k.cells); }
                for (uint32_t d = 1; d <= L; ++d, ++cases) {                 // block_size short by d: the buffer ends where the record claims to
                    std::vector<uint8_t> r = good;
                    const uint32_t nbs = bs - d;
                    memcpy(r.data(), &nbs, 4);
                    if (counts_something(r, 4u + nbs, T)) return fail("block_size short", L, d);
                }
                for (int32_t l_seq : {0x7FFFFFFF, -1, -2, (int32_t)0x80000000, -(int32_t)L, 0x7FFFFFFE, (int32_t)(L + 1u)}) {
                    std::vector<uint8_t> r = good;
                    memcpy(r.data() + 20, &l_seq, 4);
                    ++cases;
                    if (counts_something(r, r.size(), T)) return fail("l_seq", L, l_seq);
                }
                {
                    std::vector<uint8_t> r = good;
                    r[12] = 0;                                               // l_read_name 0: no record has that
                    ++cases;
                    if (counts_something(r, r.size(), T)) return fail("l_read_name 0", L, l_name);
                }
                {
                    std::vector<uint8_t> r = good;
                    r[16] = r[17] = 0xFF;                                    // n_cigar 65535
                    ++cases;
                    if (counts_something(r, r.size(), T)) return fail("n_cigar", L, n_cigar);
                }
                for (uint32_t nbs : {0u, 1u, 31u}) {                         // block_size below the fixed part, the buffer as short
                    std::vector<uint8_t> r = good;
                    memcpy(r.data(), &nbs, 4);
                    ++cases;
                    if (counts_something(r, 36, T)) return fail("block_size below 32", L, nbs);
                }
                // operations that run past L, stop short of it, or are none: one inconsistent record, no cell touched
                for (int how = 0; how < 5; ++how, ++cases) {
                    std::vector<uint32_t> bad = how == 0 ? std::vector<uint32_t>{op(L + 1u, 0)} : how == 1 ? std::vector<uint32_t>{op(L, 0), op(1, 1)} :
                                                how == 2 ? std::vector<uint32_t>{op(L - 1u, 0), op(9, 2)} : how == 3 ? std::vector<uint32_t>{op((1u << 28) - 1u, 0), op((1u << 28) - 1u, 4)} :
                                                           std::vector<uint32_t>{};
                    const std::vector<uint8_t> r = make_record(l_name, bad, L, 0x10u, 0, 50);
                    const Result k = count(r, r.size(), T);
                    if (!k.counted || k.s[AL_S_INCONSISTENT] != 1 || k.s[AL_S_RECORDS] != 0 || k.cells) return fail("inconsistent operations", L, how);
                }
                // positions at the edges of the table and of 32 bits; skips and deletions of the largest length in front of and behind the bases
                for (int32_t pos : {0x7FFFFFFF, 0x7FFFFFFF - (int32_t)L, 0x7FFFFFF0, -1, -(int32_t)L, (int32_t)0x80000000, 1002, 1003, 1003 - (int32_t)L}) {
                    for (int skips = 0; skips < 3; ++skips, ++cases) {
                        std::vector<uint32_t> o2 = skips == 1 ? std::vector<uint32_t>{op((1u << 28) - 1u, 3), op((1u << 28) - 1u, 2), op(L, 0), op((1u << 28) - 1u, 3)} :
                                                   skips == 2 ? std::vector<uint32_t>{op(L, 0), op((1u << 28) - 1u, 2), op((1u << 28) - 1u, 3), op((1u << 28) - 1u, 2)} : ops;
                        const std::vector<uint8_t> r = make_record(l_name, o2, L, (pos & 1) ? 0x10u : 0u, 0, pos);
                        const Result k = count(r, r.size(), T);
                        if (!k.counted || k.s[AL_S_RECORDS] != 1 || k.cells != k.s[AL_S_OBS] || k.cells > 400) return fail("pos at an edge", L, pos);
                    }
                }
                // a contig without sites; tid at the table's end, beyond it and negative
                { const std::vector<uint8_t> r = make_record(l_name, ops, L, 0, 1, 50); const Result k = count(r, r.size(), T); ++cases; if (!k.counted || k.s[AL_S_RECORDS] != 1 || k.cells) return fail("a contig without sites", L, 1); }
                for (int32_t tid : {2, 3, -1, 0x7FFFFFFF, (int32_t)0x80000000}) {
                    const std::vector<uint8_t> r = make_record(l_name, ops, L, 0, tid, 50);
                    const Result k = count(r, r.size(), T);
                    ++cases;
                    if (!k.counted || k.s[AL_S_OFF_CONTIG] != 1 || k.cells) return fail("off contig", L, tid);
                }
            }
    // random damage to the fixed part, the operations and the block size: only the accesses are checked
    long long walked = 0;
    for (long k = 0; k < n_random; ++k, ++cases) {
        const uint32_t L = rnd() % 300u, n_ops = rnd() % 5u;
        std::vector<uint32_t> ops;
        uint32_t left = L;
        for (uint32_t j = 0; j < n_ops; ++j) { const uint32_t n = j + 1 == n_ops ? left : (left ? rnd() % (left + 1u) : 0u); ops.push_back(op(n, (rnd() & 1u) ? 0u : rnd() % 10u)); if (mismatch_op_takes_query(ops.back() & 15u)) left -= n; }
        std::vector<uint8_t> r = make_record(1u + rnd() % 12u, ops, L, rnd() & ((rnd() & 3u) ? 0x4F3u : 0xFFFu), (int32_t)(rnd() % 4u) - 1, (int32_t)(rnd() % 1100u) - 50);
        const uint32_t hits = rnd() % 4u;
        for (uint32_t h = 0; h < hits; ++h) r[rnd() % (36u + (rnd() & 1u ? 24u : 0u)) % r.size()] = (uint8_t)rnd();
        const size_t bytes = clamp_block_size(r);
        const Result res = count(r, bytes, T, rnd() % 50u);
        if (res.cells != res.s[AL_S_OBS]) return fail("the cells and the observations differ", (long long)res.cells, (long long)res.s[AL_S_OBS]);
        if (res.s[AL_S_RECORDS]) ++walked;
    }
    printf("allele_fuzz: %lld cases, %lld of %ld random ones walked\n", cases, walked, n_random);
    return 0;
}
