// mismatch_fuzz.cpp -- TEST HARNESS ONLY: a stand-alone program (built with -fsanitize=address,undefined by tests/test_mismatch_host.py and
// run as a child process) that hands the one-thread form of --mismatches (rnaseqc_amd/csrc/rsqc_mismatch.h) damaged records, each in a heap
// buffer of exactly its size, over a reference in a heap buffer of exactly its length: a read outside [rec, rec + 4 + block_size) or
// outside the contig is a heap overflow the sanitizer reports.
//   block_size short by 1..L bytes; l_seq 0x7FFFFFFF and negative; l_read_name 0; n_cigar at its maximum        -> contributes nothing
//   operations that run past L or stop short of it, none at all                                               -> inconsistent, no table touched
//   pos near 2^31, negative, at and behind the contig's end; reference spans of 2^28 - 1 per operation        -> counted, nothing read outside
// then random damage to the fixed part and the operations, where only the memory accesses are checked.
// Usage: mismatch_fuzz [random cases] [seed].  Exit 0 and a line "mismatch_fuzz: N cases, ..." -- or 1 with the case that went wrong.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../rnaseqc_amd/csrc/rsqc_mismatch.h"
#include "stage_fuzz.h"

using namespace rsqc;

namespace {

constexpr uint64_t REF_LEN = 1003;

struct Counts {
    std::vector<uint64_t> cyc = std::vector<uint64_t>(MM_CYC_CELLS, 0), subst = std::vector<uint64_t>(MM_SUBST_CELLS, 0), byq = std::vector<uint64_t>(MM_BYQ_CELLS, 0);
    MismatchCounts c{cyc.data(), subst.data(), byq.data(), {}};
    bool tables_empty() const {
        for (uint64_t v : cyc) if (v) return false;
        for (uint64_t v : subst) if (v) return false;
        for (uint64_t v : byq) if (v) return false;
        return true;
    }
    bool empty() const {
        for (uint64_t v : c.s) if (v) return false;
        return tables_empty();
    }
    uint64_t query_bases() const {
        uint64_t n = c.s[MM_S_BEYOND];
        for (size_t k = 0; k < cyc.size(); ++k) if (k % MM_COLS != MM_MISMATCH && k % MM_COLS != MM_DELETIONS) n += cyc[k];
        return n;
    }
};

struct Reference {
    char *bases;                                       // exactly REF_LEN bytes on the heap
    const char *seq[2]; uint64_t len[2];
    Reference() {
        bases = (char *)malloc(REF_LEN);
        for (uint64_t k = 0; k < REF_LEN; ++k) bases[k] = "ACGTNacgt"[(k * 7 + k / 9) % 9];
        seq[0] = bases; seq[1] = nullptr; len[0] = REF_LEN; len[1] = 500;
    }
    ~Reference() { free(bases); }
    MismatchTextRef ref() const { return MismatchTextRef{seq, len, 2}; }
};

// the record in a heap buffer of exactly `bytes` bytes, counted into K; what mismatch_count_bam answered
bool count(const std::vector<uint8_t> &rec, size_t bytes, const Reference &R, Counts &K) {
    bool counted = false;
    on_exact_heap(rec, bytes, [&](const uint8_t *heap, uint32_t bs) { counted = mismatch_count_bam(heap, bs, R.ref(), 0, K.c); });
    return counted;
}
bool counts_something(const std::vector<uint8_t> &rec, size_t bytes, const Reference &R) {
    Counts K;
    return count(rec, bytes, R, K) || !K.empty();
}

int fail(const char *what, long long a, long long b) { printf("mismatch_fuzz: WRONG: %s (%lld, %lld)\n", what, a, b); return 1; }

}  // namespace

int main(int argc, char **argv) {
    const long n_random = argc > 1 ? atol(argv[1]) : 20000;
    seed_rnd(argc, argv);
    const Reference R;
    long long cases = 0;
    // a sound record counts (the harness would otherwise pass for the wrong reason)
    {
        const std::vector<uint8_t> r = make_record(5, {op(3, 4), op(30, 0), op(2, 2), op(4, 1)}, 37, 0, 0, 100);
        Counts K;
        if (!count(r, r.size(), R, K) || K.c.s[MM_S_RECORDS] != 1 || K.c.s[MM_S_LEN_SUM] != 37 || K.query_bases() != 37 || K.c.s[MM_S_DEL_BASES] != 2) return fail("a sound record did not count", 0, 0);
    }
    const uint32_t Ls[] = {1, 2, 3, 17, 64, 65, 129, 700};
    for (uint32_t L : Ls)
        for (uint32_t l_name : {1u, 2u, 8u, 9u})
            for (uint32_t n_cigar : {1u, 3u}) {
                std::vector<uint32_t> ops = n_cigar == 1 ? std::vector<uint32_t>{op(L, 0)} : std::vector<uint32_t>{op(0, 4), op(L, 0), op(5, 3)};
                const std::vector<uint8_t> good = make_record(l_name, ops, L, (L & 1u) ? 0x10u : 0x0u, 0, 50);
                const uint32_t bs = (uint32_t)good.size() - 4u;
                { Counts K; ++cases; if (!count(good, good.size(), R, K) || K.c.s[MM_S_RECORDS] != 1 || K.query_bases() != L) return fail("a sound record", L, l_name); }
                for (uint32_t d = 1; d <= L; ++d, ++cases) {                 // block_size short by d: the buffer ends where the record claims to
                    std::vector<uint8_t> r = good;
                    const uint32_t nbs = bs - d;
                    memcpy(r.data(), &nbs, 4);
                    if (counts_something(r, 4u + nbs, R)) return fail("block_size short", L, d);
                }
                for (int32_t l_seq : {0x7FFFFFFF, -1, -2, (int32_t)0x80000000, -(int32_t)L, 0x7FFFFFFE, (int32_t)(L + 1u)}) {
                    std::vector<uint8_t> r = good;
                    memcpy(r.data() + 20, &l_seq, 4);
                    ++cases;
                    if (counts_something(r, r.size(), R)) return fail("l_seq", L, l_seq);
                }
                {
                    std::vector<uint8_t> r = good;
                    r[12] = 0;                                               // l_read_name 0: no record has that
                    ++cases;
                    if (counts_something(r, r.size(), R)) return fail("l_read_name 0", L, l_name);
                }
                {
                    std::vector<uint8_t> r = good;
                    r[16] = r[17] = 0xFF;                                    // n_cigar 65535
                    ++cases;
                    if (counts_something(r, r.size(), R)) return fail("n_cigar", L, n_cigar);
                }
                for (uint32_t nbs : {0u, 1u, 31u}) {                         // block_size below the fixed part, the buffer as short
                    std::vector<uint8_t> r = good;
                    memcpy(r.data(), &nbs, 4);
                    ++cases;
                    if (counts_something(r, 36, R)) return fail("block_size below 32", L, nbs);
                }
                // operations that run past L, stop short of it, or are none: one inconsistent record, no table touched
                for (int how = 0; how < 5; ++how, ++cases) {
                    std::vector<uint32_t> bad = how == 0 ? std::vector<uint32_t>{op(L + 1u, 0)} : how == 1 ? std::vector<uint32_t>{op(L, 0), op(1, 1)} :
                                                how == 2 ? std::vector<uint32_t>{op(L - 1u, 0), op(9, 2)} : how == 3 ? std::vector<uint32_t>{op((1u << 28) - 1u, 0), op((1u << 28) - 1u, 4)} :
                                                           std::vector<uint32_t>{};
                    const std::vector<uint8_t> r = make_record(l_name, bad, L, 0x10u, 0, 50);
                    Counts K;
                    if (!count(r, r.size(), R, K) || K.c.s[MM_S_INCONSISTENT] != 1 || K.c.s[MM_S_RECORDS] != 0 || !K.tables_empty()) return fail("inconsistent operations", L, how);
                }
                // positions at the edges of the contig and of 32 bits; skips of the largest length in front of and behind the bases
                for (int32_t pos : {0x7FFFFFFF, 0x7FFFFFFF - (int32_t)L, 0x7FFFFFF0, -1, -(int32_t)L, (int32_t)0x80000000, (int32_t)REF_LEN - 1, (int32_t)REF_LEN, (int32_t)REF_LEN - (int32_t)L}) {
                    for (int skips = 0; skips < 2; ++skips, ++cases) {
                        std::vector<uint32_t> o2 = skips ? std::vector<uint32_t>{op((1u << 28) - 1u, 3), op((1u << 28) - 1u, 2), op(L, 0), op((1u << 28) - 1u, 3)} : ops;
                        const std::vector<uint8_t> r = make_record(l_name, o2, L, (pos & 1) ? 0x10u : 0u, 0, pos);
                        Counts K;
                        if (!count(r, r.size(), R, K) || K.c.s[MM_S_RECORDS] != 1 || K.query_bases() != L) return fail("pos at an edge", L, pos);
                    }
                }
                // a contig without bases, a tid outside the reference
                for (int32_t tid : {1, 2, -1, 0x7FFFFFFF}) {
                    const std::vector<uint8_t> r = make_record(l_name, ops, L, 0, tid, 50);
                    Counts K;
                    ++cases;
                    if (!count(r, r.size(), R, K) || K.c.s[MM_S_NO_REF] != 1 || !K.tables_empty()) return fail("no reference", L, tid);
                }
            }
    // random damage to the fixed part, the operations and the block size: only the accesses are checked
    long long refused = 0;
    for (long k = 0; k < n_random; ++k, ++cases) {
        const uint32_t L = rnd() % 300u, n_ops = rnd() % 5u;
        std::vector<uint32_t> ops;
        uint32_t left = L;
        for (uint32_t j = 0; j < n_ops; ++j) { const uint32_t n = j + 1 == n_ops ? left : (left ? rnd() % (left + 1u) : 0u); ops.push_back(op(n, (rnd() & 1u) ? 0u : rnd() % 10u)); if (mismatch_op_takes_query(ops.back() & 15u)) left -= n; }
        std::vector<uint8_t> r = make_record(1u + rnd() % 12u, ops, L, rnd() & 0xFFFu, (int32_t)(rnd() % 3u), (int32_t)(rnd() % 1100u) - 50);
        const uint32_t hits = rnd() % 4u;
        for (uint32_t h = 0; h < hits; ++h) r[rnd() % (36u + (rnd() & 1u ? 24u : 0u)) % r.size()] = (uint8_t)rnd();
        const size_t bytes = clamp_block_size(r);
        Counts K;
        if (!count(r, bytes, R, K)) ++refused;
    }
    printf("mismatch_fuzz: %lld cases, %lld of %ld random ones refused\n", cases, refused, n_random);
    return 0;
}
