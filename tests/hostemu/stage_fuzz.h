// stage_fuzz.h -- TEST HARNESS ONLY: what cycle_fuzz.cpp, mismatch_fuzz.cpp and allele_fuzz.cpp have in common: the generator of their
// random cases, a well-formed BAM record to damage, and the call of a one-thread form on a record in a heap buffer of exactly its size
// (a read outside [rec, rec + 4 + block_size) is a heap overflow the sanitizer reports).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

inline uint64_t rng_state = 1;
inline uint32_t rnd() { rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27; return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 33); }
// (main: [random cases] [seed])
inline void seed_rnd(int argc, char **argv) { rng_state = argc > 2 ? (uint64_t)atoll(argv[2]) * 0x9E3779B97F4A7C15ull | 1ull : 1ull; }

inline uint32_t op(uint32_t n, uint32_t code) { return n << 4 | code; }

// a well-formed record without an aux tail: block_size ends with QUAL
inline std::vector<uint8_t> make_record(uint32_t l_name, const std::vector<uint32_t> &ops, uint32_t L, uint32_t flag, int32_t tid, int32_t pos) {
    const uint32_t n_cigar = (uint32_t)ops.size(), bs = 32u + l_name + 4u * n_cigar + (L + 1u) / 2u + L;
    std::vector<uint8_t> r(4u + bs, 0);
    auto put32 = [&](size_t at, uint32_t v) { memcpy(r.data() + at, &v, 4); };
    put32(0, bs); put32(4, (uint32_t)tid); put32(8, (uint32_t)pos);
    r[12] = (uint8_t)l_name; r[13] = 60;
    const uint16_t nc = (uint16_t)n_cigar, fl = (uint16_t)flag;
    memcpy(r.data() + 16, &nc, 2); memcpy(r.data() + 18, &fl, 2);
    put32(20, L); put32(24, 0xFFFFFFFFu); put32(28, 0xFFFFFFFFu);
    for (uint32_t k = 0; k + 1 < l_name; ++k) r[36 + k] = 'q';
    for (uint32_t k = 0; k < n_cigar; ++k) put32(36u + l_name + 4u * k, ops[k]);
    uint8_t *seq = r.data() + 36u + l_name + 4u * n_cigar;
    for (uint32_t k = 0; k < (L + 1u) / 2u; ++k) seq[k] = (uint8_t)(0x12u << (k & 1u) | 0x48u);
    uint8_t *qual = seq + (L + 1u) / 2u;
    for (uint32_t k = 0; k < L; ++k) qual[k] = (uint8_t)(k % 41u);
    return r;
}

// the first `bytes` bytes of rec in a heap buffer of exactly that size: f(heap, block_size as the record states it)
template <class F> void on_exact_heap(const std::vector<uint8_t> &rec, size_t bytes, F f) {
    uint8_t *heap = (uint8_t *)malloc(bytes ? bytes : 1);
    memcpy(heap, rec.data(), bytes);
    uint32_t bs; memcpy(&bs, heap, 4);
    f((const uint8_t *)heap, bs);
    free(heap);
}
// the random cases' last step: a block size that leaves the record is redrawn (the framing never hands on a record that leaves its window),
// the record padded to the 36 bytes of the fixed part.  Returns the bytes of its buffer
inline size_t clamp_block_size(std::vector<uint8_t> &r) {
    uint32_t bs; memcpy(&bs, r.data(), 4);
    if (bs > r.size() - 4u) { bs = (uint32_t)(rnd() % (r.size() - 3u)); memcpy(r.data(), &bs, 4); }
    const size_t bytes = 4u + (size_t)bs < 36u ? 36u : 4u + (size_t)bs;
    r.resize(bytes > r.size() ? bytes : r.size());
    return bytes;
}
