// rsqc_k5_plan.h -- the launch plan of K5, the fragment-size sampler and the mate pairing of the GC statistics (rsqc_k5.h): how many
// buckets the candidates are cut into and the grids of the stages behind the pairing.  Host arithmetic only, plain C++ and no HIP types:
// the library (rsqc_fragsize.hip) and the host emulation of the tests (tests/hostemu/k5_emu.cpp, gc_emu.cpp) share it, so the plan that
// runs on the GPU is the plan the CPU tests check.
#pragma once

#include <stdint.h>

namespace rsqc {

constexpr uint32_t PB_MEAN = 384;            // candidates per bucket on average (the name hashes are fmix64 outputs: Poisson; <= 512, the hashed pairing's limit, in all but one bucket in 10^9)
constexpr uint32_t K5_PART_THREADS = 256;    // pair_bucket_count_kernel / pair_bucket_scatter_kernel: one candidate per thread
constexpr uint32_t K5_BIG_GRID = 64;         // workgroups of *_replay_big_kernel: listed buckets t, t + 64, ... each

// buckets of the pairing stage for n candidates
inline uint32_t k5_bucket_count(uint32_t n) { const uint32_t b = n / PB_MEAN; return b > 1u ? b : 1u; }
// grid of the count and the scatter kernels
inline uint32_t k5_part_grid(uint32_t n) { return (n + K5_PART_THREADS - 1u) / K5_PART_THREADS; }

// the stages behind the replay: ns_bound = the most samples n candidates can yield (a sample takes two candidates)
struct K5Plan {
    uint32_t n_buckets, part_grid, big_grid;
    uint32_t ns_bound;
    uint32_t select_grid;                    // sample_digit_hist_kernel, 256 threads, grid-stride
    uint32_t keep_grid;                      // sample_keep_kernel, 1024 threads, one sample per thread
    uint32_t size_grid;                      // size_hist_kernel, 256 threads, grid-stride
};
inline K5Plan k5_plan(uint32_t n, uint32_t max_samples) {
    K5Plan p;
    p.n_buckets = k5_bucket_count(n); p.part_grid = k5_part_grid(n); p.big_grid = K5_BIG_GRID;
    p.ns_bound = n / 2u + 1u;
    const uint32_t sel = (p.ns_bound + 255u) / 256u;
    p.select_grid = sel < 1024u ? sel : 1024u;
    p.keep_grid = (p.ns_bound + 1023u) / 1024u;
    const uint32_t kept = p.ns_bound < max_samples ? p.ns_bound : max_samples, sz = (kept + 255u) / 256u;
    p.size_grid = sz < 512u ? sz : 512u;
    return p;
}

}  // namespace rsqc
