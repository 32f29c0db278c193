// genebody_emu.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// The KERNEL of --gene-body -- rnaseqc_amd/csrc/rsqc_genebody.h, unmodified, with the model check and the launch plan of the same
// header -- compiled for the host on top of the 64-lane fiber emulation of wavemu.h.  The host side of rsqc_genebody_api.cpp (the
// layout of the scanned difference array, the order of the steps) is restated here with plain memory: the depth of every position
// is handed in, laid out as rsqc_track_end leaves it (contig t at off[t], one pad slot behind every contig, the depth of slot i at
// i + 1).  The expected sums are NOT computed here: tests/genebody_ref.py restates the contract in Python and the test compares.
// With -DGBEMU_MAIN the file is a stand-alone program over a case file (for a sanitizer build).
#include "wavemu.h"

#include <string>
#include <vector>

#include "../../rnaseqc_amd/csrc/rsqc_genebody.h"

using namespace rsqc;

namespace {
template <class F> void launch(uint32_t grid, F &&body) {
    wavemu::grid_dim().x = grid;
    for (uint32_t b = 0; b < grid; ++b) { wavemu::block_idx().x = b; wavemu::run_block(RSQC_GENEBODY_THREADS, body); }
}
constexpr unsigned long long kGuard64 = 0xA5A5A5A5A5A5A5A5ull;
struct State {
    GenebodyPlan plan;
    std::vector<unsigned long long> sums;
    std::string error;
} G;
}  // namespace

#define EMU_API extern "C" __attribute__((visibility("default")))

EMU_API void gbemu_set_schedule_seed(unsigned long long seed) { wavemu::set_seed(seed); }

// depth: the contigs' positions one behind the other (no pads).  stats: [0] n_genes, [1] n_measured, [2] model_bases, [3] depth_sum,
// [4] items, [5] workgroups.  Returns 0; 1: the model breaks a rule (gbemu_error); 3000 + k: check k of the harness itself
EMU_API int gbemu_run(int32_t n_contigs, const uint64_t *length, const uint32_t *depth, int32_t n_genes, const uint32_t *seg_off, const int32_t *seg_tid,
                      const uint32_t *seg_start, const uint32_t *seg_end, const uint8_t *reverse, uint64_t *stats) {
    G = State{};
    std::vector<uint64_t> off((size_t)n_contigs + 1, 0);
    std::vector<uint32_t> len32((size_t)n_contigs + 1, 0);
    for (int32_t t = 0; t < n_contigs; ++t) { len32[(size_t)t] = (uint32_t)length[t]; off[(size_t)t + 1] = off[(size_t)t] + length[t] + 1; }
    const uint64_t total = off[(size_t)n_contigs];
    G.error = genebody_check(n_genes, seg_off, seg_tid, seg_start, seg_end, n_contigs, len32.data());
    if (!G.error.empty()) return 1;
    // the scanned array: total + 1 entries, exactly (a read past it is a heap overflow under the sanitizer build)
    std::vector<uint32_t> S((size_t)total + 1, 0u);
    size_t at = 0;
    for (int32_t t = 0; t < n_contigs; ++t)
        for (uint64_t p = 0; p < length[t]; ++p) S[(size_t)(off[(size_t)t] + p) + 1] = depth[at++];
    genebody_plan(n_genes, seg_off, seg_start, seg_end, reverse, RSQC_GENEBODY_ITEM, G.plan);
    G.sums.assign((size_t)n_genes * RSQC_GENEBODY_BINS + 1, 0ull);
    G.sums.back() = kGuard64;
    unsigned long long tot[2] = {0ull, kGuard64};
    const uint64_t n_items = G.plan.items.size();
    const uint32_t grid = (uint32_t)((n_items + RSQC_GENEBODY_WAVES - 1) / RSQC_GENEBODY_WAVES);
    // (the model's columns at exactly their size as well)
    const size_t n_seg = n_genes ? seg_off[n_genes] : 0;
    std::vector<int32_t> m_tid(seg_tid, seg_tid + n_seg); std::vector<uint32_t> m_start(seg_start, seg_start + n_seg), m_end(seg_end, seg_end + n_seg);
    std::vector<GenebodyItem> items(G.plan.items);
    const GenebodyModel M{m_tid.data(), m_start.data(), m_end.data()};
    if (grid) launch(grid, [&]() { genebody_bins_kernel(S.data(), off.data(), M, items.data(), n_items, G.sums.data(), tot); });
    if (G.sums.back() != kGuard64) return 3001;
    if (tot[1] != kGuard64) return 3002;
    G.sums.pop_back();
    stats[0] = (uint64_t)n_genes; stats[1] = G.plan.n_measured; stats[2] = G.plan.model_bases; stats[3] = tot[0]; stats[4] = n_items; stats[5] = grid;
    return 0;
}

// the plan alone, of a model that keeps the rules; stats as above (depth_sum 0)
EMU_API void gbemu_plan(int32_t n_genes, const uint32_t *seg_off, const uint32_t *seg_start, const uint32_t *seg_end, const uint8_t *reverse, uint64_t *stats) {
    G = State{};
    genebody_plan(n_genes, seg_off, seg_start, seg_end, reverse, RSQC_GENEBODY_ITEM, G.plan);
    const uint64_t n_items = G.plan.items.size();
    stats[0] = (uint64_t)n_genes; stats[1] = G.plan.n_measured; stats[2] = G.plan.model_bases; stats[3] = 0; stats[4] = n_items; stats[5] = (n_items + RSQC_GENEBODY_WAVES - 1) / RSQC_GENEBODY_WAVES;
}

EMU_API const char *gbemu_error() { return G.error.c_str(); }
EMU_API void gbemu_sums(uint64_t *out) { for (size_t k = 0; k < G.sums.size(); ++k) out[k] = G.sums[k]; }
// the plan's items, six words each: gene, u0, u1, seg, seg_u, L | reverse << 31
EMU_API void gbemu_items(uint32_t *out) { if (!G.plan.items.empty()) memcpy(out, G.plan.items.data(), G.plan.items.size() * sizeof(GenebodyItem)); }

#if defined(GBEMU_MAIN)
// genebody_emu CASEFILE: four 64-bit words (contigs, genes, segments, schedule seed), the lengths (64-bit each), the depth of every
// position, seg_off, seg_tid, seg_start, seg_end (32-bit each), the reverse bytes.  Prints the figures and a weighted sum of the
// bins, exits 0, or 1 with the failed check.
int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: genebody_emu CASEFILE\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint64_t head[4];
    if (fread(head, 8, 4, f) != 4) return 2;
    const size_t nc = (size_t)head[0], ng = (size_t)head[1], ns = (size_t)head[2];
    std::vector<uint64_t> length(nc);
    if (nc && fread(length.data(), 8, nc, f) != nc) return 2;
    size_t positions = 0;
    for (uint64_t l : length) positions += (size_t)l;
    std::vector<uint32_t> depth(positions), seg_off(ng + 1), seg_start(ns), seg_end(ns); std::vector<int32_t> seg_tid(ns); std::vector<uint8_t> reverse(ng);
    if ((positions && fread(depth.data(), 4, positions, f) != positions) || fread(seg_off.data(), 4, ng + 1, f) != ng + 1 ||
        (ns && (fread(seg_tid.data(), 4, ns, f) != ns || fread(seg_start.data(), 4, ns, f) != ns || fread(seg_end.data(), 4, ns, f) != ns)) ||
        (ng && fread(reverse.data(), 1, ng, f) != ng)) { fprintf(stderr, "short case file\n"); return 2; }
    fclose(f);
    wavemu::set_seed(head[3]);
    uint64_t st[6] = {0, 0, 0, 0, 0, 0};
    const int rc = gbemu_run((int32_t)nc, length.data(), depth.data(), (int32_t)ng, seg_off.data(), seg_tid.data(), seg_start.data(), seg_end.data(), reverse.data(), st);
    unsigned long long weighted = 0;
    for (size_t k = 0; k < G.sums.size(); ++k) weighted += G.sums[k] * (unsigned long long)(k % RSQC_GENEBODY_BINS + 1);
    printf("genebody_emu: rc=%d genes=%llu measured=%llu bases=%llu depth_sum=%llu items=%llu weighted=%llu\n", rc, (unsigned long long)st[0], (unsigned long long)st[1],
           (unsigned long long)st[2], (unsigned long long)st[3], (unsigned long long)st[4], weighted);
    if (rc == 1) fprintf(stderr, "%s\n", G.error.c_str());
    return rc ? 1 : 0;
}
#endif
