// genebody_emu.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// The KERNEL of --gene-body -- rnaseqc_amd/csrc/rsqc_genebody.h, unmodified, with its launch plan and the model check and the walk
// of rsqc_genemodel.h -- compiled for the host on top of the 64-lane fiber emulation of wavemu.h.  The host side of
// rsqc_genebody_api.cpp (the layout of the scanned difference array, the order of the steps) is restated with plain memory: the depth
// of every position is handed in and laid out as rsqc_track_end leaves it (genemodel_emu.h, shared with tin_emu.cpp).  The expected
// sums are NOT computed here: tests/genebody_ref.py restates the contract in Python and the test compares.
// With -DGBEMU_MAIN the file is a stand-alone program over a case file (for a sanitizer build).
#include "wavemu.h"

#include "genemodel_emu.h"
#include "../../rnaseqc_amd/csrc/rsqc_genebody.h"

using namespace rsqc;

namespace {
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
    gmemu::Input in;
    G.error = gmemu::lay_out(in, n_contigs, length, depth, n_genes, seg_off, seg_tid, seg_start, seg_end);
    if (!G.error.empty()) return 1;
    genebody_plan(n_genes, seg_off, seg_start, seg_end, reverse, RSQC_GENEBODY_ITEM, G.plan);
    G.sums.assign((size_t)n_genes * RSQC_GENEBODY_BINS + 1, 0ull);
    G.sums.back() = kGuard64;
    unsigned long long tot[2] = {0ull, kGuard64};
    const uint64_t n_items = G.plan.items.size();
    const uint32_t grid = (uint32_t)((n_items + RSQC_GENEBODY_WAVES - 1) / RSQC_GENEBODY_WAVES);
    std::vector<GenebodyItem> items(G.plan.items);     // (the plan at exactly its size as well)
    if (grid) gmemu::launch(grid, RSQC_GENEBODY_THREADS, [&]() { genebody_bins_kernel(in.S.data(), in.off.data(), in.model(), items.data(), n_items, G.sums.data(), tot); });
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
// genebody_emu CASEFILE (genemodel_emu.h, with the reverse bytes).  Prints the figures and a weighted sum of the bins, exits 0, or 1
// with the failed check.
int main(int argc, char **argv) {
    gmemu::CaseFile C;
    if (int rc = gmemu::read_case("genebody_emu", argc, argv, true, C)) return rc;
    wavemu::set_seed(C.seed);
    uint64_t st[6] = {0, 0, 0, 0, 0, 0};
    const int rc = gbemu_run((int32_t)C.length.size(), C.length.data(), C.depth.data(), (int32_t)C.reverse.size(), C.seg_off.data(), C.seg_tid.data(), C.seg_start.data(), C.seg_end.data(), C.reverse.data(), st);
    unsigned long long weighted = 0;
    for (size_t k = 0; k < G.sums.size(); ++k) weighted += G.sums[k] * (unsigned long long)(k % RSQC_GENEBODY_BINS + 1);
    printf("genebody_emu: rc=%d genes=%llu measured=%llu bases=%llu depth_sum=%llu items=%llu weighted=%llu\n", rc, (unsigned long long)st[0], (unsigned long long)st[1],
           (unsigned long long)st[2], (unsigned long long)st[3], (unsigned long long)st[4], weighted);
    if (rc == 1) fprintf(stderr, "%s\n", G.error.c_str());
    return rc ? 1 : 0;
}
#endif
