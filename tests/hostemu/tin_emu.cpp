// tin_emu.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// The KERNELS of --tin -- rnaseqc_amd/csrc/rsqc_tin.h, unmodified, with the launch plan of the same header and the model check and
// the walk of rsqc_genemodel.h -- compiled for the host on top of the 64-lane fiber emulation of wavemu.h.  The host side of
// rsqc_tin_api.cpp (the layout of the scanned difference array, the order of the steps) is restated with plain memory: the depth of
// every position is handed in and laid out as rsqc_track_end leaves it (genemodel_emu.h, shared with genebody_emu.cpp).  The item
// slots and the rows start as a pattern that no kernel writes: a slot or row that is left out shows.  The expected rows are NOT
// computed here: tests/tin_ref.py restates the contract in Python and the test compares.
// With -DTINEMU_MAIN the file is a stand-alone program over a case file (for a sanitizer build).
#include "wavemu.h"

#include "genemodel_emu.h"
#include "../../rnaseqc_amd/csrc/rsqc_tin.h"

using namespace rsqc;

namespace {
struct State {
    TinPlan plan;
    std::vector<rsqc_tin_row> rows;
    std::string error;
} G;
}  // namespace

#define EMU_API extern "C" __attribute__((visibility("default")))

EMU_API void tinemu_set_schedule_seed(unsigned long long seed) { wavemu::set_seed(seed); }

// depth: the contigs' positions one behind the other (no pads).  stats: [0] n_genes, [1] n_measured, [2] model_bases, [3] items,
// [4] workgroups of the items kernel.  Returns 0; 1: the model breaks a rule (tinemu_error)
EMU_API int tinemu_run(int32_t n_contigs, const uint64_t *length, const uint32_t *depth, int32_t n_genes, const uint32_t *seg_off, const int32_t *seg_tid,
                       const uint32_t *seg_start, const uint32_t *seg_end, uint64_t *stats) {
    G = State{};
    gmemu::Input in;
    G.error = gmemu::lay_out(in, n_contigs, length, depth, n_genes, seg_off, seg_tid, seg_start, seg_end);
    if (!G.error.empty()) return 1;
    tin_plan(n_genes, seg_off, seg_start, seg_end, RSQC_TIN_ITEM, G.plan);
    const uint64_t n_items = G.plan.items.size();
    const uint32_t grid = (uint32_t)((n_items + RSQC_TIN_WAVES - 1) / RSQC_TIN_WAVES);
    // (the plan, the slots and the rows at exactly their size as well; slots and rows filled with 0xA5: no memset is owed)
    std::vector<TinItem> items(G.plan.items);
    std::vector<uint64_t> item_off(G.plan.item_off);
    std::vector<rsqc_tin_row> part((size_t)n_items);
    G.rows.resize((size_t)n_genes);
    if (n_items) memset(part.data(), 0xA5, part.size() * sizeof(rsqc_tin_row));
    if (n_genes) memset(G.rows.data(), 0xA5, G.rows.size() * sizeof(rsqc_tin_row));
    if (grid) gmemu::launch(grid, RSQC_TIN_THREADS, [&]() { tin_items_kernel(in.S.data(), in.off.data(), in.model(), items.data(), n_items, part.data()); });
    const uint32_t row_grid = ((uint32_t)n_genes + RSQC_TIN_THREADS - 1) / RSQC_TIN_THREADS;
    if (row_grid) gmemu::launch(row_grid, RSQC_TIN_THREADS, [&]() { tin_rows_kernel(part.data(), item_off.data(), (uint32_t)n_genes, G.rows.data()); });
    stats[0] = (uint64_t)n_genes; stats[1] = G.plan.n_measured; stats[2] = G.plan.model_bases; stats[3] = n_items; stats[4] = grid;
    return 0;
}

// the plan alone, of a model that keeps the rules; stats as above
EMU_API void tinemu_plan(int32_t n_genes, const uint32_t *seg_off, const uint32_t *seg_start, const uint32_t *seg_end, uint64_t *stats) {
    G = State{};
    tin_plan(n_genes, seg_off, seg_start, seg_end, RSQC_TIN_ITEM, G.plan);
    const uint64_t n_items = G.plan.items.size();
    stats[0] = (uint64_t)n_genes; stats[1] = G.plan.n_measured; stats[2] = G.plan.model_bases; stats[3] = n_items; stats[4] = (n_items + RSQC_TIN_WAVES - 1) / RSQC_TIN_WAVES;
}

EMU_API const char *tinemu_error() { return G.error.c_str(); }
EMU_API void tinemu_rows(rsqc_tin_row *out) { for (size_t k = 0; k < G.rows.size(); ++k) out[k] = G.rows[k]; }
// the plan's items, five words each: gene, u0, u1, seg, seg_u; and every gene's first item with one entry behind the last
EMU_API void tinemu_items(uint32_t *out) { if (!G.plan.items.empty()) memcpy(out, G.plan.items.data(), G.plan.items.size() * sizeof(TinItem)); }
EMU_API void tinemu_item_off(uint64_t *out) { memcpy(out, G.plan.item_off.data(), G.plan.item_off.size() * 8); }

#if defined(TINEMU_MAIN)
// tin_emu CASEFILE (genemodel_emu.h, without reverse bytes).  Prints the figures, the integer sums over the rows and the bits of the
// doubles folded into one word, exits 0, or 1 with the failed check.
int main(int argc, char **argv) {
    gmemu::CaseFile C;
    if (int rc = gmemu::read_case("tin_emu", argc, argv, false, C)) return rc;
    wavemu::set_seed(C.seed);
    uint64_t st[5] = {0, 0, 0, 0, 0};
    const int rc = tinemu_run((int32_t)C.length.size(), C.length.data(), C.depth.data(), (int32_t)C.seg_off.size() - 1, C.seg_off.data(), C.seg_tid.data(), C.seg_start.data(), C.seg_end.data(), st);
    unsigned long long sum = 0, covered = 0, peak = 0, bits = 0;
    for (const rsqc_tin_row &r : G.rows) {
        unsigned long long b; memcpy(&b, &r.dlog2d, 8);
        sum += r.depth_sum; covered += r.covered; peak += r.max_depth; bits = (bits * 1000003ull) ^ b;
    }
    printf("tin_emu: rc=%d genes=%llu measured=%llu bases=%llu items=%llu depth_sum=%llu covered=%llu peaks=%llu bits=%llu\n", rc, (unsigned long long)st[0], (unsigned long long)st[1],
           (unsigned long long)st[2], (unsigned long long)st[3], sum, covered, peak, bits);
    if (rc == 1) fprintf(stderr, "%s\n", G.error.c_str());
    return rc ? 1 : 0;
}
#endif
