// k3_emu.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// The end-of-file coverage KERNEL -- rnaseqc_amd/csrc/rsqc_k3.h (gene_coverage_kernel in the library's eight instances, each with the
// 128-entry and the RSQC_MAX_BIAS_WINDOW-entry bias window), unmodified -- compiled for the host on top of the 64-lane fiber emulation
// of wavemu.h, and launched by the library's own plan (rnaseqc_amd/csrc/rsqc_k3_plan.h: class counts + the eight launches).  Input: the per-base difference array and the gene
// counts a pass over the records leaves (the caller takes them from hostemu_run, the per-record code on the host); output: what
// the kernel writes -- per-gene mean / std / CV (+ validity), per-exon CV, the bias accumulators -- for comparison with the oracle.
#include "wavemu.h"

#include <algorithm>
#include <string>
#include <vector>

#include "../../rnaseqc_amd/csrc/rsqc_read.h"
#include "../../rnaseqc_amd/csrc/rsqc_device.h"
#include "../../rnaseqc_amd/csrc/rsqc_index.h"
#include "../../rnaseqc_amd/csrc/rsqc_wave.h"
#define RSQC_FIN_STAMP(sec)
#define RSQC_FIN_SECT(base, sec)
#define RSQC_FIN_BEGIN
#include "../../rnaseqc_amd/csrc/rsqc_k3.h"

using namespace rsqc;

// force: 0 = the classes the library would choose, 1 = every gene through the 1024-thread / 146 KB instance, 2 = through the
// 1024-thread / 64 KB one (longer genes scan in place in memory), 3 = 256 threads, 4 = one wave (genes beyond the instance's LDS
// capacity run its in-memory mode).  A forced configuration overrides the class counts the way RSQC_K3_FORCE does in the diagnostic
// build of the library (rsqc_finalize.cpp) and then goes through the same plan.
static void plan_for(const uint32_t *gene_coding, const uint32_t *order, uint32_t n, int force, K3Counts &c, K3Launch (&plan)[RSQC_K3_LAUNCHES]) {
    c = k3_count_classes(gene_coding, order, n);
    if (force == 1) { c.n_large = n; c.n_medium = 0; c.n_xlarge = n; } else if (force == 2) { c.n_large = n; c.n_medium = 0; c.n_xlarge = 0; }
    else if (force == 3) { c.n_large = 0; c.n_medium = n; c.n_xlarge = 0; } else if (force == 4) { c.n_large = 0; c.n_medium = 0; c.n_xlarge = 0; }
    k3_plan(n, c.n_large, c.n_medium, c.n_xlarge, c.n_le6144, c.n_le3072, c.n_le2048, c.n_le1024, plan);
}
static void plan_out(const K3Launch (&plan)[RSQC_K3_LAUNCHES], uint32_t *out /*[8][6]*/) {
    for (int k = 0; k < RSQC_K3_LAUNCHES; ++k) {
        const K3Launch &l = plan[k];
        const uint32_t row[6] = {l.threads, l.cov_bits, l.cap, l.count, l.first, l.stream};
        for (int j = 0; j < 6; ++j) out[k * 6 + j] = row[j];
    }
}

// the plan alone, from class counts as given (consistent or not): eight rows of {threads, bits of a depth in LDS, cap, count, first, stream slot}
extern "C" __attribute__((visibility("default")))
void k3emu_plan(uint32_t n, uint32_t n_large, uint32_t n_medium, uint32_t n_xlarge, uint32_t n_le6144, uint32_t n_le3072, uint32_t n_le2048,
                uint32_t n_le1024, uint32_t *out) {
    K3Launch plan[RSQC_K3_LAUNCHES];
    k3_plan(n, n_large, n_medium, n_xlarge, n_le6144, n_le3072, n_le2048, n_le1024, plan);
    plan_out(plan, out);
}
// ... from coding lengths, for `m` length vectors at once (row r: ns[r] lengths in lengths[r * width ...]): sorted longest first like
// gene_order, counted by k3_count_classes, `force` applied, then `delta` (null, or seven signed numbers per row added to {n_large, n_medium,
// n_xlarge, n_le6144, n_le3072, n_le2048, n_le1024}: counts that do not fit the lengths), then k3_plan.  Out: the counts the plan was made
// from, the plan (8 x 6 per row), the sorted lengths.
extern "C" __attribute__((visibility("default")))
void k3emu_plan_many(const uint32_t *lengths, const uint32_t *ns, uint32_t m, uint32_t width, int force, const int32_t *delta,
                     uint32_t *counts, uint32_t *out, uint32_t *sorted) {
    std::vector<uint32_t> len, order;
    for (uint32_t r = 0; r < m; ++r) {
        const uint32_t n = ns[r];
        len.assign(lengths + (size_t)r * width, lengths + (size_t)r * width + n);
        std::stable_sort(len.begin(), len.end(), [](uint32_t x, uint32_t y) { return x > y; });
        order.resize(n);
        for (uint32_t k = 0; k < n; ++k) { order[k] = k; sorted[(size_t)r * width + k] = len[k]; }
        K3Counts c; K3Launch plan[RSQC_K3_LAUNCHES];
        plan_for(len.data(), order.data(), n, force, c, plan);
        uint32_t cs[7] = {c.n_large, c.n_medium, c.n_xlarge, c.n_le6144, c.n_le3072, c.n_le2048, c.n_le1024};
        if (delta) {
            for (int j = 0; j < 7; ++j) cs[j] += (uint32_t)delta[(size_t)r * 7 + j];
            k3_plan(n, cs[0], cs[1], cs[2], cs[3], cs[4], cs[5], cs[6], plan);
        }
        for (int j = 0; j < 7; ++j) counts[(size_t)r * 7 + j] = cs[j];
        plan_out(plan, out + (size_t)r * RSQC_K3_LAUNCHES * 6);
    }
}

template <int WIN> static void run_plan(const GeneCovArgs &A, const K3Launch (&plan)[RSQC_K3_LAUNCHES]) {
    auto launch = [&](auto kernel, const K3Launch &l) {
        wavemu::grid_dim().x = l.count;
        for (uint32_t b = 0; b < l.count; ++b) { wavemu::block_idx().x = b; wavemu::run_block((int)l.threads, [&]() { kernel(A, l.first); }); }
    };
#define K3E_LAUNCH(K, T, COVT, CAP) \
    static_assert(T == K3_THREADS[K] && CAP == K3_CAPS[K] && sizeof(COVT) * 8 == K3_COV_BITS[K], "the instance its plan entry describes"); \
    launch(gene_coverage_kernel<T, WIN, COVT, CAP>, plan[K]);
    K3E_LAUNCH(0, 1024, uint16_t, RSQC_K3_LARGE_LDS16)
    K3E_LAUNCH(1, 256, uint32_t, RSQC_K3_MEDIUM_MAX)
    K3E_LAUNCH(2, 256, uint32_t, 6144)
    K3E_LAUNCH(3, 1024, uint16_t, RSQC_K3_LARGE2_LDS16)
    K3E_LAUNCH(4, 64, uint32_t, RSQC_K3_SMALL_MAX)
    K3E_LAUNCH(5, 64, uint32_t, 3072)
    K3E_LAUNCH(6, 64, uint32_t, 2048)
    K3E_LAUNCH(7, 64, uint32_t, 1024)
#undef K3E_LAUNCH
}

extern "C" __attribute__((visibility("default")))
int k3emu_run(const rsqc_params *p, const rsqc_annotation *a, const uint32_t *cov_diff, const uint64_t *gene_reads, int force,
              double *g_mean, double *g_std, double *g_cv, uint8_t *g_valid, double *e_cv, uint8_t *e_cv_valid,
              uint64_t *bias3, uint64_t *bias5, uint64_t *stats /*[8]: genes per launch, in launch order*/) {
    HostIndex hx; std::string err;
    int rc = hx.build(a, nullptr, err);
    if (rc) return rc;
    const int L = a->n_genes_listed;
    if (hx.ex_rows.empty()) hx.ex_rows.push_back(ExonRow{0, 0, 0, 0});
    std::vector<uint32_t> cov(cov_diff, cov_diff + hx.cov_entries);           // (the in-memory mode scans in place)
    std::vector<uint32_t> ex_id(a->exon_row_id, a->exon_row_id + a->n_exons); if (ex_id.empty()) ex_id.push_back(0);
    std::vector<uint32_t> order((size_t)std::max(L, 1), 0);
    for (int g = 0; g < L; ++g) order[(size_t)g] = (uint32_t)g;
    std::stable_sort(order.begin(), order.begin() + L, [&](uint32_t x, uint32_t y) { return hx.gene_coding[x] > hx.gene_coding[y]; });
    std::vector<unsigned long long> reads(gene_reads, gene_reads + std::max(L, 1)), b3((size_t)std::max(L, 1), 0ull), b5((size_t)std::max(L, 1), 0ull);
    int error = 0;
    GeneCovArgs A{};
    A.ge_off = a->gene_exon_off; A.ge_row = a->gene_exon_row; A.ex = hx.ex_rows.data(); A.ex_cov = hx.ex_cov.data(); A.ex_id = ex_id.data();
    A.gene_cov_off = hx.gene_cov_off.data(); A.gene_coding = hx.gene_coding.data(); A.gene_flags = hx.gene_flags.data(); A.gene_owned = hx.gene_owned.data();
    A.gene_order = order.data(); A.gene_reads = reads.data(); A.cov = cov.data(); A.n_listed = L;
    A.mask = p->coverage_mask; A.bias_offset = p->bias_offset; A.bias_window = p->bias_window; A.bias_gene_length = p->bias_gene_length;
    A.g_mean = g_mean; A.g_std = g_std; A.g_cv = g_cv; A.g_valid = g_valid; A.e_cv = e_cv; A.e_cv_valid = e_cv_valid;
    A.bias3 = b3.data(); A.bias5 = b5.data(); A.error = &error;
    if (A.bias_window < 1 || A.bias_window > RSQC_MAX_BIAS_WINDOW) return RSQC_ERR_ARG;                      // (as rsqc_create)
    K3Counts c; K3Launch plan[RSQC_K3_LAUNCHES];
    plan_for(hx.gene_coding.data(), order.data(), (uint32_t)L, force, c, plan);
    if (L > 0) { if (A.bias_window > 128) run_plan<RSQC_MAX_BIAS_WINDOW>(A, plan); else run_plan<128>(A, plan); }   // (wide: launch_gene_coverage)
    for (int g = 0; g < L; ++g) { bias3[g] = b3[(size_t)g]; bias5[g] = b5[(size_t)g]; }
    if (stats) for (int k = 0; k < RSQC_K3_LAUNCHES; ++k) stats[k] = plan[k].count;
    return error;
}
