// markdup_emu.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// The KERNELS of --mark-duplicates -- rnaseqc_amd/csrc/rsqc_markdup.h (mark, signature, permute, heads, list, insert, apply) and the
// collecting kernel, radix pass and scan of rnaseqc_amd/csrc/rsqc_sort.h they work with, unmodified -- compiled for the host on top of
// the 64-lane fiber emulation of wavemu.h.  The host side of rsqc_sort_api.cpp (collecting a batch) and of rsqc_markdup_api.cpp (which
// digit positions run, the two stages and their ping-pong, the buffers the marks and the list reuse, the table's size) is restated here
// with plain memory and a guard word behind every column.  The expected verdicts are NOT computed here: tests/markdup_ref.py restates
// the contract in Python and the test compares.
#include "wavemu.h"

#include <algorithm>
#include <vector>

#include "../../rnaseqc_amd/csrc/rsqc_sort.h"
#include "../../rnaseqc_amd/csrc/rsqc_markdup.h"

using namespace rsqc;

namespace {
template <class F> void launch(uint32_t grid, F &&body) {
    wavemu::grid_dim().x = grid;
    for (uint32_t b = 0; b < grid; ++b) { wavemu::block_idx().x = b; wavemu::run_block(RSQC_SORT_THREADS, body); }
}
uint32_t blocks_for(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

void emu_scan(uint32_t *data, uint64_t m, std::vector<unsigned long long> &chunk_sum, unsigned long long *total) {
    const uint32_t chunks = blocks_for(m, RSQC_SCAN_CHUNK);
    chunk_sum.assign((size_t)chunks + 1, 0xDEADull);
    if (chunks) launch(chunks, [&]() { sort_scan_sum_kernel(data, m, chunk_sum.data()); });
    launch(1, [&]() { sort_scan_top_kernel(chunk_sum.data(), chunks, total); });
    if (chunks) launch(chunks, [&]() { sort_scan_apply_kernel(data, m, chunk_sum.data()); });
}
// one stable pass (launch_sort_pass): false when the histogram does not add up
bool emu_pass(const uint64_t *kin, const uint32_t *iin, uint64_t *kout, uint32_t *iout, uint64_t n, int sh, std::vector<uint32_t> &hist, std::vector<unsigned long long> &chunk_sum) {
    const uint32_t tiles = blocks_for(n, RSQC_SORT_TILE);
    hist.assign((size_t)256 * tiles, 0);
    unsigned long long total = 0;
    launch(tiles, [&]() { sort_hist_kernel(kin, n, sh, hist.data(), tiles); });
    emu_scan(hist.data(), (uint64_t)256 * tiles, chunk_sum, &total);
    if (total != n) return false;
    launch(tiles, [&]() { sort_scatter_kernel(kin, iin, kout, iout, n, sh, hist.data(), tiles); });
    return true;
}

constexpr uint64_t kGuard64 = 0xA5A5A5A5A5A5A5A5ull;
constexpr uint32_t kGuard32 = 0xA5A5A5A5u;
constexpr uint8_t kGuard8 = 0xA5u;
struct State {
    bool two = false, first = true;                    // the pass has a qhash2 column
    std::vector<rsqc_rec_core> core; std::vector<rsqc_rec_aux> aux; std::vector<uint32_t> qh2, cigar; std::vector<uint64_t> key;
    std::vector<uint64_t> wide_index; std::vector<int32_t> wide_nm, wide_lq; std::vector<uint32_t> wide_nc;
    std::vector<uint64_t> batch_rec0, batch_pool0;
    std::vector<uint8_t> verdict;
} S;
}  // namespace

#define EMU_API extern "C" __attribute__((visibility("default")))

EMU_API void mdemu_set_schedule_seed(unsigned long long seed) { wavemu::set_seed(seed); }

EMU_API void mdemu_begin() { S = State{}; }

// one batch collected: the copies of sort_append (rsqc_sort_api.cpp) and its kernel.  Returns 1 when batches with and without qhash2 are mixed
EMU_API int mdemu_add_batch(const rsqc_rec_core *core, const rsqc_rec_aux *aux, const uint32_t *qhash2, uint64_t n, const uint32_t *cigar, uint64_t n_ops,
                            const int32_t *seg_tid, const uint64_t *seg_start, uint32_t n_seg, const uint64_t *wide_index, const int32_t *wide_nm, const int32_t *wide_lq,
                            const uint32_t *wide_nc, uint32_t n_wide) {
    if (!n) return 0;
    if (S.first) { S.two = qhash2 != nullptr; S.first = false; }
    else if (S.two != (qhash2 != nullptr)) return 1;
    const uint64_t n0 = S.core.size(), w0 = S.wide_index.size();
    S.batch_rec0.push_back(n0); S.batch_pool0.push_back(S.cigar.size());
    S.core.insert(S.core.end(), core, core + n); S.aux.insert(S.aux.end(), aux, aux + n);
    if (qhash2) S.qh2.insert(S.qh2.end(), qhash2, qhash2 + n);
    S.cigar.insert(S.cigar.end(), cigar, cigar + n_ops);
    S.key.resize((size_t)(n0 + n)); S.wide_index.resize((size_t)(w0 + n_wide)); S.wide_nm.resize((size_t)(w0 + n_wide)); S.wide_lq.resize((size_t)(w0 + n_wide)); S.wide_nc.resize((size_t)(w0 + n_wide));
    const uint64_t lanes = std::max<uint64_t>(n, n_wide);
    launch(blocks_for(lanes, RSQC_SORT_THREADS), [&]() {
        sort_append_kernel(core, n, seg_tid, seg_start, n_seg, S.key.data() + n0, n0, wide_index, wide_nm, wide_lq, wide_nc, n_wide,
                           S.wide_index.data() + w0, S.wide_nm.data() + w0, S.wide_lq.data() + w0, S.wide_nc.data() + w0);
    });
    return 0;
}

// the stage of markdup_run.  stats: [0] records, [1] population, [2] anchors, [3] sets, [4] duplicate fragments, [5] flagged records,
// [6] cleared records, [7] passes of stage 1, [8] of stage 2, [9] slots of the name table (0: none).  Returns 0, or 4000 + k for check k
// of the harness itself
EMU_API int mdemu_end(uint64_t *stats) {
    const uint64_t N = S.core.size();
    for (int k = 0; k < 10; ++k) stats[k] = 0;
    stats[0] = N;
    S.verdict.assign((size_t)N + 1, kGuard8);
    if (!N) return 0;
    std::vector<uint64_t> tab(S.batch_rec0);
    tab.push_back(N);
    const size_t nb = S.batch_rec0.size();
    tab.insert(tab.end(), S.batch_pool0.begin(), S.batch_pool0.end());
    unsigned long long counters[4] = {0, 0, 0, kGuard64};
    MarkdupCollection C{};
    C.core = S.core.data(); C.aux = S.aux.data(); C.qhash2 = S.two ? S.qh2.data() : nullptr; C.key = S.key.data(); C.cigar = S.cigar.data(); C.n = N;
    C.batch_rec0 = tab.data(); C.batch_pool0 = tab.data() + nb + 1; C.n_batches = (uint32_t)nb;
    C.wide_index = S.wide_index.data(); C.wide_n_cigar = S.wide_nc.data(); C.n_wide = S.wide_index.size(); C.n_ops = S.cigar.size();
    const uint32_t blocks = blocks_for(N, RSQC_MD_THREADS);
    std::vector<uint32_t> block_anchors((size_t)blocks + 1, kGuard32);
    std::vector<unsigned long long> chunk_sum;
    std::vector<uint32_t> hist;
    launch(blocks, [&]() { markdup_mark_kernel(C, block_anchors.data(), counters); });
    unsigned long long A = 0;
    emu_scan(block_anchors.data(), blocks, chunk_sum, &A);
    if (block_anchors[blocks] != kGuard32) return 4001;
    if (A > N || counters[0] > N || A > counters[0]) return 4002;
    stats[1] = counters[0]; stats[2] = A;
    unsigned long long n_dup = 0;
    std::vector<uint64_t> kb[2]; std::vector<uint32_t> ib[2];
    const uint32_t *d_list = nullptr;
    if (A) {
        std::vector<uint64_t> k_hi((size_t)A + 1, kGuard64), k_lo((size_t)A + 1, kGuard64);
        std::vector<uint32_t> ci((size_t)A + 1, kGuard32);
        for (int h = 0; h < 2; ++h) { kb[h].assign((size_t)A + 1, kGuard64); ib[h].assign((size_t)A + 1, kGuard32); }
        launch(blocks, [&]() { markdup_signature_kernel(C, block_anchors.data(), A, k_hi.data(), k_lo.data(), kb[0].data(), ci.data()); });
        if (k_hi[(size_t)A] != kGuard64 || k_lo[(size_t)A] != kGuard64 || ci[(size_t)A] != kGuard32 || kb[0][(size_t)A] != kGuard64) return 4003;
        for (uint64_t s = 0; s < A; ++s) if (ci[(size_t)s] == kGuard32 && N <= kGuard32) return 4004;       // a slot nobody wrote
        const uint32_t prep_grid = std::min<uint32_t>(3, blocks_for(A, RSQC_SORT_THREADS));
        std::vector<unsigned long long> part((size_t)prep_grid * 6, 0);
        launch(prep_grid, [&]() { sort_prepare_kernel(k_hi.data(), A, ib[1].data(), part.data() + (size_t)prep_grid * 3); });
        launch(prep_grid, [&]() { sort_prepare_kernel(kb[0].data(), A, ib[0].data(), part.data()); });
        uint64_t oa[2][2] = {{0, ~0ull}, {0, ~0ull}};
        for (int h = 0; h < 2; ++h)
            for (uint32_t k = 0; k < prep_grid; ++k) { oa[h][0] |= part[(size_t)h * prep_grid * 3 + 3 * k]; oa[h][1] &= part[(size_t)h * prep_grid * 3 + 3 * k + 1]; }
        int shift[8], kc = 0, ic = 0;
        const int n_lo = sort_live_digits(oa[0][0], oa[0][1], shift);
        for (int p = 0; p < n_lo; ++p) {
            if (!emu_pass(kb[kc].data(), ib[ic].data(), kb[kc ^ 1].data(), ib[ic ^ 1].data(), A, shift[p], hist, chunk_sum)) return 4005;
            kc ^= 1; ic ^= 1;
        }
        kc ^= 1;
        launch(blocks_for(A, RSQC_MD_THREADS), [&]() { markdup_permute_kernel(k_hi.data(), ib[ic].data(), A, kb[kc].data()); });
        const int n_hi = sort_live_digits(oa[1][0], oa[1][1], shift);
        for (int p = 0; p < n_hi; ++p) {
            if (!emu_pass(kb[kc].data(), ib[ic].data(), kb[kc ^ 1].data(), ib[ic ^ 1].data(), A, shift[p], hist, chunk_sum)) return 4006;
            kc ^= 1; ic ^= 1;
        }
        stats[7] = (uint64_t)n_lo; stats[8] = (uint64_t)n_hi;
        for (int h = 0; h < 2; ++h) if (kb[h][(size_t)A] != kGuard64 || ib[h][(size_t)A] != kGuard32) return 4007;       // a write past the columns
        uint32_t *mark = ib[ic ^ 1].data(), *list = (uint32_t *)kb[kc ^ 1].data();
        launch(blocks_for(A, RSQC_MD_THREADS), [&]() { markdup_heads_kernel(kb[kc].data(), ib[ic].data(), k_lo.data(), A, mark); });
        emu_scan(mark, A, chunk_sum, &n_dup);
        launch(blocks_for(A, RSQC_MD_THREADS), [&]() { markdup_list_kernel(mark, &n_dup, ib[ic].data(), ci.data(), A, list); });
        for (int h = 0; h < 2; ++h) if (kb[h][(size_t)A] != kGuard64 || ib[h][(size_t)A] != kGuard32) return 4008;
        if (n_dup >= A) return 4009;
        d_list = list;
    }
    stats[3] = A - n_dup; stats[4] = n_dup;
    std::vector<uint32_t> table;
    uint32_t mask = 0;
    if (n_dup) {
        const uint64_t slots = markdup_table_size(n_dup);
        if (slots < 2 * n_dup || slots < 1024 || (slots & (slots - 1))) return 4010;
        table.assign((size_t)slots + 1, RSQC_MD_EMPTY);
        table[(size_t)slots] = kGuard32;
        mask = (uint32_t)(slots - 1);
        stats[9] = slots;
        launch(blocks_for(n_dup, RSQC_MD_THREADS), [&]() { markdup_insert_kernel(C, d_list, n_dup, table.data(), mask); });
        if (table[(size_t)slots] != kGuard32) return 4011;
    }
    launch(blocks, [&]() { markdup_apply_kernel(C, d_list, n_dup, n_dup ? table.data() : nullptr, mask, S.verdict.data(), counters); });
    if (S.verdict[(size_t)N] != kGuard8 || counters[3] != kGuard64) return 4012;
    for (uint64_t i = 0; i < N; ++i) if (S.verdict[(size_t)i] > 1) return 4013;
    stats[5] = counters[1]; stats[6] = counters[2];
    return 0;
}

// the verdict bytes and the flags the records leave with, in arrival order
EMU_API void mdemu_rows(uint8_t *verdict, uint16_t *flag) {
    const size_t n = S.core.size();
    for (size_t i = 0; i < n; ++i) { verdict[i] = S.verdict[i]; flag[i] = S.aux[i].flag; }
}
