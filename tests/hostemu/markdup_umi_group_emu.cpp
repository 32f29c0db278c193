// markdup_umi_group_emu.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// The stage of --mark-duplicates with UMIs one substitution apart grouped (rsqc_markdup_umi_edits(1)): the kernels of
// rnaseqc_amd/csrc/rsqc_markdup.h -- mark, signature, umi_keys, permute, heads_umi, heads_pos, group_nodes, group_parents, group_roots,
// group_marks, list, insert, apply -- and the collecting kernel, radix pass and scan of rsqc_sort.h, unmodified, on the 64-lane fiber
// emulation of wavemu.h.  The host side of rsqc_markdup_api.cpp in that mode (the four LSD stages, the two scans of the marks, which
// buffers of the sort the node columns reuse) is restated here with plain memory and a guard word behind every column.
// The expected verdicts, figures and roots are NOT computed here: tests/markdup_umi_group_ref.py restates the contract in Python.
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
constexpr uint64_t kNoAnchor = ~0ull;
struct State {
    bool two = false, first = true;
    std::vector<rsqc_rec_core> core; std::vector<rsqc_rec_aux> aux; std::vector<uint32_t> qh2, cigar; std::vector<uint64_t> key, umi;
    std::vector<uint64_t> wide_index; std::vector<int32_t> wide_nm, wide_lq; std::vector<uint32_t> wide_nc;
    std::vector<uint64_t> batch_rec0, batch_pool0;
    std::vector<uint8_t> verdict;
    std::vector<uint64_t> root;                        // per record: the root key of an anchor, kNoAnchor otherwise
} S;
}  // namespace

#define EMU_API extern "C" __attribute__((visibility("default")))

EMU_API void mdgemu_set_schedule_seed(unsigned long long seed) { wavemu::set_seed(seed); }

EMU_API void mdgemu_begin() { S = State{}; }

// one batch collected with its umi column.  Returns 1 when batches with and without qhash2 are mixed, 2 for a batch without the column
EMU_API int mdgemu_add_batch(const rsqc_rec_core *core, const rsqc_rec_aux *aux, const uint32_t *qhash2, const uint64_t *umi, uint64_t n, const uint32_t *cigar, uint64_t n_ops,
                             const int32_t *seg_tid, const uint64_t *seg_start, uint32_t n_seg, const uint64_t *wide_index, const int32_t *wide_nm, const int32_t *wide_lq,
                             const uint32_t *wide_nc, uint32_t n_wide) {
    if (!n) return 0;
    if (!umi) return 2;
    if (S.first) { S.two = qhash2 != nullptr; S.first = false; }
    else if (S.two != (qhash2 != nullptr)) return 1;
    const uint64_t n0 = S.core.size(), w0 = S.wide_index.size();
    S.batch_rec0.push_back(n0); S.batch_pool0.push_back(S.cigar.size());
    S.core.insert(S.core.end(), core, core + n); S.aux.insert(S.aux.end(), aux, aux + n); S.umi.insert(S.umi.end(), umi, umi + n);
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

// the stage of markdup_run under rsqc_markdup_umi_edits(1).  stats: [0] records, [1] population, [2] anchors, [3] sets, [4] duplicate
// fragments, [5] flagged records, [6] cleared records, [7] anchors with a UMI, [8] position duplicate fragments, [9] slots of the name
// table, [10] nodes, [11] merged nodes, [12] exact duplicate fragments, [13] keys looked up, [14] position sets.  smallest_key_parent != 0
// replaces the parents kernel by a WRONG rule on purpose -- the eligible neighbour with the smallest key instead of the highest count --
// so that the test can show that its catalogue tells the two apart.  Returns 0, or 4000 + k for check k of the harness itself
EMU_API int mdgemu_end(uint64_t *stats, int smallest_key_parent) {
    const uint64_t N = S.core.size();
    for (int k = 0; k < 15; ++k) stats[k] = 0;
    stats[0] = N;
    S.verdict.assign((size_t)N + 1, kGuard8);
    S.root.assign((size_t)N, kNoAnchor);
    if (!N) return 0;
    std::vector<uint64_t> tab(S.batch_rec0);
    tab.push_back(N);
    const size_t nb = S.batch_rec0.size();
    tab.insert(tab.end(), S.batch_pool0.begin(), S.batch_pool0.end());
    unsigned long long counters[9] = {0, 0, 0, 0, 0, 0, 0, 0, kGuard64};
    MarkdupCollection C{};
    C.core = S.core.data(); C.aux = S.aux.data(); C.qhash2 = S.two ? S.qh2.data() : nullptr; C.key = S.key.data(); C.cigar = S.cigar.data(); C.n = N;
    C.batch_rec0 = tab.data(); C.batch_pool0 = tab.data() + nb + 1; C.n_batches = (uint32_t)nb;
    C.wide_index = S.wide_index.data(); C.wide_n_cigar = S.wide_nc.data(); C.n_wide = S.wide_index.size(); C.n_ops = S.cigar.size();
    C.umi = S.umi.data();
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
        std::vector<uint64_t> k_hi((size_t)A + 1, kGuard64), k_lo((size_t)A + 1, kGuard64), k_umi((size_t)A + 1, kGuard64);
        std::vector<uint32_t> ci((size_t)A + 1, kGuard32);
        for (int h = 0; h < 2; ++h) { kb[h].assign((size_t)A + 1, kGuard64); ib[h].assign((size_t)A + 1, kGuard32); }
        launch(blocks, [&]() { markdup_signature_kernel(C, block_anchors.data(), A, k_hi.data(), k_lo.data(), kb[0].data(), ci.data()); });
        if (k_hi[(size_t)A] != kGuard64 || k_lo[(size_t)A] != kGuard64 || ci[(size_t)A] != kGuard32 || kb[0][(size_t)A] != kGuard64) return 4003;
        for (uint64_t s = 0; s < A; ++s) if (ci[(size_t)s] == kGuard32 && N <= kGuard32) return 4004;
        launch(blocks_for(A, RSQC_MD_THREADS), [&]() { markdup_umi_keys_kernel(C, ci.data(), A, k_umi.data(), counters); });
        if (k_umi[(size_t)A] != kGuard64) return 4014;
        for (uint64_t s = 0; s < A; ++s) if (k_umi[(size_t)s] != S.umi[ci[(size_t)s]]) return 4015;
        const uint32_t prep_grid = std::min<uint32_t>(3, blocks_for(A, RSQC_SORT_THREADS));
        std::vector<unsigned long long> part((size_t)prep_grid * 9, 0);
        launch(prep_grid, [&]() { sort_prepare_kernel(k_umi.data(), A, ib[1].data(), part.data() + (size_t)prep_grid * 6); });
        launch(prep_grid, [&]() { sort_prepare_kernel(k_hi.data(), A, ib[1].data(), part.data() + (size_t)prep_grid * 3); });
        launch(prep_grid, [&]() { sort_prepare_kernel(kb[0].data(), A, ib[0].data(), part.data()); });
        uint64_t oa[3][2] = {{0, ~0ull}, {0, ~0ull}, {0, ~0ull}};
        for (int h = 0; h < 3; ++h)
            for (uint32_t k = 0; k < prep_grid; ++k) { oa[h][0] |= part[(size_t)h * prep_grid * 3 + 3 * k]; oa[h][1] &= part[(size_t)h * prep_grid * 3 + 3 * k + 1]; }
        int shift[8], shift_u[8], kc = 0, ic = 0, err = 0;
        auto passes = [&](int n, const int *sh) {
            for (int p = 0; p < n && !err; ++p) {
                if (!emu_pass(kb[kc].data(), ib[ic].data(), kb[kc ^ 1].data(), ib[ic ^ 1].data(), A, sh[p], hist, chunk_sum)) { err = 4005; return; }
                kc ^= 1; ic ^= 1;
            }
        };
        auto gather = [&](const std::vector<uint64_t> &src) { launch(blocks_for(A, RSQC_MD_THREADS), [&]() { markdup_permute_kernel(src.data(), ib[ic].data(), A, kb[kc].data()); }); };
        const int n_lo_all = sort_live_digits(oa[0][0], oa[0][1], shift);
        const int n_umi = sort_live_digits(oa[2][0], oa[2][1], shift_u);
        const int n_mapq = (n_lo_all && shift[0] == 0) ? 1 : 0;
        passes(n_mapq, shift);
        if (n_umi) { gather(k_umi); passes(n_umi, shift_u); }
        if (n_lo_all - n_mapq) { gather(k_lo); passes(n_lo_all - n_mapq, shift + n_mapq); }
        if (err) return err;
        kc ^= 1;
        gather(k_hi);
        const int n_hi = sort_live_digits(oa[1][0], oa[1][1], shift);
        passes(n_hi, shift);
        if (err) return 4006;
        for (int h = 0; h < 2; ++h) if (kb[h][(size_t)A] != kGuard64 || ib[h][(size_t)A] != kGuard32) return 4007;
        // the order the heads rely on: (K_hi, K_lo >> 8, umi, 255 - mapq, arrival)
        for (uint64_t r = 1; r < A; ++r) {
            const uint32_t s = ib[ic][(size_t)r], p = ib[ic][(size_t)(r - 1)];
            if (s >= A || p >= A) return 4016;
            const uint64_t a[5] = {k_hi[p], k_lo[p] >> 8, k_umi[p], k_lo[p] & 0xFF, p}, b[5] = {k_hi[s], k_lo[s] >> 8, k_umi[s], k_lo[s] & 0xFF, s};
            if (!std::lexicographical_compare(a, a + 5, b, b + 5)) return 4017;
        }
        uint32_t *mark = ib[ic ^ 1].data(), *list = (uint32_t *)kb[kc ^ 1].data();
        launch(blocks_for(A, RSQC_MD_THREADS), [&]() { markdup_heads_umi_kernel(kb[kc].data(), ib[ic].data(), k_lo.data(), k_umi.data(), A, mark, counters); });
        // ---- the grouping, with the buffers rsqc_markdup_api.cpp gives it: node keys in the keys' free buffer (the list follows them
        // there), the nodes' best anchors over the sorted K_hi, the groups' best over K_hi by slot, parent and root in the halves of k_umi
        std::vector<uint32_t> mark_pos((size_t)A + 1, kGuard32), node_head((size_t)A + 2, kGuard32), node_set((size_t)A + 1, kGuard32), set_first((size_t)A + 2, kGuard32);
        launch(blocks_for(A, RSQC_MD_THREADS), [&]() { markdup_heads_pos_kernel(kb[kc].data(), ib[ic].data(), k_lo.data(), A, mark_pos.data()); });
        unsigned long long tot[2] = {0, 0};
        emu_scan(mark, A, chunk_sum, &tot[0]);
        emu_scan(mark_pos.data(), A, chunk_sum, &tot[1]);
        if (tot[0] >= A || tot[1] >= A || tot[0] > tot[1]) return 4020;
        const uint32_t n_nodes = (uint32_t)(A - tot[0]), n_sets = (uint32_t)(A - tot[1]);
        uint64_t *node_key = kb[kc ^ 1].data(), *node_best = kb[kc].data();
        unsigned long long *group_best = (unsigned long long *)k_hi.data();
        uint32_t *parent = (uint32_t *)k_umi.data(), *root = parent + A;
        launch(blocks_for(A, RSQC_MD_THREADS), [&]() {
            markdup_group_nodes_kernel(mark, mark_pos.data(), tot, ib[ic].data(), k_lo.data(), k_umi.data(), A, node_key, node_head.data(), node_best, node_set.data(), set_first.data(), group_best);
        });
        if (node_head[n_nodes] != A || node_head[(size_t)n_nodes + 1] != kGuard32 || set_first[n_sets] != n_nodes || set_first[(size_t)n_sets + 1] != kGuard32 || node_set[n_nodes] != kGuard32) return 4021;
        for (uint32_t m = 0; m < n_nodes; ++m) {         // every node written, heads and sets ascending, keys ascending inside a set
            if (node_head[m] >= node_head[m + 1] || node_set[m] >= n_sets || (m && node_set[m] < node_set[m - 1])) return 4022;
            if (m && node_set[m] == node_set[m - 1] && node_key[m] <= node_key[m - 1]) return 4023;
            if (set_first[node_set[m]] > m || set_first[node_set[m] + 1] <= m || group_best[m] != ~0ull) return 4024;
        }
        if (smallest_key_parent) {                     // the WRONG rule, in plain loops
            for (uint32_t m = 0; m < n_nodes; ++m) {
                parent[m] = RSQC_MD_EMPTY;
                const uint64_t k = node_key[m], c = node_head[m + 1] - node_head[m];
                if (!k) continue;
                const int L = (63 - __builtin_clzll(k)) >> 1;
                for (uint32_t q = set_first[node_set[m]]; q < set_first[node_set[m] + 1]; ++q) {       // ascending keys: the first eligible one is the smallest
                    const uint64_t d = node_key[q] ^ k, cq = node_head[q + 1] - node_head[q];
                    bool one = false;
                    for (int j = 0; j < L; ++j) one = one || (d != 0 && (d & ~(3ull << (2 * j))) == 0);
                    if (node_key[q] && one && cq >= 2 * c - 1 && (cq > c || (cq == c && node_key[q] < k))) { parent[m] = q; break; }
                }
                if (parent[m] != RSQC_MD_EMPTY) ++counters[5];
            }
            counters[6] += n_nodes;
        } else
            launch(blocks_for(n_nodes, RSQC_MD_THREADS), [&]() { markdup_group_parents_kernel(node_key, node_head.data(), node_set.data(), set_first.data(), n_nodes, n_sets, parent, counters); });
        if (counters[6] != n_nodes) return 4025;
        launch(blocks_for(n_nodes, RSQC_MD_THREADS), [&]() { markdup_group_roots_kernel(parent, node_set.data(), set_first.data(), node_best, n_nodes, n_sets, root, group_best); });
        for (uint32_t m = 0; m < n_nodes; ++m) if (root[m] >= n_nodes || parent[root[m]] != RSQC_MD_EMPTY || node_set[root[m]] != node_set[m]) return 4026;
        launch(blocks_for(A, RSQC_MD_THREADS), [&]() { markdup_group_marks_kernel(mark, tot, ib[ic].data(), k_lo.data(), root, group_best, A, n_nodes, mark_pos.data()); });
        if (mark_pos[(size_t)A] != kGuard32 || k_hi[(size_t)A] != kGuard64 || k_umi[(size_t)A] != kGuard64) return 4027;
        for (uint64_t r = 0, node = 0; r < A; ++r) {    // per record the root key of its anchor (the list below takes the node keys' buffer)
            if (r && node + 1 < n_nodes && node_head[node + 1] == r) ++node;
            S.root[ci[ib[ic][(size_t)r]]] = node_key[root[node]];
        }
        stats[10] = n_nodes; stats[11] = counters[5]; stats[12] = tot[0]; stats[13] = counters[7]; stats[14] = n_sets;
        mark = mark_pos.data();
        emu_scan(mark, A, chunk_sum, &n_dup);
        if (n_dup != tot[0] + counters[5] || counters[4] < n_dup) return 4028;
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
    if (S.verdict[(size_t)N] != kGuard8 || counters[8] != kGuard64) return 4012;
    for (uint64_t i = 0; i < N; ++i) if (S.verdict[(size_t)i] > 1) return 4013;
    stats[5] = counters[1]; stats[6] = counters[2]; stats[7] = counters[3]; stats[8] = counters[4];
    return 0;
}

// the verdict bytes, the flags the records leave with and the root keys (all ones: not an anchor), in arrival order
EMU_API void mdgemu_rows(uint8_t *verdict, uint16_t *flag, uint64_t *root) {
    const size_t n = S.core.size();
    for (size_t i = 0; i < n; ++i) { verdict[i] = S.verdict[i]; flag[i] = S.aux[i].flag; root[i] = S.root[i]; }
}
