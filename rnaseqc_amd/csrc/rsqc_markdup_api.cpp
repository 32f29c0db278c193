// rsqc_markdup_api.cpp -- rsqc_markdup_begin / rsqc_markdup_end / rsqc_markdup_verdicts: duplicate fragments are found on the complete
// collection of rsqc_sort_begin and flag 0x400 of every record is rewritten, at the head of rsqc_sort_end (markdup_run, called by
// rsqc_sort_api.cpp).  The kernels are rsqc_markdup.hip's, the order is made with the radix passes of --sort (rsqc_sort.hip).
#include "rsqc_ctx.h"
#include "rsqc_markdup.h"
#include "rsqc_sort.h"

namespace {

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

int alloc_or_capacity(rsqc_ctx *c, DevBuf &b, size_t bytes, const char *what, uint64_t anchors) {
    if (dev_reserve(b, bytes)) return 0;
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    return fail(c, RSQC_ERR_CAPACITY, std::string("rsqc_sort_end: no device memory for ") + what + " of the duplicate marking (" + std::to_string(bytes >> 20) + " MiB; " +
                                          std::to_string(c->sort.n) + " records collected, " + std::to_string(anchors) + " anchors, " + std::to_string(free_b >> 20) + " MiB of " +
                                          std::to_string(total_b >> 20) + " MiB free)");
}

// scratch of the stage: released before markdup_run returns, so before the coordinate sort allocates
struct Scratch {
    DevBuf batch_tab, block_anchors, counters, totals, chunk_sum, k_hi, k_lo, ci, key0, key1, idx0, idx1, hist, part, table;
    DevBuf k_umi;                                      // rsqc_markdup_use_umi only: the anchors' UMI keys by slot
    DevBuf g_mark, g_head, g_set, g_first;             // rsqc_markdup_umi_edits(1) only: position marks (then the final marks), node head ranks, node sets, first node of a set
    size_t bytes() { size_t n = 0; for (DevBuf *b : {&batch_tab, &block_anchors, &counters, &totals, &chunk_sum, &k_hi, &k_lo, &ci, &key0, &key1, &idx0, &idx1, &hist, &part, &table, &k_umi, &g_mark, &g_head, &g_set, &g_first}) n += b->bytes; return n; }
    void release() { for (DevBuf *b : {&batch_tab, &block_anchors, &counters, &totals, &chunk_sum, &k_hi, &k_lo, &ci, &key0, &key1, &idx0, &idx1, &hist, &part, &table, &k_umi, &g_mark, &g_head, &g_set, &g_first}) b->release(); }
};

int markdup_stage(rsqc_ctx *c, Scratch &X) {
    SortState &S = c->sort;
    MarkdupState &M = c->markdup;
    rsqc_markdup_info &info = M.info;
    const uint64_t N = S.n;
    int rc;
    // ---- what the kernels read: the collection, the batch table for the CIGAR pools
    std::vector<uint64_t> tab(S.batch_rec0);
    tab.push_back(N);
    const size_t nb = S.batch_rec0.size();
    tab.insert(tab.end(), S.batch_pool0.begin(), S.batch_pool0.end());
    const uint64_t blocks = (N + RSQC_MD_THREADS - 1) / RSQC_MD_THREADS;
    if ((rc = alloc_or_capacity(c, M.verdict, (size_t)N + 64, "the verdict column", 0)) || (rc = alloc_or_capacity(c, X.batch_tab, tab.size() * 8 + 64, "the batch table", 0)) ||
        (rc = alloc_or_capacity(c, X.block_anchors, (size_t)blocks * 4 + 64, "the anchor counts", 0)) || (rc = alloc_or_capacity(c, X.counters, 64, "the counters", 0)) ||
        (rc = alloc_or_capacity(c, X.totals, 64, "the scan totals", 0)) ||
        (rc = alloc_or_capacity(c, X.chunk_sum, ((blocks + RSQC_SCAN_CHUNK - 1) / RSQC_SCAN_CHUNK + 1) * 8, "the scan's chunk sums", 0))) return rc;
    HIP_TRY(c, hipMemcpyAsync(X.batch_tab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(X.counters.p, 0, 64, c->stream));
    MarkdupCollection C{};
    C.core = (const rsqc_rec_core *)S.core.p; C.aux = (rsqc_rec_aux *)S.aux.p; C.qhash2 = c->name_mode == 1 ? (const uint32_t *)S.qh2.p : nullptr;
    C.key = (const uint64_t *)S.key.p; C.cigar = (const uint32_t *)S.cigar.p; C.n = N;
    C.batch_rec0 = (const uint64_t *)X.batch_tab.p; C.batch_pool0 = C.batch_rec0 + nb + 1; C.n_batches = (uint32_t)nb;
    C.wide_index = (const uint64_t *)S.wide_index.p; C.wide_n_cigar = (const uint32_t *)S.wide_nc.p; C.n_wide = S.n_wide; C.n_ops = S.n_ops;
    C.umi = M.use_umi ? (const uint64_t *)S.umi.p : nullptr;
    unsigned long long *d_cnt = (unsigned long long *)X.counters.p, *d_tot = (unsigned long long *)X.totals.p, *d_chunk = (unsigned long long *)X.chunk_sum.p;
    // ---- 1 mark, 2 signature (host clocks around kernels and the synchronisation behind them; allocations are outside them)
    auto t0 = std::chrono::steady_clock::now();
    launch_markdup_mark(c->stream, C, (uint32_t *)X.block_anchors.p, d_cnt);
    launch_sort_scan(c->stream, (uint32_t *)X.block_anchors.p, blocks, d_chunk, d_tot);
    unsigned long long A = 0, population = 0;
    HIP_TRY(c, hipMemcpyAsync(&A, d_tot, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&population, d_cnt, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    info.sig_ms = ms_since(t0);
    if (A > N || population > N || A > population) return fail(c, RSQC_ERR_HIP, "rsqc_sort_end: the anchor marks of the duplicate marking do not add up");
    info.population = population; info.anchors = A;
    unsigned long long n_dup = 0;
    const uint32_t *d_list = nullptr;
    if (A) {
        const uint64_t tiles = (A + RSQC_SORT_TILE - 1) / RSQC_SORT_TILE;
        const uint32_t prep_grid = (uint32_t)std::min<uint64_t>(RSQC_SORT_PREP_GRID, (A + RSQC_SORT_THREADS - 1) / RSQC_SORT_THREADS);
        const uint64_t scan_chunks = std::max<uint64_t>((256 * tiles + RSQC_SCAN_CHUNK - 1) / RSQC_SCAN_CHUNK, (A + RSQC_SCAN_CHUNK - 1) / RSQC_SCAN_CHUNK) + 1;
        if ((rc = alloc_or_capacity(c, X.k_hi, A * 8 + 64, "the K_hi column", A)) || (rc = alloc_or_capacity(c, X.k_lo, A * 8 + 64, "the K_lo column", A)) ||
            (rc = alloc_or_capacity(c, X.ci, A * 4 + 64, "the anchors' record indices", A)) || (rc = alloc_or_capacity(c, X.key0, A * 8 + 64, "the sort's key column", A)) ||
            (rc = alloc_or_capacity(c, X.key1, A * 8 + 64, "the sort's second key column", A)) || (rc = alloc_or_capacity(c, X.idx0, A * 4 + 64, "the sort's index column", A)) ||
            (rc = alloc_or_capacity(c, X.idx1, A * 4 + 64, "the sort's second index column", A)) || (rc = alloc_or_capacity(c, X.hist, 256 * tiles * 4 + 64, "the digit histograms", A)) ||
            (rc = alloc_or_capacity(c, X.chunk_sum, scan_chunks * 8, "the scan's chunk sums", A)) || (rc = alloc_or_capacity(c, X.part, (size_t)prep_grid * (M.use_umi ? 72 : 48), "the key reduction", A)) ||
            (M.use_umi && (rc = alloc_or_capacity(c, X.k_umi, A * 8 + 64, "the UMI key column", A)))) return rc;
        if (M.umi_edits && ((rc = alloc_or_capacity(c, X.g_mark, A * 4 + 64, "the position marks of the UMI grouping", A)) || (rc = alloc_or_capacity(c, X.g_head, A * 4 + 64, "the node heads of the UMI grouping", A)) ||
                            (rc = alloc_or_capacity(c, X.g_set, A * 4 + 64, "the node sets of the UMI grouping", A)) || (rc = alloc_or_capacity(c, X.g_first, A * 4 + 64, "the set starts of the UMI grouping", A)))) return rc;
        d_chunk = (unsigned long long *)X.chunk_sum.p;
        uint64_t *kbuf[2] = {(uint64_t *)X.key0.p, (uint64_t *)X.key1.p};
        uint32_t *ibuf[2] = {(uint32_t *)X.idx0.p, (uint32_t *)X.idx1.p};
        const uint64_t *k_hi = (const uint64_t *)X.k_hi.p, *k_lo = (const uint64_t *)X.k_lo.p;
        unsigned long long *d_part = (unsigned long long *)X.part.p;
        t0 = std::chrono::steady_clock::now();
        launch_markdup_signature(c->stream, C, (const uint32_t *)X.block_anchors.p, A, (uint64_t *)X.k_hi.p, (uint64_t *)X.k_lo.p, kbuf[0], (uint32_t *)X.ci.p);
        if (M.use_umi) launch_markdup_umi_keys(c->stream, C, (const uint32_t *)X.ci.p, A, (uint64_t *)X.k_umi.p, d_cnt);
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
        info.sig_ms += ms_since(t0);
        // ---- 3 sort: LSD over (K_hi, K_lo) in two stages of 64-bit radix passes, dead digit positions skipped in both.  OR and AND
        // of both parts in one read-back; the index column the second prepare call writes is scratch
        t0 = std::chrono::steady_clock::now();
        const uint64_t *k_umi = (const uint64_t *)X.k_umi.p;
        const int n_parts = M.use_umi ? 3 : 2;         // K_lo, K_hi and, in the UMI mode, the UMI keys
        if (M.use_umi) launch_sort_prepare(c->stream, k_umi, A, ibuf[1], d_part + (size_t)prep_grid * 6, prep_grid);
        launch_sort_prepare(c->stream, k_hi, A, ibuf[1], d_part + (size_t)prep_grid * 3, prep_grid);
        launch_sort_prepare(c->stream, kbuf[0], A, ibuf[0], d_part, prep_grid);
        std::vector<unsigned long long> part((size_t)prep_grid * 3 * (size_t)n_parts);
        HIP_TRY(c, hipMemcpyAsync(part.data(), X.part.p, part.size() * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
        uint64_t oa[3][2] = {{0, ~0ull}, {0, ~0ull}, {0, ~0ull}};
        for (int h = 0; h < n_parts; ++h)
            for (uint32_t k = 0; k < prep_grid; ++k) { oa[h][0] |= part[(size_t)h * prep_grid * 3 + 3 * k]; oa[h][1] &= part[(size_t)h * prep_grid * 3 + 3 * k + 1]; }
        int shift[8], kc = 0, ic = 0;                  // kbuf[kc] / ibuf[ic]: the current keys and payload
        auto passes = [&](int n, const int *sh) {
            for (int p = 0; p < n; ++p) {
                launch_sort_pass(c->stream, kbuf[kc], ibuf[ic], kbuf[kc ^ 1], ibuf[ic ^ 1], A, sh[p], (uint32_t *)X.hist.p, d_chunk, d_tot);
                kc ^= 1; ic ^= 1;
            }
        };
        int n_lo = sort_live_digits(oa[0][0], oa[0][1], shift);
        if (M.use_umi) {
            // the UMI ranks ABOVE the mapq byte: (K_hi, K_lo >> 8, umi, 255 - mapq, arrival).  LSD: the mapq byte alone, then the UMI keys, then
            // K_lo above its lowest byte -- each stage's keys gathered through the payload of the stage before, a stage without a live digit
            // skipped with its gather; K_hi follows below as ever
            const int n_mapq = (n_lo && shift[0] == 0) ? 1 : 0;
            passes(n_mapq, shift);
            int shift_u[8];
            const int n_umi = sort_live_digits(oa[2][0], oa[2][1], shift_u);
            if (n_umi) { launch_markdup_permute(c->stream, k_umi, ibuf[ic], A, kbuf[kc]); passes(n_umi, shift_u); }
            if (n_lo - n_mapq) { launch_markdup_permute(c->stream, k_lo, ibuf[ic], A, kbuf[kc]); passes(n_lo - n_mapq, shift + n_mapq); }
            M.passes_mapq = n_mapq; M.passes_umi = n_umi;
            n_lo -= n_mapq;
        } else
        for (int p = 0; p < n_lo; ++p) {               // stage 1: by K_lo
            launch_sort_pass(c->stream, kbuf[kc], ibuf[ic], kbuf[kc ^ 1], ibuf[ic ^ 1], A, shift[p], (uint32_t *)X.hist.p, d_chunk, d_tot);
            kc ^= 1; ic ^= 1;
        }
        kc ^= 1;                                       // (the sorted K_lo keys are done with: K_hi in their order takes the other buffer)
        launch_markdup_permute(c->stream, k_hi, ibuf[ic], A, kbuf[kc]);
        const int n_hi = sort_live_digits(oa[1][0], oa[1][1], shift);
        for (int p = 0; p < n_hi; ++p) {               // stage 2: by K_hi, stable
            launch_sort_pass(c->stream, kbuf[kc], ibuf[ic], kbuf[kc ^ 1], ibuf[ic ^ 1], A, shift[p], (uint32_t *)X.hist.p, d_chunk, d_tot);
            kc ^= 1; ic ^= 1;
        }
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
        info.sort_ms = ms_since(t0);
        M.passes_lo = n_lo; M.passes_hi = n_hi;
        // ---- 4 heads: the marks take the payload's free buffer, D the keys' free buffer
        t0 = std::chrono::steady_clock::now();
        uint32_t *mark = ibuf[ic ^ 1], *list = (uint32_t *)kbuf[kc ^ 1];
        double heads_ms = 0;                           // (rsqc_markdup_umi_edits: the heads kernel, clocked apart from the grouping)
        if (M.use_umi) launch_markdup_heads_umi(c->stream, kbuf[kc], ibuf[ic], k_lo, k_umi, A, mark, d_cnt);
        else launch_markdup_heads(c->stream, kbuf[kc], ibuf[ic], k_lo, A, mark);
        if (M.umi_edits) {
            // ---- 4b rsqc_markdup_umi_edits(1): nodes, parents, roots, and marks that replace the plain ones.  The columns take buffers the
            // sort is done with: the node keys the keys' free buffer (D follows them there), the nodes' best anchors the sorted K_hi, the
            // groups' best anchors K_hi by slot, parents and roots the two halves of the UMI keys by slot (read last by the nodes kernel)
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            HIP_TRY(c, hipGetLastError());
            heads_ms = ms_since(t0);
            const bool profile = getenv("RSQC_MARKDUP_PROFILE") != nullptr;
            double part_ms[5] = {0, 0, 0, 0, 0};
            auto tg = std::chrono::steady_clock::now(), tk = tg;
            auto lap = [&](int k) {                        // the profile's split by kernel: a synchronisation behind each (an error stays for the one below)
                if (!profile) return;
                (void)hipStreamSynchronize(c->stream);
                part_ms[k] = ms_since(tk); tk = std::chrono::steady_clock::now();
            };
            uint32_t *mark_pos = (uint32_t *)X.g_mark.p, *node_head = (uint32_t *)X.g_head.p, *node_set = (uint32_t *)X.g_set.p, *set_first = (uint32_t *)X.g_first.p;
            uint64_t *node_key = kbuf[kc ^ 1], *node_best = kbuf[kc];
            unsigned long long *group_best = (unsigned long long *)X.k_hi.p;
            uint32_t *parent = (uint32_t *)X.k_umi.p, *root = parent + A;
            launch_markdup_heads_pos(c->stream, kbuf[kc], ibuf[ic], k_lo, A, mark_pos);
            launch_sort_scan(c->stream, mark, A, d_chunk, d_tot + 1);
            launch_sort_scan(c->stream, mark_pos, A, d_chunk, d_tot + 2);
            unsigned long long tot[2] = {0, 0};
            HIP_TRY(c, hipMemcpyAsync(tot, d_tot + 1, 16, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            HIP_TRY(c, hipGetLastError());
            if (tot[0] >= A || tot[1] >= A || tot[0] > tot[1]) return fail(c, RSQC_ERR_HIP, "rsqc_sort_end: the node marks of the UMI grouping do not add up");
            const uint32_t n_nodes = (uint32_t)(A - tot[0]), n_sets = (uint32_t)(A - tot[1]);
            lap(0);
            launch_markdup_group_nodes(c->stream, mark, mark_pos, d_tot + 1, ibuf[ic], k_lo, k_umi, A, node_key, node_head, node_best, node_set, set_first, group_best);
            lap(1);
            launch_markdup_group_parents(c->stream, node_key, node_head, node_set, set_first, n_nodes, n_sets, parent, d_cnt);
            lap(2);
            launch_markdup_group_roots(c->stream, parent, node_set, set_first, node_best, n_nodes, n_sets, root, group_best);
            lap(3);
            launch_markdup_group_marks(c->stream, mark, d_tot + 1, ibuf[ic], k_lo, root, group_best, A, n_nodes, mark_pos);
            lap(4);
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            HIP_TRY(c, hipGetLastError());
            M.group_info.group_ms = ms_since(tg);
            M.group_info.umi_nodes = n_nodes; M.group_info.exact_duplicate_fragments = tot[0];
            if (profile)
                fprintf(stderr, "markdup group: nodes %u, sets %u, heads_scans_ms %.3f, nodes_ms %.3f, parents_ms %.3f, roots_ms %.3f, marks_ms %.3f, device_bytes %llu\n", n_nodes, n_sets, part_ms[0],
                        part_ms[1], part_ms[2], part_ms[3], part_ms[4], (unsigned long long)(X.bytes() + M.verdict.bytes));
            t0 = std::chrono::steady_clock::now();
            mark = mark_pos;                           // the final marks; the scanned plain ones are done with
        }
        launch_sort_scan(c->stream, mark, A, d_chunk, d_tot);
        launch_markdup_list(c->stream, mark, d_tot, ibuf[ic], (const uint32_t *)X.ci.p, A, list);
        HIP_TRY(c, hipMemcpyAsync(&n_dup, d_tot, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
        info.mark_ms = heads_ms + ms_since(t0);
        if (n_dup >= A) return fail(c, RSQC_ERR_HIP, "rsqc_sort_end: the head marks of the duplicate marking do not add up");
        d_list = list;
    }
    info.duplicate_fragments = n_dup; info.sets = A - n_dup;
    // ---- 5 name set, 6 apply
    uint32_t mask = 0;
    if (n_dup) {
        if (n_dup > (1ull << 30)) return fail(c, RSQC_ERR_CAPACITY, "rsqc_sort_end: " + std::to_string(n_dup) + " duplicate fragments (the name table of the duplicate marking holds 2^30)");
        const uint64_t slots = markdup_table_size(n_dup);
        if ((rc = alloc_or_capacity(c, X.table, (size_t)slots * 4 + 64, "the name table", A))) return rc;
        mask = (uint32_t)(slots - 1);
    }
    t0 = std::chrono::steady_clock::now();
    if (n_dup) {
        HIP_TRY(c, hipMemsetAsync(X.table.p, 0xFF, ((size_t)mask + 1) * 4, c->stream));
        launch_markdup_insert(c->stream, C, d_list, n_dup, (uint32_t *)X.table.p, mask);
    }
    launch_markdup_apply(c->stream, C, d_list, n_dup, n_dup ? (const uint32_t *)X.table.p : nullptr, mask, (uint8_t *)M.verdict.p, d_cnt);
    unsigned long long cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(cnt, d_cnt, M.umi_edits ? 64 : 40, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    info.mark_ms += ms_since(t0);
    info.flagged_records = cnt[1]; info.cleared_records = cnt[2];
    if (M.use_umi) {
        if (cnt[3] > A || cnt[4] >= std::max<unsigned long long>(A, 1) || cnt[4] < n_dup) return fail(c, RSQC_ERR_HIP, "rsqc_sort_end: the UMI figures of the duplicate marking do not add up");
        M.umi_info.anchors_with_umi = cnt[3]; M.umi_info.anchors_without_umi = A - cnt[3]; M.umi_info.position_duplicate_fragments = cnt[4];
    }
    if (M.umi_edits && A) {
        rsqc_markdup_umi_group_info &G = M.group_info;
        G.merged_nodes = cnt[5];
        if (cnt[6] != G.umi_nodes || n_dup != G.exact_duplicate_fragments + G.merged_nodes || cnt[4] < n_dup || n_dup < G.exact_duplicate_fragments)
            return fail(c, RSQC_ERR_HIP, "rsqc_sort_end: the figures of the UMI grouping do not add up");
        if (getenv("RSQC_MARKDUP_PROFILE")) fprintf(stderr, "markdup group: merged_nodes %llu, probes %llu\n", cnt[5], cnt[7]);
    }
    // RSQC_MARKDUP_PROFILE: what the sort stages had to move (tools/markdup_bench.py) -- key + payload, read and written once per pass
    // and what the stage holds on the device at its end, the verdict column included (nothing is freed before)
    if (getenv("RSQC_MARKDUP_PROFILE"))
        fprintf(stderr, "markdup: anchors %llu, passes_lo %d, passes_hi %d, radix_bytes %llu, table_slots %llu, device_bytes %llu%s\n", A, M.passes_lo, M.passes_hi,
                (unsigned long long)(M.passes_lo + M.passes_hi + M.passes_mapq + M.passes_umi) * 2ull * 12ull * A, n_dup ? (unsigned long long)mask + 1ull : 0ull, (unsigned long long)(X.bytes() + M.verdict.bytes),
                M.use_umi ? (", passes_mapq " + std::to_string(M.passes_mapq) + ", passes_umi " + std::to_string(M.passes_umi) + ", umi_column_bytes " + std::to_string(S.umi.bytes)).c_str() : "");
    return 0;
}

}  // namespace

namespace rsqc {

void markdup_drop(rsqc_ctx *c) {
    MarkdupState &M = c->markdup;
    M.active = M.done = false;
    M.n = 0; M.passes_lo = M.passes_hi = M.passes_mapq = M.passes_umi = 0;
    M.use_umi = false; M.umi_edits = 0;
    M.info = rsqc_markdup_info{}; M.umi_info = rsqc_markdup_umi_info{}; M.group_info = rsqc_markdup_umi_group_info{};
    M.verdict.release();
    M.h_verdict.clear(); M.h_verdict.shrink_to_fit();
}

// called by rsqc_sort_end on the complete collection (the stream has been synchronised), before its key reduction
int markdup_run(rsqc_ctx *c) {
    MarkdupState &M = c->markdup;
    M.info = rsqc_markdup_info{}; M.umi_info = rsqc_markdup_umi_info{}; M.group_info = rsqc_markdup_umi_group_info{};
    M.info.records = M.n = c->sort.n;
    if (M.n == 0) { M.done = true; return 0; }
    Scratch X;
    const int rc = markdup_stage(c, X);
    if (rc) (void)hipStreamSynchronize(c->stream);
    X.release();                                       // everything but the verdict column goes before the coordinate sort allocates
    c->sort.umi.release(); c->sort.cap_umi = 0;        // ... the collection's UMI column with it: the gather into output batches never sees it
    if (rc) return rc;
    M.done = true;
    return 0;
}

}  // namespace rsqc

int rsqc_markdup_begin(rsqc_ctx *c) {
    if (!c) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (!c->sort.active) return fail(c, RSQC_ERR_ARG, "rsqc_sort_begin must precede rsqc_markdup_begin");
    if (c->markdup.active) return fail(c, RSQC_ERR_ARG, "rsqc_markdup_begin: the context is marking duplicates already");
    if (c->name_mode >= 0 || c->sort.batches_in || c->sort.n)
        return fail(c, RSQC_ERR_ARG, "rsqc_markdup_begin must precede the first submit of the pass");
    markdup_drop(c);
    c->markdup.active = true;
    return RSQC_OK;
}

int rsqc_markdup_use_umi(rsqc_ctx *c) {
    if (!c) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (!c->markdup.active || c->markdup.done) return fail(c, RSQC_ERR_ARG, "rsqc_markdup_begin must precede rsqc_markdup_use_umi");
    if (c->name_mode >= 0 || c->sort.batches_in || c->sort.n)
        return fail(c, RSQC_ERR_ARG, "rsqc_markdup_use_umi must precede the first submit of the pass");
    c->markdup.use_umi = true;
    return RSQC_OK;
}

int rsqc_markdup_umi_edits(rsqc_ctx *c, uint32_t max_edits) {
    if (!c) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (!c->markdup.active || c->markdup.done || !c->markdup.use_umi) return fail(c, RSQC_ERR_ARG, "rsqc_markdup_use_umi must precede rsqc_markdup_umi_edits");
    if (c->name_mode >= 0 || c->sort.batches_in || c->sort.n)
        return fail(c, RSQC_ERR_ARG, "rsqc_markdup_umi_edits must precede the first submit of the pass");
    if (max_edits > 1) return fail(c, RSQC_ERR_ARG, "rsqc_markdup_umi_edits: max_edits is 0 or 1, not " + std::to_string(max_edits));
    c->markdup.umi_edits = max_edits;
    return RSQC_OK;
}

int rsqc_markdup_umi_group_end(rsqc_ctx *c, rsqc_markdup_umi_group_info *out) {
    if (!c || !out) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (!c->markdup.active || !c->markdup.use_umi || !c->markdup.umi_edits) return fail(c, RSQC_ERR_ARG, "rsqc_markdup_umi_edits(1) must precede rsqc_markdup_umi_group_end");
    if (!c->markdup.done) return fail(c, RSQC_ERR_ARG, "rsqc_sort_end must precede rsqc_markdup_umi_group_end");
    *out = c->markdup.group_info;
    return RSQC_OK;
}

int rsqc_markdup_umi_end(rsqc_ctx *c, rsqc_markdup_umi_info *out) {
    if (!c || !out) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (!c->markdup.active || !c->markdup.use_umi) return fail(c, RSQC_ERR_ARG, "rsqc_markdup_use_umi must precede rsqc_markdup_umi_end");
    if (!c->markdup.done) return fail(c, RSQC_ERR_ARG, "rsqc_sort_end must precede rsqc_markdup_umi_end");
    *out = c->markdup.umi_info;
    return RSQC_OK;
}

int rsqc_markdup_end(rsqc_ctx *c, rsqc_markdup_info *out) {
    if (!c || !out) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (!c->markdup.active) return fail(c, RSQC_ERR_ARG, "rsqc_markdup_begin must precede rsqc_markdup_end");
    if (!c->markdup.done) return fail(c, RSQC_ERR_ARG, "rsqc_sort_end must precede rsqc_markdup_end");
    *out = c->markdup.info;
    return RSQC_OK;
}

int rsqc_markdup_verdicts(rsqc_ctx *c, uint64_t first, uint64_t n, const uint8_t **dup) {
    if (!c || !dup) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    MarkdupState &M = c->markdup;
    if (!M.active || !M.done) return fail(c, RSQC_ERR_ARG, "rsqc_markdup_begin and rsqc_sort_end must precede rsqc_markdup_verdicts");
    if (first > M.n || n > M.n - first) return fail(c, RSQC_ERR_ARG, "rsqc_markdup_verdicts: rows [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(n) + ") of " + std::to_string(M.n));
    M.h_verdict.resize((size_t)std::max<uint64_t>(n, 1));
    if (n) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipMemcpy(M.h_verdict.data(), (const uint8_t *)M.verdict.p + first, (size_t)n, hipMemcpyDeviceToHost));
    }
    *dup = M.h_verdict.data();
    return RSQC_OK;
}
