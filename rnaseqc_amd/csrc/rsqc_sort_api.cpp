// rsqc_sort_api.cpp -- rsqc_sort_begin / rsqc_sort_end: records in any order are collected on the device, ordered there (rsqc_sort.hip)
// and run as ordinary batches through run_batch, the path rsqc_submit_resident takes.
#include "rsqc_ctx.h"
#include "rsqc_sort.h"

namespace {

// `need` entries in every column of a group (cols / width), grown by doubling: new columns, a stream-ordered copy of what they hold,
// and the old ones freed as soon as that copy is through -- the stream is synchronised here, a dozen times for 100 M records, so
// that no outgrown generation stays beside the collection.  A column the device cannot give is RSQC_ERR_CAPACITY.
int grow_columns(rsqc_ctx *c, DevBuf *const *cols, const size_t *width, int n_col, uint64_t used, uint64_t need, uint64_t &cap, const char *what) {
    if (need <= cap) return 0;
    uint64_t ncap = std::max<uint64_t>(std::max<uint64_t>(need, 2 * cap), 1ull << 16);
    for (int attempt = 0; attempt < 2; ++attempt) {
        std::vector<DevBuf> fresh((size_t)n_col);
        bool ok = true;
        for (int k = 0; k < n_col && ok; ++k) {
            const size_t bytes = (size_t)ncap * width[k] + 64;
            if (hipMalloc(&fresh[(size_t)k].p, bytes) != hipSuccess) { (void)hipGetLastError(); fresh[(size_t)k].p = nullptr; ok = false; }
            else fresh[(size_t)k].bytes = bytes;
        }
        if (ok) {
            hipError_t e = hipSuccess;
            for (int k = 0; k < n_col && used && e == hipSuccess; ++k)
                e = hipMemcpyAsync(fresh[(size_t)k].p, cols[k]->p, (size_t)used * width[k], hipMemcpyDeviceToDevice, c->stream);
            if (e == hipSuccess && used) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) {
                for (auto &b : fresh) b.release();
                return fail(c, RSQC_ERR_HIP, std::string("rsqc_sort_begin: growing ") + what + ": " + hipGetErrorString(e));
            }
            for (int k = 0; k < n_col; ++k) { cols[k]->release(); *cols[k] = fresh[(size_t)k]; }
            if (used) free_parked(c);                  // (the stream has been synchronised)
            cap = ncap;
            return 0;
        }
        for (auto &b : fresh) b.release();
        if (ncap == need) break;
        ncap = need;                                   // (doubling did not fit: exactly what is needed, once)
        if (!c->parked.empty() && hipStreamSynchronize(c->stream) == hipSuccess) free_parked(c);
    }
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    return fail(c, RSQC_ERR_CAPACITY, std::string("the collection of rsqc_sort_begin does not fit the device: ") + what + " for " + std::to_string(need) + " entries (" +
                                          std::to_string(c->sort.n) + " records and " + std::to_string(c->sort.n_ops) + " CIGAR operations collected, " +
                                          std::to_string(free_b >> 20) + " MiB of " + std::to_string(total_b >> 20) + " MiB free)");
}

int alloc_or_capacity(rsqc_ctx *c, DevBuf &b, size_t bytes, const char *what) {
    if (dev_reserve(b, bytes)) return 0;
    return fail(c, RSQC_ERR_CAPACITY, std::string("rsqc_sort_end: no device memory for ") + what + " (" + std::to_string(bytes >> 20) + " MiB, " + std::to_string(c->sort.n) + " records collected)");
}

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// scratch of rsqc_sort_end: released when it returns
struct EndScratch {
    DevBuf idx0, idx1, key1, hist, chunk_sum, totals, part, batch_tab, moved;
    DevBuf o_core, o_aux, o_qh2, o_cigar, o_seg_tid, o_seg_start, o_wide_index, o_wide_nm, o_wide_lq, o_wide_nc, n_ops, seg_mark, wide_mark;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;             // around the gather kernels of every output batch
    void release(rsqc_ctx *c) {                                        // caller: the stream has been synchronised
        for (auto &pr : events) { c->event_pool.push_back(pr.first); c->event_pool.push_back(pr.second); }
        events.clear();
        for (DevBuf *b : {&idx0, &idx1, &key1, &hist, &chunk_sum, &totals, &part, &batch_tab, &moved, &o_core, &o_aux, &o_qh2, &o_cigar, &o_seg_tid, &o_seg_start,
                          &o_wide_index, &o_wide_nm, &o_wide_lq, &o_wide_nc, &n_ops, &seg_mark, &wide_mark}) b->release();
    }
};

int sort_end_run(rsqc_ctx *c, EndScratch &X, rsqc_sort_info &info) {
    SortState &S = c->sort;
    const uint64_t N = S.n;
    info.records = N; info.batches_in = S.batches_in;
    HIP_TRY(c, hipStreamSynchronize(c->stream));                       // (the collection is complete; parked columns can go)
    free_parked(c);
    int rc;
    if (c->markdup.active && (rc = markdup_run(c))) return rc;          // --mark-duplicates: flag 0x400 of the collection is rewritten first
    if (N == 0) { info.was_sorted = 1; return 0; }
    // ---- the payload, and what the keys say about the work: OR, AND, order
    // (key_ms and sort_ms are host clocks around kernels and the synchronisation behind them: every allocation is made before its clock starts)
    const uint32_t prep_grid = (uint32_t)std::min<uint64_t>(RSQC_SORT_PREP_GRID, (N + RSQC_SORT_THREADS - 1) / RSQC_SORT_THREADS);
    if ((rc = alloc_or_capacity(c, X.idx0, N * 4 + 64, "the sort's index column")) || (rc = alloc_or_capacity(c, X.part, (size_t)prep_grid * 24, "the key reduction"))) return rc;
    auto t0 = std::chrono::steady_clock::now();
    launch_sort_prepare(c->stream, (const uint64_t *)S.key.p, N, (uint32_t *)X.idx0.p, (unsigned long long *)X.part.p, prep_grid);
    std::vector<unsigned long long> part((size_t)prep_grid * 3);
    HIP_TRY(c, hipMemcpyAsync(part.data(), X.part.p, part.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    uint64_t key_or = 0, key_and = ~0ull; bool disorder = false;
    for (uint32_t k = 0; k < prep_grid; ++k) { key_or |= part[3 * k]; key_and &= part[3 * k + 1]; disorder = disorder || part[3 * k + 2] != 0; }
    info.key_ms = ms_since(t0);
    info.was_sorted = disorder ? 0 : 1;
    // ---- the radix passes over the digit positions in which the keys differ
    const uint64_t *key = (const uint64_t *)S.key.p;
    const uint32_t *idx = (const uint32_t *)X.idx0.p;
    const uint64_t tiles = (N + RSQC_SORT_TILE - 1) / RSQC_SORT_TILE;
    const uint64_t B_env = getenv("RSQC_SORT_BATCH") ? (uint64_t)atoll(getenv("RSQC_SORT_BATCH")) : (uint64_t)1 << 21;
    // (at most 16 384 batches in one pass, rsqc_submit.cpp: a larger collection gets larger batches)
    const uint64_t B = std::min<uint64_t>(std::max<uint64_t>(std::max<uint64_t>(B_env, 1), (N + 15999) / 16000), (1ull << 31) - 1);
    const uint64_t Bn = std::min(B, N);
    const uint64_t scan_chunks = std::max<uint64_t>((256 * tiles + RSQC_SCAN_CHUNK - 1) / RSQC_SCAN_CHUNK, (Bn + RSQC_SCAN_CHUNK - 1) / RSQC_SCAN_CHUNK) + 1;
    if ((rc = alloc_or_capacity(c, X.chunk_sum, scan_chunks * 8, "the scan's chunk sums")) || (rc = alloc_or_capacity(c, X.totals, 64, "the scan totals"))) return rc;
    if (disorder && ((rc = alloc_or_capacity(c, X.idx1, N * 4 + 64, "the sort's second index column")) || (rc = alloc_or_capacity(c, X.key1, N * 8 + 64, "the sort's second key column")) ||
                     (rc = alloc_or_capacity(c, X.hist, 256 * tiles * 4 + 64, "the digit histograms")))) return rc;
    t0 = std::chrono::steady_clock::now();
    if (disorder) {
        int shift[8];
        const int n_pass = sort_live_digits(key_or, key_and, shift);
        uint64_t *kbuf[2] = {(uint64_t *)S.key.p, (uint64_t *)X.key1.p};
        uint32_t *ibuf[2] = {(uint32_t *)X.idx0.p, (uint32_t *)X.idx1.p};
        int cur = 0;
        for (int p = 0; p < n_pass; ++p) {
            launch_sort_pass(c->stream, kbuf[cur], ibuf[cur], kbuf[cur ^ 1], ibuf[cur ^ 1], N, shift[p], (uint32_t *)X.hist.p, (unsigned long long *)X.chunk_sum.p, (unsigned long long *)X.totals.p);
            cur ^= 1;
        }
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
        key = kbuf[cur]; idx = ibuf[cur];
    }
    info.sort_ms = ms_since(t0);
    // ---- output batches: ranks [r0, r0 + n) gathered into one set of buffers, batch after batch in stream order
    std::vector<uint64_t> tab(S.batch_rec0);
    tab.push_back(N);
    const size_t nb = S.batch_rec0.size();
    tab.insert(tab.end(), S.batch_pool0.begin(), S.batch_pool0.end());
    if ((rc = alloc_or_capacity(c, X.batch_tab, tab.size() * 8 + 64, "the batch table"))) return rc;
    HIP_TRY(c, hipMemcpyAsync(X.batch_tab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, c->stream));
    SortCollection C{};
    C.core = (const rsqc_rec_core *)S.core.p; C.aux = (const rsqc_rec_aux *)S.aux.p; C.qhash2 = c->name_mode == 1 ? (const uint32_t *)S.qh2.p : nullptr; C.cigar = (const uint32_t *)S.cigar.p;
    C.batch_rec0 = (const uint64_t *)X.batch_tab.p; C.batch_pool0 = C.batch_rec0 + nb + 1; C.n_batches = (uint32_t)nb;
    C.wide_index = (const uint64_t *)S.wide_index.p; C.wide_nm = (const int32_t *)S.wide_nm.p; C.wide_l_qseq = (const int32_t *)S.wide_lq.p; C.wide_n_cigar = (const uint32_t *)S.wide_nc.p; C.n_wide = S.n_wide; C.n_ops = S.n_ops;
    const uint32_t moved_blocks = (uint32_t)((Bn + RSQC_SORT_THREADS - 1) / RSQC_SORT_THREADS);
    if ((rc = alloc_or_capacity(c, X.o_core, Bn * 16 + 64, "an output batch")) || (rc = alloc_or_capacity(c, X.o_aux, Bn * 16 + 64, "an output batch")) ||
        (rc = alloc_or_capacity(c, X.o_qh2, Bn * 4 + 64, "an output batch")) || (rc = alloc_or_capacity(c, X.o_seg_tid, Bn * 4 + 64, "an output batch")) ||
        (rc = alloc_or_capacity(c, X.o_seg_start, (Bn + 1) * 8 + 64, "an output batch")) || (rc = alloc_or_capacity(c, X.o_wide_index, Bn * 8 + 64, "an output batch")) ||
        (rc = alloc_or_capacity(c, X.o_wide_nm, Bn * 4 + 64, "an output batch")) || (rc = alloc_or_capacity(c, X.o_wide_lq, Bn * 4 + 64, "an output batch")) ||
        (rc = alloc_or_capacity(c, X.o_wide_nc, Bn * 4 + 64, "an output batch")) || (rc = alloc_or_capacity(c, X.n_ops, Bn * 4 + 64, "an output batch")) ||
        (rc = alloc_or_capacity(c, X.seg_mark, Bn * 4 + 64, "an output batch")) || (rc = alloc_or_capacity(c, X.wide_mark, Bn * 4 + 64, "an output batch")) ||
        (rc = alloc_or_capacity(c, X.moved, (size_t)moved_blocks * 4 + 64, "an output batch"))) return rc;
    std::vector<uint32_t> h_moved(moved_blocks);
    unsigned long long *d_tot = (unsigned long long *)X.totals.p;
    for (uint64_t r0 = 0; r0 < N; r0 += B) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(B, N - r0);
        const uint32_t blocks = (n + RSQC_SORT_THREADS - 1) / RSQC_SORT_THREADS;
        hipEvent_t e0 = get_event(c), e1 = get_event(c), e2 = get_event(c), e3 = get_event(c);
        X.events.emplace_back(e0, e1); X.events.emplace_back(e2, e3);  // (the scratch hands them back, however this call ends)
        HIP_TRY(c, hipEventRecord(e0, c->stream));
        launch_sort_gather_count(c->stream, C, key, idx, r0, n, (uint32_t *)X.n_ops.p, (uint32_t *)X.seg_mark.p, (uint32_t *)X.wide_mark.p, (uint32_t *)X.moved.p);
        launch_sort_scan(c->stream, (uint32_t *)X.n_ops.p, n, (unsigned long long *)X.chunk_sum.p, d_tot);
        launch_sort_scan(c->stream, (uint32_t *)X.seg_mark.p, n, (unsigned long long *)X.chunk_sum.p, d_tot + 1);
        launch_sort_scan(c->stream, (uint32_t *)X.wide_mark.p, n, (unsigned long long *)X.chunk_sum.p, d_tot + 2);
        HIP_TRY(c, hipEventRecord(e1, c->stream));
        unsigned long long tot[3] = {0, 0, 0};
        HIP_TRY(c, hipMemcpyAsync(tot, d_tot, 24, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(h_moved.data(), X.moved.p, (size_t)blocks * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));   // (also: the per-read kernels of the batch before this one are through)
        HIP_TRY(c, hipGetLastError());
        for (uint32_t k = 0; k < blocks; ++k) info.moved += h_moved[k];
        if (tot[0] >= (1ull << 30))
            return fail(c, RSQC_ERR_CAPACITY, "rsqc_sort_end: an output batch of " + std::to_string(n) + " records holds " + std::to_string(tot[0]) + " CIGAR operations (the limit of a batch is 2^30): lower RSQC_SORT_BATCH");
        if ((rc = alloc_or_capacity(c, X.o_cigar, (size_t)(tot[0] + tot[0] / 4) * 4 + 64, "an output batch's CIGAR pool"))) return rc;
        SortOutput O{};
        O.core = (rsqc_rec_core *)X.o_core.p; O.aux = (rsqc_rec_aux *)X.o_aux.p; O.qhash2 = (uint32_t *)X.o_qh2.p; O.cigar = (uint32_t *)X.o_cigar.p;
        O.seg_tid = (int32_t *)X.o_seg_tid.p; O.seg_start = (uint64_t *)X.o_seg_start.p;
        O.wide_index = (uint64_t *)X.o_wide_index.p; O.wide_nm = (int32_t *)X.o_wide_nm.p; O.wide_l_qseq = (int32_t *)X.o_wide_lq.p; O.wide_n_cigar = (uint32_t *)X.o_wide_nc.p;
        HIP_TRY(c, hipEventRecord(e2, c->stream));
        launch_sort_gather(c->stream, C, key, idx, r0, n, (const uint32_t *)X.n_ops.p, (const uint32_t *)X.seg_mark.p, (const uint32_t *)X.wide_mark.p, (uint32_t)tot[0], (uint32_t)tot[1], O);
        HIP_TRY(c, hipEventRecord(e3, c->stream));
        UploadedBatch *u = new UploadedBatch();        // (owns nothing: the columns are the scratch's)
        u->pooled = false;
        u->n = n; u->n_cigar_total = tot[0]; u->file_index_base = r0;          // a record's file index is its rank
        DevBatch &d = u->d;
        d.n = n; d.core = O.core; d.aux = O.aux; d.cigar = O.cigar; d.qhash2 = C.qhash2 ? O.qhash2 : nullptr;
        d.n_seg = (uint32_t)tot[1]; d.seg_tid = O.seg_tid; d.seg_start = O.seg_start; d.seg_file_index = nullptr;
        d.n_wide = (uint32_t)tot[2]; d.wide_index = O.wide_index; d.wide_nm = O.wide_nm; d.wide_l_qseq = O.wide_l_qseq; d.wide_n_cigar = O.wide_n_cigar;
        c->transient.push_back(u);
        if ((rc = run_batch(c, u))) return rc;
        info.batches_out += 1;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));       // the last batch has read the buffers this call is about to free
    HIP_TRY(c, hipGetLastError());
    for (auto &pr : X.events) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) info.gather_ms += ms;
    }
    return 0;
}

}  // namespace

namespace rsqc {

void sort_drop(rsqc_ctx *c) {
    SortState &S = c->sort;
    for (DevBuf *b : {&S.core, &S.aux, &S.qh2, &S.key, &S.cigar, &S.wide_index, &S.wide_nm, &S.wide_lq, &S.wide_nc, &S.umi}) b->release();
    S.active = false;
    S.n = S.n_ops = S.n_wide = S.cap_n = S.cap_ops = S.cap_wide = S.cap_umi = S.batches_in = 0;
    S.batch_rec0.clear(); S.batch_pool0.clear();
}

static int sort_append_run(rsqc_ctx *c, UploadedBatch *u) {
    SortState &S = c->sort;
    if (!u->seg_file_index.empty()) return fail(c, RSQC_ERR_ARG, "a batch with rsqc_batch.seg_file_index cannot be collected (rsqc_sort_begin): its file indices are ranks of the sorted order");
    const DevBatch &d = u->d;
    if (S.n + u->n > 0xFFFFFFF0ull) return fail(c, RSQC_ERR_CAPACITY, "more than 2^32 - 16 records between rsqc_sort_begin and rsqc_sort_end (" + std::to_string(S.n + u->n) + ")");
    int rc;
    {
        DevBuf *cols[4] = {&S.core, &S.aux, &S.qh2, &S.key}; const size_t width[4] = {16, 16, 4, 8};
        if ((rc = grow_columns(c, cols, width, 4, S.n, S.n + u->n, S.cap_n, "the record columns"))) return rc;
    }
    if (c->markdup.use_umi) {                          // the UMI keys: a column of its own, so that the record columns are what they are without the mode
        DevBuf *cols[1] = {&S.umi}; const size_t width[1] = {8};
        if ((rc = grow_columns(c, cols, width, 1, S.n, S.n + u->n, S.cap_umi, "the UMI column"))) return rc;
    }
    {
        DevBuf *cols[1] = {&S.cigar}; const size_t width[1] = {4};
        if ((rc = grow_columns(c, cols, width, 1, S.n_ops, S.n_ops + u->n_cigar_total + 1, S.cap_ops, "the CIGAR pool"))) return rc;
    }
    {
        DevBuf *cols[4] = {&S.wide_index, &S.wide_nm, &S.wide_lq, &S.wide_nc}; const size_t width[4] = {8, 4, 4, 4};
        if ((rc = grow_columns(c, cols, width, 4, S.n_wide, S.n_wide + d.n_wide + 1, S.cap_wide, "the wide table"))) return rc;
    }
    // stream-ordered copies out of the batch's device columns (a decode window's buffers, a transient upload, a resident batch):
    // made before anything later on the stream may overwrite them
    HIP_TRY(c, hipMemcpyAsync((char *)S.core.p + S.n * 16, d.core, (size_t)u->n * 16, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync((char *)S.aux.p + S.n * 16, d.aux, (size_t)u->n * 16, hipMemcpyDeviceToDevice, c->stream));
    if (d.qhash2) HIP_TRY(c, hipMemcpyAsync((char *)S.qh2.p + S.n * 4, d.qhash2, (size_t)u->n * 4, hipMemcpyDeviceToDevice, c->stream));
    if (c->markdup.use_umi) HIP_TRY(c, hipMemcpyAsync((char *)S.umi.p + S.n * 8, u->umi, (size_t)u->n * 8, hipMemcpyDeviceToDevice, c->stream));
    if (u->n_cigar_total) HIP_TRY(c, hipMemcpyAsync((char *)S.cigar.p + S.n_ops * 4, d.cigar, (size_t)u->n_cigar_total * 4, hipMemcpyDeviceToDevice, c->stream));
    launch_sort_append(c->stream, d.core, u->n, d.seg_tid, d.seg_start, d.n_seg, (uint64_t *)S.key.p + S.n, S.n, d.wide_index, d.wide_nm, d.wide_l_qseq, d.wide_n_cigar, d.n_wide,
                       (uint64_t *)S.wide_index.p + S.n_wide, (int32_t *)S.wide_nm.p + S.n_wide, (int32_t *)S.wide_lq.p + S.n_wide, (uint32_t *)S.wide_nc.p + S.n_wide);
    HIP_TRY(c, hipGetLastError());
    S.batch_rec0.push_back(S.n); S.batch_pool0.push_back(S.n_ops);
    S.n += u->n; S.n_ops += u->n_cigar_total; S.n_wide += d.n_wide; S.batches_in += 1;
    return 0;
}

int sort_append(rsqc_ctx *c, UploadedBatch *u) {
    const int rc = sort_append_run(c, u);
    // a batch that was refused for what it is (RSQC_ERR_ARG) leaves the collection as it was, like a refused batch of an ordinary
    // pass; one that was lost on the way in (capacity, a HIP error) voids the pass until rsqc_reset: never a partial result
    if (rc && rc != RSQC_ERR_ARG) c->sticky = rc;
    return rc;
}

}  // namespace rsqc

int rsqc_sort_begin(rsqc_ctx *c) {
    if (!c) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (!c->have_ann) return fail(c, RSQC_ERR_ARG, "rsqc_set_annotation must precede rsqc_sort_begin");
    if (c->finalized) return fail(c, RSQC_ERR_ARG, "rsqc_reset required after rsqc_finalize");
    if (c->sort.active) return fail(c, RSQC_ERR_ARG, "rsqc_sort_begin: the context is collecting already");
    if (c->name_mode >= 0 || !c->batch_file_index.empty() || c->next_record_base)
        return fail(c, RSQC_ERR_ARG, "rsqc_sort_begin must precede the first submit of the pass");
    HIP_TRY(c, hipSetDevice(c->device));
    sort_drop(c);
    markdup_drop(c);
    c->sort.active = true;
    return RSQC_OK;
}

int rsqc_sort_end(rsqc_ctx *c, rsqc_sort_info *out) {
    if (!c) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (!c->sort.active) return fail(c, RSQC_ERR_ARG, "rsqc_sort_begin must precede rsqc_sort_end");
    if (c->dec.active) return fail(c, RSQC_ERR_ARG, "rsqc_decode_end must precede rsqc_sort_end");
    HIP_TRY(c, hipSetDevice(c->device));
    c->sort.active = false;                            // (the output batches are RUN)
    rsqc_sort_info info{};
    EndScratch X;
    const int rc = sort_end_run(c, X, info);
    if (rc) (void)hipStreamSynchronize(c->stream);
    X.release(c);
    sort_drop(c);
    if (rc) { c->sticky = rc; return rc; }             // the collection is gone, some of it may have been counted: the pass is void until rsqc_reset
    c->dec.unsorted = false;                           // what the input's order would have triggered is settled
    if (out) *out = info;
    return RSQC_OK;
}
