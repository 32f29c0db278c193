// rsqc_junction_api.cpp -- rsqc_junctions_begin / rsqc_junctions_end: every batch that run_batch runs leaves its splice-junction
// instances in a device-resident collection (one extra kernel per batch, rsqc_junction.hip); at the end of the pass they are ordered
// with the radix passes of --sort (rsqc_sort.hip) and reduced to one row per junction.
#include "rsqc_ctx.h"
#include "rsqc_junction.h"
#include "rsqc_sort.h"

namespace {

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

int alloc_or_capacity(rsqc_ctx *c, DevBuf &b, size_t bytes, const char *what) {
    if (dev_reserve(b, bytes)) return 0;
    return fail(c, RSQC_ERR_CAPACITY, std::string("rsqc_junctions_end: no device memory for ") + what + " (" + std::to_string(bytes >> 20) + " MiB)");
}

// the collection's three columns with room for `need` instances, grown by doubling like the columns of --sort: new columns, a
// stream-ordered copy of the `filled` entries that may hold instances, the old ones freed once that copy is through (the stream is
// synchronised here: a handful of times per pass).  The true count stays in the device cursor.
int grow_collection(rsqc_ctx *c, uint64_t filled, uint64_t need) {
    JunctionState &J = c->junc;
    if (need <= J.cap && J.key_hi.p) return 0;
    need = std::min<uint64_t>(std::max<uint64_t>(need, 1), RSQC_JUNC_MAX);
    const uint64_t ncap = std::min<uint64_t>(std::max<uint64_t>(need, 2 * J.cap), RSQC_JUNC_MAX);
    DevBuf *cols[3] = {&J.key_hi, &J.end, &J.info}; const size_t width[3] = {8, 4, 4};
    if (J.key_hi.p && J.key_hi.bytes >= (size_t)ncap * 8 + 64 && J.end.bytes >= (size_t)ncap * 4 + 64 && J.info.bytes >= (size_t)ncap * 4 + 64) { J.cap = ncap; return 0; }   // (buffers kept from an earlier pass)
    DevBuf fresh[3];
    for (int k = 0; k < 3; ++k) {
        const size_t bytes = (size_t)ncap * width[k] + 64;
        if (hipMalloc(&fresh[k].p, bytes) != hipSuccess) {
            (void)hipGetLastError(); fresh[k].p = nullptr;
            for (auto &b : fresh) b.release();
            return fail(c, RSQC_ERR_CAPACITY, "the junction collection does not fit the device: " + std::to_string(ncap) + " instances of 16 bytes");
        }
        fresh[k].bytes = bytes;
    }
    filled = std::min(filled, J.cap);
    hipError_t e = hipSuccess;
    for (int k = 0; k < 3 && filled && cols[k]->p && e == hipSuccess; ++k)
        e = hipMemcpyAsync(fresh[k].p, cols[k]->p, (size_t)filled * width[k], hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess && J.key_hi.p) e = hipStreamSynchronize(c->stream);       // (earlier batches' extractions write the old columns)
    if (e != hipSuccess) {
        for (auto &b : fresh) b.release();
        return fail(c, RSQC_ERR_HIP, std::string("growing the junction collection: ") + hipGetErrorString(e));
    }
    for (int k = 0; k < 3; ++k) { cols[k]->release(); *cols[k] = fresh[k]; }
    J.cap = ncap;
    return 0;
}

// scratch of the order and the reduction: released when rsqc_junctions_end returns
struct EndScratch {
    DevBuf key0, key1, idx0, idx1, hist, chunk_sum, totals, part, mark, rows;
    void release() { for (DevBuf *b : {&key0, &key1, &idx0, &idx1, &hist, &chunk_sum, &totals, &part, &mark, &rows}) b->release(); }
};

int junctions_end_run(rsqc_ctx *c, EndScratch &X) {
    JunctionState &J = c->junc;
    rsqc_junction_table &T = J.table;
    T = rsqc_junction_table{};
    unsigned long long cur[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(cur, J.cursor.p, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    for (auto &pr : J.events) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) T.extract_ms += ms;
        c->event_pool.push_back(pr.first); c->event_pool.push_back(pr.second);
    }
    J.events.clear();
    const uint64_t N = cur[0];
    if (N > J.cap || N >= RSQC_JUNC_MAX)
        return fail(c, RSQC_ERR_CAPACITY, "rsqc_junctions_end: " + std::to_string(N) + " junction instances, the collection holds " + std::to_string(J.cap) + " (the limit of a pass is 2^32 - 16)");
    T.instances = N; T.population = cur[1];
    J.tid.clear(); J.start.clear(); J.end_h.clear(); J.reads.clear(); J.hq_reads.clear(); J.max_overhang.clear();
    if (N == 0) return 0;
    int rc;
    // ---- order: LSD over the 96-bit key in two stages of 64-bit radix passes, dead digit positions skipped in both
    const uint64_t tiles = (N + RSQC_SORT_TILE - 1) / RSQC_SORT_TILE;
    const uint32_t prep_grid = (uint32_t)std::min<uint64_t>(RSQC_SORT_PREP_GRID, (N + RSQC_SORT_THREADS - 1) / RSQC_SORT_THREADS);
    const uint64_t scan_chunks = std::max<uint64_t>((256 * tiles + RSQC_SCAN_CHUNK - 1) / RSQC_SCAN_CHUNK, (N + RSQC_SCAN_CHUNK - 1) / RSQC_SCAN_CHUNK) + 1;
    if ((rc = alloc_or_capacity(c, X.key0, N * 8 + 64, "the sort's key column")) || (rc = alloc_or_capacity(c, X.key1, N * 8 + 64, "the sort's second key column")) ||
        (rc = alloc_or_capacity(c, X.idx0, N * 4 + 64, "the sort's index column")) || (rc = alloc_or_capacity(c, X.idx1, N * 4 + 64, "the sort's second index column")) ||
        (rc = alloc_or_capacity(c, X.hist, 256 * tiles * 4 + 64, "the digit histograms")) || (rc = alloc_or_capacity(c, X.chunk_sum, scan_chunks * 8, "the scan's chunk sums")) ||
        (rc = alloc_or_capacity(c, X.totals, 64, "the scan totals")) || (rc = alloc_or_capacity(c, X.part, (size_t)prep_grid * 48, "the key reduction")) ||
        (rc = alloc_or_capacity(c, X.mark, N * 4 + 64, "the head marks"))) return rc;
    const uint64_t *key_hi = (const uint64_t *)J.key_hi.p; const uint32_t *end = (const uint32_t *)J.end.p, *info = (const uint32_t *)J.info.p;
    uint64_t *kbuf[2] = {(uint64_t *)X.key0.p, (uint64_t *)X.key1.p};
    uint32_t *ibuf[2] = {(uint32_t *)X.idx0.p, (uint32_t *)X.idx1.p};
    unsigned long long *d_part = (unsigned long long *)X.part.p, *d_tot = (unsigned long long *)X.totals.p;
    auto t0 = std::chrono::steady_clock::now();
    // OR and AND of both key parts in one read-back (they do not depend on the order): the prepare kernel's index column of the
    // second call is scratch, its "already in order" answer is not used -- it says nothing about the two-stage key
    launch_junction_widen(c->stream, end, N, kbuf[0]);
    launch_sort_prepare(c->stream, key_hi, N, ibuf[1], d_part + (size_t)prep_grid * 3, prep_grid);
    launch_sort_prepare(c->stream, kbuf[0], N, ibuf[0], d_part, prep_grid);
    std::vector<unsigned long long> part((size_t)prep_grid * 6);
    HIP_TRY(c, hipMemcpyAsync(part.data(), X.part.p, part.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    uint64_t oa[2][2] = {{0, ~0ull}, {0, ~0ull}};
    for (int h = 0; h < 2; ++h)
        for (uint32_t k = 0; k < prep_grid; ++k) { oa[h][0] |= part[(size_t)h * prep_grid * 3 + 3 * k]; oa[h][1] &= part[(size_t)h * prep_grid * 3 + 3 * k + 1]; }
    int shift[8], kc = 0, ic = 0;                      // kbuf[kc] / ibuf[ic]: the current keys and payload
    const int n_end = sort_live_digits(oa[0][0], oa[0][1], shift);
    for (int p = 0; p < n_end; ++p) {                  // stage 1: by `end`
        launch_sort_pass(c->stream, kbuf[kc], ibuf[ic], kbuf[kc ^ 1], ibuf[ic ^ 1], N, shift[p], (uint32_t *)X.hist.p, (unsigned long long *)X.chunk_sum.p, d_tot);
        kc ^= 1; ic ^= 1;
    }
    kc ^= 1;                                           // (the sorted `end` keys are done with: key_hi in their order takes the other buffer)
    launch_junction_permute(c->stream, key_hi, ibuf[ic], N, kbuf[kc]);
    const int n_hi = sort_live_digits(oa[1][0], oa[1][1], shift);
    for (int p = 0; p < n_hi; ++p) {                   // stage 2: by (tid, start), stable
        launch_sort_pass(c->stream, kbuf[kc], ibuf[ic], kbuf[kc ^ 1], ibuf[ic ^ 1], N, shift[p], (uint32_t *)X.hist.p, (unsigned long long *)X.chunk_sum.p, d_tot);
        kc ^= 1; ic ^= 1;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    T.sort_ms = ms_since(t0);
    // ---- reduce: head marks, their prefix sum (the row of every instance, the number of rows), the rows
    t0 = std::chrono::steady_clock::now();
    launch_junction_heads(c->stream, kbuf[kc], ibuf[ic], end, N, (uint32_t *)X.mark.p);
    launch_sort_scan(c->stream, (uint32_t *)X.mark.p, N, (unsigned long long *)X.chunk_sum.p, d_tot);
    unsigned long long rows = 0;
    HIP_TRY(c, hipMemcpyAsync(&rows, d_tot, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (rows == 0 || rows > N) return fail(c, RSQC_ERR_HIP, "rsqc_junctions_end: the head marks do not add up");
    if ((rc = alloc_or_capacity(c, X.rows, (size_t)rows * 24 + 64, "the junction table"))) return rc;
    HIP_TRY(c, hipMemsetAsync(X.rows.p, 0, (size_t)rows * 24, c->stream));
    JunctionRows R{};
    R.tid = (int32_t *)X.rows.p; R.start = R.tid + rows; R.end = R.start + rows;
    R.reads = (uint32_t *)(R.end + rows); R.hq_reads = R.reads + rows; R.max_overhang = R.hq_reads + rows;
    launch_junction_reduce(c->stream, kbuf[kc], ibuf[ic], end, info, N, (const uint32_t *)X.mark.p, d_tot, R);
    J.tid.resize(rows); J.start.resize(rows); J.end_h.resize(rows); J.reads.resize(rows); J.hq_reads.resize(rows); J.max_overhang.resize(rows);
    void *dst[6] = {J.tid.data(), J.start.data(), J.end_h.data(), J.reads.data(), J.hq_reads.data(), J.max_overhang.data()};
    for (int k = 0; k < 6; ++k) HIP_TRY(c, hipMemcpyAsync(dst[k], (char *)X.rows.p + (size_t)k * rows * 4, (size_t)rows * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    T.reduce_ms = ms_since(t0);
    T.n = rows;
    T.tid = J.tid.data(); T.start = J.start.data(); T.end = J.end_h.data();
    T.reads = J.reads.data(); T.hq_reads = J.hq_reads.data(); T.max_overhang = J.max_overhang.data();
    return 0;
}

}  // namespace

namespace rsqc {

void junction_drop(rsqc_ctx *c, bool free_buffers) {
    JunctionState &J = c->junc;
    for (auto &pr : J.events) { c->event_pool.push_back(pr.first); c->event_pool.push_back(pr.second); }
    J.events.clear();
    J.active = J.done = false;
    J.bound = 0;
    J.table = rsqc_junction_table{};
    J.tid.clear(); J.start.clear(); J.end_h.clear(); J.reads.clear(); J.hq_reads.clear(); J.max_overhang.clear();
    if (free_buffers) { for (DevBuf *b : {&J.key_hi, &J.end, &J.info, &J.cursor}) b->release(); J.cap = 0; }
}

// called by run_batch for every batch it runs, on the main stream in front of the event that retires the batch
int junction_extract(rsqc_ctx *c, const UploadedBatch *u, const DevBatch &d) {
    JunctionState &J = c->junc;
    // the host's bound on the instances so far needs nothing from the device: half the operations of every batch
    const uint64_t filled = J.bound;
    J.bound += u->n_cigar_total / 2;
    int rc = grow_collection(c, filled, std::max<uint64_t>(J.bound, J.cap0));
    if (rc) { c->sticky = rc; return rc; }
    JunctionBatch B{};
    B.core = d.core; B.aux = d.aux; B.cigar = d.cigar; B.n = d.n; B.n_ops = u->n_cigar_total;
    B.seg_tid = d.seg_tid; B.seg_start = d.seg_start; B.n_seg = d.n_seg;
    B.wide_index = d.wide_index; B.wide_n_cigar = d.wide_n_cigar; B.n_wide = d.n_wide;
    JunctionCollection C{(uint64_t *)J.key_hi.p, (uint32_t *)J.end.p, (uint32_t *)J.info.p, J.cap, (unsigned long long *)J.cursor.p};
    hipEvent_t e0 = get_event(c), e1 = get_event(c);
    J.events.emplace_back(e0, e1);
    HIP_TRY(c, hipEventRecord(e0, c->stream));
    launch_junction_extract(c->stream, B, c->n_contigs, c->dparams.mapq_threshold, C, c->acc.error);
    HIP_TRY(c, hipEventRecord(e1, c->stream));
    return 0;
}

}  // namespace rsqc

int rsqc_junctions_begin(rsqc_ctx *c) {
    if (!c) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (!c->have_ann) return fail(c, RSQC_ERR_ARG, "rsqc_set_annotation must precede rsqc_junctions_begin");
    if (c->finalized) return fail(c, RSQC_ERR_ARG, "rsqc_reset required after rsqc_finalize");
    if (c->junc.active) return fail(c, RSQC_ERR_ARG, "rsqc_junctions_begin: the context is counting junctions already");
    if (c->name_mode >= 0 || !c->batch_file_index.empty() || c->next_record_base)
        return fail(c, RSQC_ERR_ARG, "rsqc_junctions_begin must precede the first submit of the pass");
    HIP_TRY(c, hipSetDevice(c->device));
    junction_drop(c, false);
    JunctionState &J = c->junc;
    J.cap0 = RSQC_JUNC_CAP0;
    if (const char *e = getenv("RSQC_JUNCTION_CAP0")) J.cap0 = std::min<uint64_t>(std::max<long long>(atoll(e), 1), RSQC_JUNC_MAX);
    J.cap = 0;                                         // (kept buffers are taken up again by the first batch, at the size the pass asks for)
    if (!J.cursor.p) { HIP_TRY(c, hipMalloc(&J.cursor.p, 64)); J.cursor.bytes = 64; }
    HIP_TRY(c, hipMemsetAsync(J.cursor.p, 0, 64, c->stream));
    J.active = true;
    return RSQC_OK;
}

int rsqc_junctions_end(rsqc_ctx *c, rsqc_junction_table *out) {
    if (!c || !out) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (!c->junc.active) return fail(c, RSQC_ERR_ARG, "rsqc_junctions_begin must precede rsqc_junctions_end");
    if (!c->finalized) return fail(c, RSQC_ERR_ARG, "rsqc_finalize (or rsqc_finalize_device) must precede rsqc_junctions_end");
    if (!c->junc.done) {
        HIP_TRY(c, hipSetDevice(c->device));
        EndScratch X;
        const int rc = junctions_end_run(c, X);
        if (rc) (void)hipStreamSynchronize(c->stream);
        X.release();
        if (rc) { c->sticky = rc; return rc; }         // never a partial table: the pass is void until rsqc_reset
        c->junc.done = true;
    }
    *out = c->junc.table;
    return RSQC_OK;
}
