// rsqc_tin_api.cpp -- rsqc_tin_begin / rsqc_tin_end / rsqc_tin_rows: the model of the pass is checked (genebody_check), planned and
// uploaded at its begin; behind rsqc_track_end TWO kernels (rsqc_tin.hip) walk the scanned difference array along every measured gene
// -- one partial per plan item, then one row per gene in item order -- and every row is copied to page-locked memory of the context.
#include "rsqc_ctx.h"
#include "rsqc_genebody.h"
#include "rsqc_tin.h"

namespace {

int alloc_or_capacity(rsqc_ctx *c, DevBuf &b, size_t bytes, const char *what, const std::string &sizes) {
    if (b.bytes >= bytes) return 0;
    b.release();
    if (hipMalloc(&b.p, bytes) != hipSuccess) {
        (void)hipGetLastError(); b.p = nullptr;
        return fail(c, RSQC_ERR_CAPACITY, std::string("rsqc_tin_begin: no device memory for ") + what + " (" + std::to_string(bytes) + " bytes; " + sizes + ")");
    }
    b.bytes = bytes;
    return 0;
}

int tin_end_run(rsqc_ctx *c) {
    TinState &N = c->tin;
    const TrackState &T = c->track;
    N.info.depth_sum = 0; N.info.covered_bases = 0; N.info.tin_ms = 0;
    if (!N.n_genes) return 0;
    hipEvent_t e0 = get_event(c), e1 = get_event(c);
    HIP_TRY(c, hipEventRecord(e0, c->stream));
    launch_tin_items(c->stream, (const uint32_t *)T.diff.p, (const uint64_t *)T.off.p,
                     TinModel{(const int32_t *)N.seg_tid.p, (const uint32_t *)N.seg_start.p, (const uint32_t *)N.seg_end.p},
                     (const TinItem *)N.items.p, N.n_items, (rsqc_tin_row *)N.part.p);
    launch_tin_rows(c->stream, (const rsqc_tin_row *)N.part.p, (const uint64_t *)N.item_off.p, (uint32_t)N.n_genes, (rsqc_tin_row *)N.rows.p);
    HIP_TRY(c, hipEventRecord(e1, c->stream));
    HIP_TRY(c, hipMemcpyAsync(N.h_rows, N.rows.p, (size_t)N.n_genes * sizeof(rsqc_tin_row), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) N.info.tin_ms = ms;
    c->event_pool.push_back(e0); c->event_pool.push_back(e1);
    for (int32_t g = 0; g < N.n_genes; ++g) { N.info.depth_sum += N.h_rows[g].depth_sum; N.info.covered_bases += N.h_rows[g].covered; }
    return 0;
}

}  // namespace

namespace rsqc {

void tin_drop(rsqc_ctx *c, bool free_buffers) {
    TinState &N = c->tin;
    N.active = N.done = false;
    N.n_genes = 0; N.n_items = 0;
    N.info = rsqc_tin_info{};
    if (free_buffers) {
        for (DevBuf *b : {&N.seg_tid, &N.seg_start, &N.seg_end, &N.items, &N.item_off, &N.part, &N.rows}) b->release();
        if (N.h_rows) (void)hipHostFree(N.h_rows);
        N.h_rows = nullptr; N.h_rows_cap = 0;
    }
}

}  // namespace rsqc

int rsqc_tin_begin(rsqc_ctx *c, int32_t n_genes, const uint32_t *seg_off, const int32_t *seg_tid, const uint32_t *seg_start, const uint32_t *seg_end) {
    if (!c) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (n_genes < 0 || (n_genes && !seg_off)) return fail(c, RSQC_ERR_ARG, "rsqc_tin_begin: n_genes genes with their segment offsets");
    if (!c->track.active || c->track.done) return fail(c, RSQC_ERR_ARG, "rsqc_track_begin of the same pass must precede rsqc_tin_begin");
    if (c->tin.active) return fail(c, RSQC_ERR_ARG, "rsqc_tin_begin: the context holds a tin model already");
    if (c->finalized || c->name_mode >= 0 || !c->batch_file_index.empty() || c->next_record_base)
        return fail(c, RSQC_ERR_ARG, "rsqc_tin_begin must precede the first submit of the pass");
    const size_t n_seg = n_genes ? seg_off[n_genes] : 0;
    if (n_seg && (!seg_tid || !seg_start || !seg_end)) return fail(c, RSQC_ERR_ARG, "rsqc_tin_begin: " + std::to_string(n_seg) + " segments without their columns");
    HIP_TRY(c, hipSetDevice(c->device));
    const TrackState &T = c->track;
    std::vector<uint32_t> length((size_t)T.n + 1, 0);
    if (T.n) {                                         // (the track keeps its contigs' lengths on the device only)
        HIP_TRY(c, hipMemcpyAsync(length.data(), T.length.p, (size_t)T.n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    const std::string broken = genebody_check(n_genes, seg_off, seg_tid, seg_start, seg_end, T.n, length.data());
    if (!broken.empty()) return fail(c, RSQC_ERR_ARG, "rsqc_tin_begin: " + broken);
    TinPlan P;
    tin_plan(n_genes, seg_off, seg_start, seg_end, RSQC_TIN_ITEM, P);
    tin_drop(c, false);
    TinState &N = c->tin;
    const std::string sizes = std::to_string(n_genes) + " genes, " + std::to_string(n_seg) + " segments, " + std::to_string(P.items.size()) + " items";
    const size_t row_bytes = (size_t)n_genes * sizeof(rsqc_tin_row);
    int rc;
    if ((rc = alloc_or_capacity(c, N.rows, row_bytes + 64, "the rows", sizes)) ||
        (rc = alloc_or_capacity(c, N.part, P.items.size() * sizeof(rsqc_tin_row) + 64, "the items' partials", sizes)) ||
        (rc = alloc_or_capacity(c, N.seg_tid, n_seg * 4 + 64, "the model", sizes)) ||
        (rc = alloc_or_capacity(c, N.seg_start, n_seg * 4 + 64, "the model", sizes)) ||
        (rc = alloc_or_capacity(c, N.seg_end, n_seg * 4 + 64, "the model", sizes)) ||
        (rc = alloc_or_capacity(c, N.items, P.items.size() * sizeof(TinItem) + 64, "the plan", sizes)) ||
        (rc = alloc_or_capacity(c, N.item_off, P.item_off.size() * 8 + 64, "the plan", sizes))) return rc;
    if (N.h_rows_cap < (size_t)n_genes) {
        if (N.h_rows) (void)hipHostFree(N.h_rows);
        N.h_rows = nullptr; N.h_rows_cap = 0;
        if (hipHostMalloc((void **)&N.h_rows, row_bytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError(); N.h_rows = nullptr;
            return fail(c, RSQC_ERR_CAPACITY, "rsqc_tin_begin: no page-locked memory for the rows (" + std::to_string(row_bytes) + " bytes; " + sizes + ")");
        }
        N.h_rows_cap = (size_t)n_genes;
    }
    // (pageable sources: the copies have left these arrays when the calls return; no memset: the kernels write every slot and row)
    if (n_seg) {
        HIP_TRY(c, hipMemcpyAsync(N.seg_tid.p, seg_tid, n_seg * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(N.seg_start.p, seg_start, n_seg * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(N.seg_end.p, seg_end, n_seg * 4, hipMemcpyHostToDevice, c->stream));
    }
    if (!P.items.empty()) HIP_TRY(c, hipMemcpyAsync(N.items.p, P.items.data(), P.items.size() * sizeof(TinItem), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(N.item_off.p, P.item_off.data(), P.item_off.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    N.n_genes = n_genes; N.n_items = P.items.size();
    N.info.n_genes = (uint64_t)n_genes; N.info.n_measured = P.n_measured; N.info.model_bases = P.model_bases;
    N.active = true;
    return RSQC_OK;
}

int rsqc_tin_end(rsqc_ctx *c, rsqc_tin_info *out) {
    if (!c || !out) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (!c->tin.active) return fail(c, RSQC_ERR_ARG, "rsqc_tin_begin must precede rsqc_tin_end");
    if (!c->track.active || !c->track.done) return fail(c, RSQC_ERR_ARG, "rsqc_track_end must precede rsqc_tin_end");
    if (!c->tin.done) {
        HIP_TRY(c, hipSetDevice(c->device));
        const int rc = tin_end_run(c);
        if (rc) { (void)hipStreamSynchronize(c->stream); c->sticky = rc; return rc; }      // never partial rows: the pass is void until rsqc_reset
        c->tin.done = true;
    }
    *out = c->tin.info;
    return RSQC_OK;
}

int rsqc_tin_rows(rsqc_ctx *c, uint32_t first_gene, uint32_t n, const rsqc_tin_row **rows) {
    if (!c || !rows) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    const TinState &N = c->tin;
    if (!N.active || !N.done) return fail(c, RSQC_ERR_ARG, "rsqc_tin_end must precede rsqc_tin_rows");
    if (first_gene > (uint32_t)N.n_genes || n > (uint32_t)N.n_genes - first_gene)
        return fail(c, RSQC_ERR_ARG, "rsqc_tin_rows: genes [" + std::to_string(first_gene) + ", + " + std::to_string(n) + ") of " + std::to_string(N.n_genes));
    *rows = N.h_rows ? N.h_rows + first_gene : nullptr;        // (no gene ever: NULL)
    return RSQC_OK;
}
