// rsqc_genebody_api.cpp -- rsqc_genebody_begin / rsqc_genebody_end / rsqc_genebody_sums: the model of the pass is checked, planned and
// uploaded at its begin; behind rsqc_track_end ONE kernel (rsqc_genebody.hip) walks the scanned difference array along every measured
// gene and leaves 100 sums per gene on the device; windows of them are copied to the host on request.
#include "rsqc_ctx.h"
#include "rsqc_genebody.h"

namespace {

int alloc_or_capacity(rsqc_ctx *c, DevBuf &b, size_t bytes, const char *what, const std::string &sizes) {
    if (b.bytes >= bytes) return 0;
    b.release();
    if (hipMalloc(&b.p, bytes) != hipSuccess) {
        (void)hipGetLastError(); b.p = nullptr;
        return fail(c, RSQC_ERR_CAPACITY, std::string("rsqc_genebody_begin: no device memory for ") + what + " (" + std::to_string(bytes) + " bytes; " + sizes + ")");
    }
    b.bytes = bytes;
    return 0;
}

int genebody_end_run(rsqc_ctx *c) {
    GenebodyState &G = c->genebody;
    const TrackState &T = c->track;
    G.info.depth_sum = 0; G.info.bins_ms = 0;
    if (!G.n_items) return 0;                          // (no measured gene: the sums are the zeroes of rsqc_genebody_begin)
    hipEvent_t e0 = get_event(c), e1 = get_event(c);
    HIP_TRY(c, hipEventRecord(e0, c->stream));
    launch_genebody_bins(c->stream, (const uint32_t *)T.diff.p, (const uint64_t *)T.off.p,
                         GenebodyModel{(const int32_t *)G.seg_tid.p, (const uint32_t *)G.seg_start.p, (const uint32_t *)G.seg_end.p},
                         (const GenebodyItem *)G.items.p, G.n_items, (unsigned long long *)G.sums.p, (unsigned long long *)G.total.p);
    HIP_TRY(c, hipEventRecord(e1, c->stream));
    unsigned long long total = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, G.total.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) G.info.bins_ms = ms;
    c->event_pool.push_back(e0); c->event_pool.push_back(e1);
    G.info.depth_sum = total;
    return 0;
}

}  // namespace

namespace rsqc {

void genebody_drop(rsqc_ctx *c, bool free_buffers) {
    GenebodyState &G = c->genebody;
    G.active = G.done = false;
    G.n_genes = 0; G.n_items = 0;
    G.info = rsqc_genebody_info{};
    if (free_buffers) {
        for (DevBuf *b : {&G.seg_tid, &G.seg_start, &G.seg_end, &G.items, &G.sums, &G.total}) b->release();
        if (G.h_sums) (void)hipHostFree(G.h_sums);
        G.h_sums = nullptr; G.h_sums_cap = 0;
    }
}

}  // namespace rsqc

int rsqc_genebody_begin(rsqc_ctx *c, int32_t n_genes, const uint32_t *seg_off, const int32_t *seg_tid, const uint32_t *seg_start, const uint32_t *seg_end, const uint8_t *reverse) {
    if (!c) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (n_genes < 0 || (n_genes && (!seg_off || !reverse))) return fail(c, RSQC_ERR_ARG, "rsqc_genebody_begin: n_genes genes with their segment offsets and reverse bytes");
    if (!c->track.active || c->track.done) return fail(c, RSQC_ERR_ARG, "rsqc_track_begin of the same pass must precede rsqc_genebody_begin");
    if (c->genebody.active) return fail(c, RSQC_ERR_ARG, "rsqc_genebody_begin: the context holds a gene-body model already");
    if (c->finalized || c->name_mode >= 0 || !c->batch_file_index.empty() || c->next_record_base)
        return fail(c, RSQC_ERR_ARG, "rsqc_genebody_begin must precede the first submit of the pass");
    const size_t n_seg = n_genes ? seg_off[n_genes] : 0;
    if (n_seg && (!seg_tid || !seg_start || !seg_end)) return fail(c, RSQC_ERR_ARG, "rsqc_genebody_begin: " + std::to_string(n_seg) + " segments without their columns");
    HIP_TRY(c, hipSetDevice(c->device));
    const TrackState &T = c->track;
    std::vector<uint32_t> length((size_t)T.n + 1, 0);
    if (T.n) {                                         // (the track keeps its contigs' lengths on the device only)
        HIP_TRY(c, hipMemcpyAsync(length.data(), T.length.p, (size_t)T.n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    const std::string broken = genebody_check(n_genes, seg_off, seg_tid, seg_start, seg_end, T.n, length.data());
    if (!broken.empty()) return fail(c, RSQC_ERR_ARG, "rsqc_genebody_begin: " + broken);
    GenebodyPlan P;
    genebody_plan(n_genes, seg_off, seg_start, seg_end, reverse, RSQC_GENEBODY_ITEM, P);
    genebody_drop(c, false);
    GenebodyState &G = c->genebody;
    const std::string sizes = std::to_string(n_genes) + " genes, " + std::to_string(n_seg) + " segments, " + std::to_string(P.items.size()) + " items";
    const size_t sum_bytes = (size_t)n_genes * RSQC_GENEBODY_BINS * 8;
    int rc;
    if ((rc = alloc_or_capacity(c, G.sums, sum_bytes + 64, "the sums", sizes)) ||
        (rc = alloc_or_capacity(c, G.seg_tid, n_seg * 4 + 64, "the model", sizes)) ||
        (rc = alloc_or_capacity(c, G.seg_start, n_seg * 4 + 64, "the model", sizes)) ||
        (rc = alloc_or_capacity(c, G.seg_end, n_seg * 4 + 64, "the model", sizes)) ||
        (rc = alloc_or_capacity(c, G.items, P.items.size() * sizeof(GenebodyItem) + 64, "the plan", sizes)) ||
        (rc = alloc_or_capacity(c, G.total, 64, "the total", sizes))) return rc;
    // (pageable sources: the copies have left these arrays when the calls return)
    HIP_TRY(c, hipMemsetAsync(G.sums.p, 0, sum_bytes + 64, c->stream));
    HIP_TRY(c, hipMemsetAsync(G.total.p, 0, 64, c->stream));
    if (n_seg) {
        HIP_TRY(c, hipMemcpyAsync(G.seg_tid.p, seg_tid, n_seg * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(G.seg_start.p, seg_start, n_seg * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(G.seg_end.p, seg_end, n_seg * 4, hipMemcpyHostToDevice, c->stream));
    }
    if (!P.items.empty()) HIP_TRY(c, hipMemcpyAsync(G.items.p, P.items.data(), P.items.size() * sizeof(GenebodyItem), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    G.n_genes = n_genes; G.n_items = P.items.size();
    G.info.n_genes = (uint64_t)n_genes; G.info.n_measured = P.n_measured; G.info.model_bases = P.model_bases;
    G.active = true;
    return RSQC_OK;
}

int rsqc_genebody_end(rsqc_ctx *c, rsqc_genebody_info *out) {
    if (!c || !out) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (!c->genebody.active) return fail(c, RSQC_ERR_ARG, "rsqc_genebody_begin must precede rsqc_genebody_end");
    if (!c->track.active || !c->track.done) return fail(c, RSQC_ERR_ARG, "rsqc_track_end must precede rsqc_genebody_end");
    if (!c->genebody.done) {
        HIP_TRY(c, hipSetDevice(c->device));
        const int rc = genebody_end_run(c);
        if (rc) { (void)hipStreamSynchronize(c->stream); c->sticky = rc; return rc; }      // never partial sums: the pass is void until rsqc_reset
        c->genebody.done = true;
    }
    *out = c->genebody.info;
    return RSQC_OK;
}

int rsqc_genebody_sums(rsqc_ctx *c, uint32_t first_gene, uint32_t n, const uint64_t **sums) {
    if (!c || !sums) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    GenebodyState &G = c->genebody;
    if (!G.active || !G.done) return fail(c, RSQC_ERR_ARG, "rsqc_genebody_end must precede rsqc_genebody_sums");
    if (first_gene > (uint32_t)G.n_genes || n > (uint32_t)G.n_genes - first_gene)
        return fail(c, RSQC_ERR_ARG, "rsqc_genebody_sums: genes [" + std::to_string(first_gene) + ", + " + std::to_string(n) + ") of " + std::to_string(G.n_genes));
    const size_t values = (size_t)n * RSQC_GENEBODY_BINS;
    if (values) {
        HIP_TRY(c, hipSetDevice(c->device));
        if (G.h_sums_cap < values) {
            if (G.h_sums) (void)hipHostFree(G.h_sums);
            G.h_sums = nullptr; G.h_sums_cap = 0;
            if (hipHostMalloc((void **)&G.h_sums, values * 8, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError(); G.h_sums = nullptr;
                return fail(c, RSQC_ERR_CAPACITY, "rsqc_genebody_sums: no page-locked memory for a window of " + std::to_string(values * 8) + " bytes");
            }
            G.h_sums_cap = values;
        }
        HIP_TRY(c, hipMemcpyAsync(G.h_sums, (const uint64_t *)G.sums.p + (size_t)first_gene * RSQC_GENEBODY_BINS, values * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    *sums = G.h_sums;                                  // (no gene: may be NULL)
    return RSQC_OK;
}
