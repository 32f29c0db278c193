// rsqc_genebody_api.cpp -- rsqc_genebody_begin / rsqc_genebody_end / rsqc_genebody_sums: the model of the pass is checked, planned and
// uploaded at its begin (the part it shares with --tin: rsqc_genemodel_api.cpp); behind rsqc_track_end ONE kernel (rsqc_genebody.hip)
// walks the scanned difference array along every measured gene and leaves 100 sums per gene on the device; windows of them are
// copied to the host on request.
#include "rsqc_ctx.h"
#include "rsqc_genebody.h"

namespace {

int genebody_end_run(rsqc_ctx *c) {
    GenebodyState &G = c->genebody;
    const TrackState &T = c->track;
    G.info.depth_sum = 0; G.info.bins_ms = 0;
    if (!G.n_items) return 0;                          // (no measured gene: the sums are the zeroes of rsqc_genebody_begin)
    unsigned long long total = 0;
    const int rc = run_timed(c, &G.info.bins_ms, [&] {
        launch_genebody_bins(c->stream, (const uint32_t *)T.diff.p, (const uint64_t *)T.off.p,
                             GeneModel{(const int32_t *)G.seg_tid.p, (const uint32_t *)G.seg_start.p, (const uint32_t *)G.seg_end.p},
                             (const GenebodyItem *)G.items.p, G.n_items, (unsigned long long *)G.sums.p, (unsigned long long *)G.total.p);
    }, [&]() -> int { HIP_TRY(c, hipMemcpyAsync(&total, G.total.p, 8, hipMemcpyDeviceToHost, c->stream)); return 0; });
    if (rc) return rc;
    G.info.depth_sum = total;
    return 0;
}

}  // namespace

namespace rsqc {

void genebody_drop(rsqc_ctx *c, bool free_buffers) {
    GenebodyState &G = c->genebody;
    gene_drop(G, free_buffers);
    G.info = rsqc_genebody_info{};
    if (free_buffers) { G.sums.release(); G.total.release(); G.h_sums.release(); }
}

}  // namespace rsqc

int rsqc_genebody_begin(rsqc_ctx *c, int32_t n_genes, const uint32_t *seg_off, const int32_t *seg_tid, const uint32_t *seg_start, const uint32_t *seg_end, const uint8_t *reverse) {
    static const char who[] = "rsqc_genebody_begin";
    if (!c) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (n_genes < 0 || (n_genes && (!seg_off || !reverse))) return fail(c, RSQC_ERR_ARG, "rsqc_genebody_begin: n_genes genes with their segment offsets and reverse bytes");
    size_t n_seg = 0;
    int rc;
    if ((rc = gene_begin_check(c, who, "gene-body", c->genebody, n_genes, seg_off, seg_tid, seg_start, seg_end, &n_seg))) return rc;
    GenebodyPlan P;
    genebody_plan(n_genes, seg_off, seg_start, seg_end, reverse, RSQC_GENEBODY_ITEM, P);
    genebody_drop(c, false);
    GenebodyState &G = c->genebody;
    const std::string sizes = gene_sizes(n_genes, n_seg, P.items.size());
    const size_t sum_bytes = (size_t)n_genes * RSQC_GENEBODY_BINS * 8;
    if ((rc = gene_reserve(c, who, G.sums, sum_bytes + 64, "the sums", sizes)) ||
        (rc = gene_upload(c, who, G, sizes, n_genes, n_seg, seg_tid, seg_start, seg_end, P.items.data(), P.items.size(), sizeof(GenebodyItem))) ||
        (rc = gene_reserve(c, who, G.total, 64, "the total", sizes))) return rc;
    HIP_TRY(c, hipMemsetAsync(G.sums.p, 0, sum_bytes + 64, c->stream));
    HIP_TRY(c, hipMemsetAsync(G.total.p, 0, 64, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    G.info.n_genes = (uint64_t)n_genes; G.info.n_measured = P.n_measured; G.info.model_bases = P.model_bases;
    G.active = true;
    return RSQC_OK;
}

int rsqc_genebody_end(rsqc_ctx *c, rsqc_genebody_info *out) {
    if (!c || !out) return RSQC_ERR_ARG;
    if (int rc = gene_end(c, c->genebody, "rsqc_genebody_begin", "rsqc_genebody_end", genebody_end_run)) return rc;
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
    const size_t bytes = (size_t)n * RSQC_GENEBODY_BINS * 8;
    if (bytes) {
        HIP_TRY(c, hipSetDevice(c->device));
        if (!host_reserve(G.h_sums, bytes)) return fail(c, RSQC_ERR_CAPACITY, "rsqc_genebody_sums: no page-locked memory for a window of " + std::to_string(bytes) + " bytes");
        HIP_TRY(c, hipMemcpyAsync(G.h_sums.p, (const uint64_t *)G.sums.p + (size_t)first_gene * RSQC_GENEBODY_BINS, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    *sums = (const uint64_t *)G.h_sums.p;              // (no gene: may be NULL)
    return RSQC_OK;
}
