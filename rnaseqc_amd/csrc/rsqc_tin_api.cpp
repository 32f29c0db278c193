// rsqc_tin_api.cpp -- rsqc_tin_begin / rsqc_tin_end / rsqc_tin_rows: the model of the pass is checked, planned and uploaded at its
// begin (the part it shares with --gene-body: rsqc_genemodel_api.cpp); behind rsqc_track_end TWO kernels (rsqc_tin.hip) walk the
// scanned difference array along every measured gene -- one partial per plan item, then one row per gene in item order -- and every
// row is copied to page-locked memory of the context.
#include "rsqc_ctx.h"
#include "rsqc_tin.h"

namespace {

int tin_end_run(rsqc_ctx *c) {
    TinState &N = c->tin;
    const TrackState &T = c->track;
    N.info.depth_sum = 0; N.info.covered_bases = 0; N.info.tin_ms = 0;
    if (!N.n_genes) return 0;
    const rsqc_tin_row *h_rows = (const rsqc_tin_row *)N.h_rows.p;
    const int rc = run_timed(c, &N.info.tin_ms, [&] {
        launch_tin_items(c->stream, (const uint32_t *)T.diff.p, (const uint64_t *)T.off.p,
                         GeneModel{(const int32_t *)N.seg_tid.p, (const uint32_t *)N.seg_start.p, (const uint32_t *)N.seg_end.p},
                         (const TinItem *)N.items.p, N.n_items, (rsqc_tin_row *)N.part.p);
        launch_tin_rows(c->stream, (const rsqc_tin_row *)N.part.p, (const uint64_t *)N.item_off.p, (uint32_t)N.n_genes, (rsqc_tin_row *)N.rows.p);
    }, [&]() -> int { HIP_TRY(c, hipMemcpyAsync(N.h_rows.p, N.rows.p, (size_t)N.n_genes * sizeof(rsqc_tin_row), hipMemcpyDeviceToHost, c->stream)); return 0; });
    if (rc) return rc;
    for (int32_t g = 0; g < N.n_genes; ++g) { N.info.depth_sum += h_rows[g].depth_sum; N.info.covered_bases += h_rows[g].covered; }
    return 0;
}

}  // namespace

namespace rsqc {

void tin_drop(rsqc_ctx *c, bool free_buffers) {
    TinState &N = c->tin;
    gene_drop(N, free_buffers);
    N.info = rsqc_tin_info{};
    if (free_buffers) { N.item_off.release(); N.part.release(); N.rows.release(); N.h_rows.release(); }
}

}  // namespace rsqc

int rsqc_tin_begin(rsqc_ctx *c, int32_t n_genes, const uint32_t *seg_off, const int32_t *seg_tid, const uint32_t *seg_start, const uint32_t *seg_end) {
    static const char who[] = "rsqc_tin_begin";
    if (!c) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (n_genes < 0 || (n_genes && !seg_off)) return fail(c, RSQC_ERR_ARG, "rsqc_tin_begin: n_genes genes with their segment offsets");
    size_t n_seg = 0;
    int rc;
    if ((rc = gene_begin_check(c, who, "tin", c->tin, n_genes, seg_off, seg_tid, seg_start, seg_end, &n_seg))) return rc;
    TinPlan P;
    tin_plan(n_genes, seg_off, seg_start, seg_end, RSQC_TIN_ITEM, P);
    tin_drop(c, false);
    TinState &N = c->tin;
    const std::string sizes = gene_sizes(n_genes, n_seg, P.items.size());
    const size_t row_bytes = (size_t)n_genes * sizeof(rsqc_tin_row);
    if ((rc = gene_reserve(c, who, N.rows, row_bytes + 64, "the rows", sizes)) ||
        (rc = gene_reserve(c, who, N.part, P.items.size() * sizeof(rsqc_tin_row) + 64, "the items' partials", sizes)) ||
        (rc = gene_upload(c, who, N, sizes, n_genes, n_seg, seg_tid, seg_start, seg_end, P.items.data(), P.items.size(), sizeof(TinItem))) ||
        (rc = gene_reserve(c, who, N.item_off, P.item_off.size() * 8 + 64, "the plan", sizes))) return rc;
    if (!host_reserve(N.h_rows, row_bytes))
        return fail(c, RSQC_ERR_CAPACITY, "rsqc_tin_begin: no page-locked memory for the rows (" + std::to_string(row_bytes) + " bytes; " + sizes + ")");
    // (no memset: the kernels write every slot and row)
    HIP_TRY(c, hipMemcpyAsync(N.item_off.p, P.item_off.data(), P.item_off.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    N.info.n_genes = (uint64_t)n_genes; N.info.n_measured = P.n_measured; N.info.model_bases = P.model_bases;
    N.active = true;
    return RSQC_OK;
}

int rsqc_tin_end(rsqc_ctx *c, rsqc_tin_info *out) {
    if (!c || !out) return RSQC_ERR_ARG;
    if (int rc = gene_end(c, c->tin, "rsqc_tin_begin", "rsqc_tin_end", tin_end_run)) return rc;
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
    *rows = N.h_rows.p ? (const rsqc_tin_row *)N.h_rows.p + first_gene : nullptr;      // (no gene ever: NULL)
    return RSQC_OK;
}
