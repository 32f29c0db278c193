// rsqc_genemodel_api.cpp -- what rsqc_genebody_api.cpp and rsqc_tin_api.cpp have in common: the begin of a stage over the pass's track
// that follows a gene model (the order of the calls, the model against the track's contigs, its columns and the plan's items uploaded)
// and its end (one run a pass, never a partial result).  The public call's name is a parameter; each stage holds a model of its own.
#include "rsqc_ctx.h"
#include "rsqc_genemodel.h"

namespace rsqc {

int gene_begin_check(rsqc_ctx *c, const char *who, const char *what, const GeneStage &G, int32_t n_genes, const uint32_t *seg_off, const int32_t *seg_tid,
                     const uint32_t *seg_start, const uint32_t *seg_end, size_t *n_seg) {
    const std::string w(who);
    if (!c->track.active || c->track.done) return fail(c, RSQC_ERR_ARG, "rsqc_track_begin of the same pass must precede " + w);
    if (G.active) return fail(c, RSQC_ERR_ARG, w + ": the context holds a " + what + " model already");
    if (c->finalized || c->name_mode >= 0 || !c->batch_file_index.empty() || c->next_record_base)
        return fail(c, RSQC_ERR_ARG, w + " must precede the first submit of the pass");
    *n_seg = n_genes ? seg_off[n_genes] : 0;
    if (*n_seg && (!seg_tid || !seg_start || !seg_end)) return fail(c, RSQC_ERR_ARG, w + ": " + std::to_string(*n_seg) + " segments without their columns");
    HIP_TRY(c, hipSetDevice(c->device));
    const TrackState &T = c->track;
    std::vector<uint32_t> length((size_t)T.n + 1, 0);
    if (T.n) {                                         // (the track keeps its contigs' lengths on the device only)
        HIP_TRY(c, hipMemcpyAsync(length.data(), T.length.p, (size_t)T.n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    const std::string broken = genebody_check(n_genes, seg_off, seg_tid, seg_start, seg_end, T.n, length.data());
    if (!broken.empty()) return fail(c, RSQC_ERR_ARG, w + ": " + broken);
    return 0;
}

std::string gene_sizes(int32_t n_genes, size_t n_seg, size_t n_items) {
    return std::to_string(n_genes) + " genes, " + std::to_string(n_seg) + " segments, " + std::to_string(n_items) + " items";
}

int gene_reserve(rsqc_ctx *c, const char *who, DevBuf &b, size_t bytes, const char *what, const std::string &sizes) {
    if (dev_reserve(b, bytes)) return 0;
    return fail(c, RSQC_ERR_CAPACITY, std::string(who) + ": no device memory for " + what + " (" + std::to_string(bytes) + " bytes; " + sizes + ")");
}

int gene_upload(rsqc_ctx *c, const char *who, GeneStage &G, const std::string &sizes, int32_t n_genes, size_t n_seg, const int32_t *seg_tid,
                const uint32_t *seg_start, const uint32_t *seg_end, const void *items, size_t n_items, size_t item_bytes) {
    int rc;
    if ((rc = gene_reserve(c, who, G.seg_tid, n_seg * 4 + 64, "the model", sizes)) ||
        (rc = gene_reserve(c, who, G.seg_start, n_seg * 4 + 64, "the model", sizes)) ||
        (rc = gene_reserve(c, who, G.seg_end, n_seg * 4 + 64, "the model", sizes)) ||
        (rc = gene_reserve(c, who, G.items, n_items * item_bytes + 64, "the plan", sizes))) return rc;
    // (pageable sources: the copies have left these arrays when the calls return)
    if (n_seg) {
        HIP_TRY(c, hipMemcpyAsync(G.seg_tid.p, seg_tid, n_seg * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(G.seg_start.p, seg_start, n_seg * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(G.seg_end.p, seg_end, n_seg * 4, hipMemcpyHostToDevice, c->stream));
    }
    if (n_items) HIP_TRY(c, hipMemcpyAsync(G.items.p, items, n_items * item_bytes, hipMemcpyHostToDevice, c->stream));
    G.n_genes = n_genes; G.n_items = n_items;
    return 0;
}

void gene_drop(GeneStage &G, bool free_buffers) {
    G.active = G.done = false;
    G.n_genes = 0; G.n_items = 0;
    if (free_buffers) for (DevBuf *b : {&G.seg_tid, &G.seg_start, &G.seg_end, &G.items}) b->release();
}

int gene_end(rsqc_ctx *c, GeneStage &G, const char *begin, const char *end, int (*run)(rsqc_ctx *)) {
    if (c->sticky) return c->sticky;
    if (!G.active) return fail(c, RSQC_ERR_ARG, std::string(begin) + " must precede " + end);
    if (!c->track.active || !c->track.done) return fail(c, RSQC_ERR_ARG, std::string("rsqc_track_end must precede ") + end);
    if (!G.done) {
        HIP_TRY(c, hipSetDevice(c->device));
        const int rc = run(c);
        if (rc) { (void)hipStreamSynchronize(c->stream); c->sticky = rc; return rc; }      // never a partial result: the pass is void until rsqc_reset
        G.done = true;
    }
    return 0;
}

}  // namespace rsqc
