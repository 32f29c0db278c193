// rsqc_api.cpp -- the C ABI of include/rnaseqc_amd.h on top of the HIP kernels: a context's lifetime and inputs (the rest: rsqc_ctx.h).
// One context = one GPU = one shard of contigs.  Everything the per-record path reads
// (annotation index, uploaded batches) and writes (count vectors, per-base coverage,
// de-dup tables) stays resident in HBM; the host only builds the index once, enqueues
// work on the context's stream and reads the small result vectors back at end of file.
// There is no CPU fallback: without a HIP device rsqc_create() fails.
#include "rsqc_ctx.h"
#include "rsqc_index.h"

namespace rsqc {

int fail(rsqc_ctx *c, int code, const std::string &msg) {
    if (c) { c->last_error = msg; }
    return code;
}
int dev_alloc(rsqc_ctx *c, DevBuf &b, size_t bytes, bool zero) {
    if (bytes == 0) bytes = 16;
    bytes = (bytes + 15) & ~(size_t)15;          // whole 16-byte vectors (the reset kernel clears uint4s)
    if (b.bytes < bytes) {
        b.release();
        HIP_TRY(c, hipMalloc(&b.p, bytes));
        b.bytes = bytes;
    }
    if (zero) HIP_TRY(c, hipMemsetAsync(b.p, 0, b.bytes, c->stream));
    return 0;
}
bool dev_reserve(DevBuf &b, size_t bytes) {
    if (b.bytes >= bytes) return true;
    b.release();
    if (hipMalloc(&b.p, bytes) != hipSuccess) { (void)hipGetLastError(); b.p = nullptr; return false; }
    b.bytes = bytes;
    return true;
}
bool host_reserve(HostBuf &b, size_t bytes) {
    if (b.bytes >= bytes) return true;
    b.release();
    if (hipHostMalloc(&b.p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); b.p = nullptr; return false; }
    b.bytes = bytes;
    return true;
}

static int zero_accumulators(rsqc_ctx *c) {
    // one zeroing kernel + one store (rl_stats[1] = min l_qseq starts at UINT_MAX) instead of several memsets
    launch_reset(c->stream, c->d_arena.p, c->arena_bytes, c->d_cov.p, c->d_cov.bytes, (uint32_t *)((char *)c->d_arena.p + c->off_misc + 36));
    HIP_TRY(c, hipGetLastError());
    for (auto &pb : c->pair_pool) pb.used = false;
    c->pairs_in_flight.clear();
    c->pair_arena.used = c->frag_arena.used = c->gc_arena.used = 0;
    for (auto &fb : c->frag_pool) fb.used = false;
    c->frags_in_flight.clear();
    c->h_fsize.clear(); c->h_fcount.clear();
    c->frag_remaining = c->have_bed ? c->params.fragment_samples : 0;
    for (auto &gb : c->gc_pool) gb.used = false;
    c->gcs_in_flight.clear();
    if (c->have_ref) {
        HIP_TRY(c, hipMemsetAsync(c->d_gc_bins.p, 0, (RSQC_GC_BINS + 1) * 8, c->stream));
        c->h_gc.assign(RSQC_GC_BINS + 1, 0);
    }
    c->finalized = false;
    c->next_record_base = 0; c->name_mode = -1; c->have_ranges = false; c->have_composed_rl = false;
    c->batch_file_index.clear(); c->batch_records.clear();
    c->h_rl_offset.clear(); c->h_rl_span.clear(); c->h_rl_state.clear();
    c->h_sample_file.clear(); c->h_sample_size.clear(); c->frag_kept = 0;
    c->sticky = 0;
    return 0;
}

}  // namespace rsqc

int rsqc_create(const rsqc_params *params, rsqc_ctx **out) {
    if (!params || !out) return RSQC_ERR_ARG;
    if (params->abi_version != RSQC_ABI_VERSION) return RSQC_ERR_ARG;
    if (params->n_filter_tags < 0 || params->n_filter_tags > RSQC_MAX_FILTER_TAGS) return RSQC_ERR_ARG;
    if (params->bias_offset < 0 || params->bias_window < 1 || params->bias_window > RSQC_MAX_BIAS_WINDOW) return RSQC_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RSQC_ERR_NO_DEVICE;
    if (params->device < 0 || params->device >= ndev) return RSQC_ERR_NO_DEVICE;
    rsqc_ctx *c = new rsqc_ctx();
    c->params = *params;
    c->device = params->device;
    // Stream priorities (RSQC_STREAM_PRIO = 1 or 2; default 0 = none): the context's stream -- the per-record kernels and the fragment-counting
    // chain, the end-of-file stage's critical path -- above the side streams of the coverage kernels.  Measured (calls r6i, r6l): the fragment
    // scatter gets faster (1.24 -> 1.00 ms), the coverage kernels and the fragment count behind them slower, the stage's end does not move:
    // it is the SUM of the kernels' work on the chip that sets it.  Left as a switch.
    if (const char *e = getenv("RSQC_STREAM_PRIO")) c->stream_prio = atoi(e);
    int prio_least = 0, prio_greatest = 0;
    if (hipSetDevice(c->device) == hipSuccess) (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    c->prio_side = c->stream_prio ? prio_least : 0;
    if (hipSetDevice(c->device) != hipSuccess ||
        (c->stream_prio == 1 ? hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_greatest) : hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
        delete c;
        return RSQC_ERR_HIP;
    }
    c->dparams.mapq_threshold = params->mapq_threshold;
    c->dparams.base_mismatch = params->base_mismatch;
    c->dparams.chimeric_distance = params->chimeric_distance;
    c->dparams.stranded = params->stranded;
    c->dparams.unpaired = params->unpaired;
    c->dparams.exclude_chimeric = params->exclude_chimeric;
    c->dparams.n_filter_tags = params->n_filter_tags;
    c->dparams.legacy = params->legacy ? 1 : 0;
    c->pair_arena.n_col = 1; c->pair_arena.width[0] = sizeof(PairRec);   // {gene, second name hash, name hash}
    c->frag_arena.n_col = 6; { const size_t w[6] = {8, 8, 4, 4, 4, 4}; for (int k = 0; k < 6; ++k) c->frag_arena.width[k] = w[k]; }   // ..., second name hash
    c->gc_arena.n_col = 7; { const size_t w[7] = {8, 8, 4, 4, 4, 4, 4}; for (int k = 0; k < 7; ++k) c->gc_arena.width[k] = w[k]; }   // ..., second name hash
    if (const char *e = getenv("RSQC_K1_GRID")) c->k1_grid = std::min(16384, std::max(1, atoi(e)));
    *out = c;
    return RSQC_OK;
}

void rsqc_destroy(rsqc_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto *u : c->resident) if (u) free_batch(u);
    for (auto *u : c->transient) free_batch(u);
    for (auto &b : c->upload_pool) b.release();
    for (auto &b : c->ann_bufs) b.release();
    for (auto &pb : c->pair_pool) { pb.rec.release(); pb.counts.release(); if (pb.h_counts) (void)hipHostFree(pb.h_counts); if (pb.done) (void)hipEventDestroy(pb.done); if (pb.kernels) (void)hipEventDestroy(pb.kernels); }
    for (auto &fb : c->frag_pool) { fb.file.release(); fb.qhash.release(); fb.name.release(); fb.endpos.release(); fb.fs.release(); fb.h2.release(); fb.count.release(); fb.r_file.release(); fb.r_qhash.release(); fb.r_name.release(); fb.r_endpos.release(); fb.r_fs.release(); fb.r_h2.release(); fb.r_counts.release(); if (fb.h_count) (void)hipHostFree(fb.h_count); }
    for (auto &gb : c->gc_pool) { gb.file.release(); gb.qhash.release(); gb.row.release(); gb.endpos.release(); gb.flag_lq.release(); gb.tid.release(); gb.h2.release(); gb.count.release(); if (gb.h_count) (void)hipHostFree(gb.h_count); }
    for (Arena *a : {&c->pair_arena, &c->frag_arena, &c->gc_arena}) for (int k = 0; k < a->n_col; ++k) a->col[k].release();
    c->d_arena_count.release(); c->d_rl_summary.release();
    {
        DecodeState &D = c->dec;
        for (DevBuf *b : {&D.comp, &D.blocks, &D.ubuf, &D.seg, &D.seg_rec0, &D.seg_ops0, &D.rec_off, &D.ops_at, &D.mark, &D.core, &D.aux, &D.qh2, &D.cigar,
                          &D.seg_tid, &D.seg_start, &D.wide_index, &D.wide_nm, &D.wide_lq, &D.wide_nc, &D.sum, &D.carry, &D.tailtmp, &D.scratch, &D.umi}) b->release();
        if (D.h_sum) (void)hipHostFree(D.h_sum);
        if (D.h_blocks) (void)hipHostFree(D.h_blocks);
        if (D.ev_copy) (void)hipEventDestroy(D.ev_copy);
        if (D.copy_stream) (void)hipStreamDestroy(D.copy_stream);
        for (auto &e : D.pe) if (e) (void)hipEventDestroy(e);
    }
    sort_drop(c);
    markdup_drop(c);
    junction_drop(c, true);
    track_drop(c, true);
    genebody_drop(c, true);
    tin_drop(c, true);
    window_stages_drop(c, true, true);
    for (auto &b : c->parked) b.release();
    free_sort_scratch(c->gc_scratch); free_sort_scratch(c->frag_scratch);
    c->d_ref_bits.release(); c->d_ref_off.release(); c->d_ref_len.release(); c->d_gc_bins.release(); c->d_exon_gc.release();
    DevBuf *all[] = {&c->d_arena, &c->d_cov, &c->d_ovf_index, &c->d_tiles, &c->d_defer, &c->d_ei_rank, &c->d_table, &c->d_tab_off, &c->d_tab_cap};
    if (c->h_arena) (void)hipHostFree(c->h_arena);
    if (c->h_rl_raw) (void)hipHostFree(c->h_rl_raw);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    if (c->stream3) (void)hipStreamDestroy(c->stream3);
    if (c->stream4) (void)hipStreamDestroy(c->stream4);
    if (c->ev_join3) (void)hipEventDestroy(c->ev_join3);
    if (c->ev_join4) (void)hipEventDestroy(c->ev_join4);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_retired) (void)hipEventDestroy(c->ev_retired);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    for (auto *b : all) b->release();
    for (auto &pr : c->k1_events) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (auto &pr : c->long_events) (void)hipEventDestroy(pr.second);      // (.first is the K1 pair's second event)
    for (auto e : c->event_pool) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

int rsqc_set_annotation(rsqc_ctx *c, const rsqc_annotation *a, const uint8_t *owned_contig) {
    if (!c || !a) return RSQC_ERR_ARG;
    if (c->have_ann) return fail(c, RSQC_ERR_ARG, "annotation already set");
    HIP_TRY(c, hipSetDevice(c->device));
    const int nc = a->n_contigs, G = a->n_genes, L = a->n_genes_listed, E = a->n_exons;
    c->n_ref = a->n_ref; c->n_contigs = nc; c->n_genes = G; c->n_listed = L; c->n_exons = E;
    HostIndex hx;
    {
        std::string err;
        int brc = hx.build(a, owned_contig, err);
        if (brc) return fail(c, brc, err);
    }
    const uint64_t run = hx.cov_entries;
    c->cov_entries = run;
    c->exon_row_id.assign(a->exon_row_id, a->exon_row_id + E);

    // ---- upload ---------------------------------------------------------------------------------
    DevAnnotation &d = c->dann;
    d.n_ref = a->n_ref; d.n_contigs = nc; d.n_genes = G; d.n_listed = L; d.n_exons = E;
    d.bin_shift = HostIndex::kBinShift;
    int rc;
#define UPV(dst, vec) if ((rc = upload(c, c->ann_bufs, (vec).data(), (vec).size(), &(dst)))) return rc
#define UPA(dst, ptr, n) if ((rc = upload(c, c->ann_bufs, (ptr), (size_t)(n), &(dst)))) return rc
    UPV(d.ex, hx.ex_rows); UPV(d.gb, hx.gb); UPV(d.contig, hx.contig);
    UPV(d.ex_binhi, hx.ex_binhi); UPV(d.gb_bin, hx.gb_bin); UPV(d.ex_cov, hx.ex_cov); UPV(d.ex_pmax, hx.ex_pmax);
    UPV(d.ex_id, c->exon_row_id);
    UPV(d.ei, hx.ei); UPV(d.ei_coarse, hx.ei_coarse);
    if ((rc = dev_alloc(c, c->d_ei_rank, ((size_t)hx.rank_words + 1) * sizeof(EiRank), true)))
        return fail(c, rc, "no device memory for the interval index's rank table: " + std::to_string((((size_t)hx.rank_words + 1) * sizeof(EiRank)) >> 20) +
                           " MiB (16 bytes per 64 positions up to every contig's last feature; 775 MB for the human contig lengths)");
    d.ei_rank = (const EiRank *)c->d_ei_rank.p;
    for (int k = 0; k < nc; ++k)                  // (stream order: after the upload of the entries)
        launch_ei_rank(c->stream, d.ei, hx.ei_range[(size_t)k], hx.ei_range[(size_t)k + 1],
                       (EiRank *)c->d_ei_rank.p + hx.contig[(size_t)k].rk_base, hx.contig[(size_t)k].rk_words);
    d.legacy = nullptr;
    if (c->params.legacy) {                       // tables of the --legacy rules (rsqc_read.h: LegacyTables)
        LegacyTables lt{};
        UPV(lt.gr, hx.gr_rows); UPV(lt.gr_pmax, hx.g_pmax); UPV(lt.gr_range, hx.g_range); UPV(lt.ex_ord, hx.ex_ord); UPV(lt.gr_binhi, hx.gr_binhi);
        std::vector<LegacyTables> one(1, lt);
        UPV(d.legacy, one);
    }
    auto &gene_cov_off = hx.gene_cov_off; auto &gene_coding = hx.gene_coding;
    auto &gene_flags = hx.gene_flags; auto &gene_owned = hx.gene_owned;
    // empty BED until rsqc_set_bed
    std::vector<uint32_t> zero_range((size_t)nc + 1, 0);
    UPV(d.bed_range, zero_range);
    d.bed_start = d.bed_end = d.bed_pmax = nullptr; d.bed_binhi = d.bed_bin_base = nullptr; d.have_bed = 0;
    UPA(c->d_ge_off, a->gene_exon_off, (size_t)G + 1);
    UPA(c->d_ge_row, a->gene_exon_row, E);
    UPV(c->d_gene_cov_off, gene_cov_off);
    UPV(c->d_gene_coding, gene_coding);
    UPV(c->d_gene_flags, gene_flags);
    UPV(c->d_gene_owned, gene_owned);
    std::vector<uint32_t> gene_order((size_t)std::max(L, 1), 0);
    for (int g = 0; g < L; ++g) gene_order[(size_t)g] = (uint32_t)g;
    std::stable_sort(gene_order.begin(), gene_order.begin() + L, [&](uint32_t x, uint32_t y) { return gene_coding[x] > gene_coding[y]; });
    UPV(c->d_gene_order, gene_order);
    // workgroup size classes of the end-of-file coverage stage (rsqc_kernels.hip, K3)
    {
        const K3Counts k3 = k3_count_classes(gene_coding.data(), gene_order.data(), (uint32_t)L);      // (rsqc_k3_plan.h)
        c->k3_large = k3.n_large; c->k3_medium = k3.n_medium; c->k3_xlarge = k3.n_xlarge;
        c->k3_le6144 = k3.n_le6144; c->k3_le3072 = k3.n_le3072; c->k3_le2048 = k3.n_le2048; c->k3_le1024 = k3.n_le1024;
    }
#undef UPV
#undef UPA
    // ---- accumulators -----------------------------------------------------------------------------
    const size_t n_u64 = (size_t)G * 3 + RSQC_N_COUNTERS;
    const size_t Lz = (size_t)std::max(L, 1), Ez = (size_t)std::max(E, 1);
    auto pad8 = [](size_t x) { return (x + 7) & ~(size_t)7; };
    size_t at = 0;
    // three runs of one element type each, so that a sharded run sum-reduces everything with three collectives
    // (rsqc_device_vectors): u64 counts | f64 sums and owner-only statistics | u8 validity flags
    c->off_u64 = at; at += n_u64 * 8;
    c->off_bias3 = at; at += Lz * 8;
    c->off_bias5 = at; at += Lz * 8;
    c->off_exon = at; at += Ez * 8;
    c->off_gmean = at; at += Lz * 8;
    c->off_gstd = at; at += Lz * 8;
    c->off_gcv = at; at += Lz * 8;
    c->off_ecv = at; at += Ez * 8;
    c->off_gvalid = at; at += pad8(Lz);
    c->off_ecvv = at; at += pad8(Ez);
    c->off_ehit = at; at += pad8(Ez);
    at = (at + 15) & ~(size_t)15;                 // rl_stats (off_misc + 32) starts a 16-byte vector: the reset kernel arms it
    c->off_misc = at; at += 64;
    c->arena_bytes = at;
    if ((rc = dev_alloc(c, c->d_arena, at, false))) return rc;
    HIP_TRY(c, hipHostMalloc((void **)&c->h_arena, at, hipHostMallocDefault));
    if ((rc = dev_alloc(c, c->d_cov, (size_t)(run + 64) * 4, false))) return rc;
    const uint32_t ovf_cap = 1u << 20;
    if ((rc = dev_alloc(c, c->d_ovf_index, (size_t)ovf_cap * 8, false))) return rc;
    // (the side streams and their events outlive rsqc_clear_inputs: made for the first annotation, reused by the next)
    for (hipStream_t *s : {&c->stream2, &c->stream3, &c->stream4})
        if (!*s) HIP_TRY(c, hipStreamCreateWithPriority(s, hipStreamNonBlocking, c->prio_side));
    for (hipEvent_t *e : {&c->ev_join3, &c->ev_join4, &c->ev_fork, &c->ev_join, &c->ev_retired})
        if (!*e) HIP_TRY(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
    char *A = (char *)c->d_arena.p;
    DevAccum &acc = c->acc;
    acc.gene_reads = (unsigned long long *)(A + c->off_u64);
    acc.gene_unique = acc.gene_reads + G;
    acc.gene_frag = acc.gene_unique + G;
    acc.counters = acc.gene_frag + G;
    acc.exon_acc = (double *)(A + c->off_exon);
    acc.cov_diff = (uint32_t *)c->d_cov.p;
    acc.ovf_count = (uint32_t *)(A + c->off_misc);
    acc.read_length = (int32_t *)(A + c->off_misc + 8);
    acc.error = (int *)(A + c->off_misc + 16);
    acc.rl_stats = (uint32_t *)(A + c->off_misc + 32);
    acc.defer_total = (uint32_t *)(A + c->off_misc + 48);    // (zeroed with the arena, re-armed by the last kernel of every batch)
    acc.ovf_index = (uint64_t *)c->d_ovf_index.p; acc.ovf_cap = ovf_cap;
    c->have_ann = true;
    if ((rc = zero_accumulators(c))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->last_error = hx.warning;                  // (RSQC_OK with a warning: an exon outside its gene's row, see rsqc_index.h)
    c->n_exons_outside_gene = hx.n_exons_outside_gene;
    return RSQC_OK;
}

int rsqc_set_reference(rsqc_ctx *c, const rsqc_reference *ref) {
    if (!c || !ref || !c->have_ann) return RSQC_ERR_ARG;
    if (c->have_ref) return fail(c, RSQC_ERR_ARG, "reference already set");
    HIP_TRY(c, hipSetDevice(c->device));
    const int nc = c->n_contigs;
    std::vector<unsigned long long> off((size_t)nc, ~0ull), len((size_t)nc, 0ull);
    unsigned long long words = 0, longest = 0;
    for (int i = 0; i < ref->n; ++i) {
        const int k = ref->contig[i];
        if (k < 0 || k >= nc || off[(size_t)k] != ~0ull) return fail(c, RSQC_ERR_ARG, "reference contig out of range or repeated");
        if (ref->length[i] && !ref->sequence[i]) return fail(c, RSQC_ERR_ARG, "reference contig without bases");
        off[(size_t)k] = words; len[(size_t)k] = ref->length[i];
        words += (ref->length[i] + 63) / 64;
        longest = std::max<unsigned long long>(longest, ref->length[i]);
    }
    int rc;
    if ((rc = dev_alloc(c, c->d_ref_bits, (size_t)(words + 2) * 8, false)) || (rc = dev_alloc(c, c->d_ref_off, (size_t)std::max(nc, 1) * 8, false)) ||
        (rc = dev_alloc(c, c->d_ref_len, (size_t)std::max(nc, 1) * 8, false)) || (rc = dev_alloc(c, c->d_gc_bins, (RSQC_GC_BINS + 1) * 8, false)) ||
        (rc = dev_alloc(c, c->d_exon_gc, (size_t)std::max(c->n_exons, 1) * 8, false))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_ref_off.p, off.data(), (size_t)nc * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_ref_len.p, len.data(), (size_t)nc * 8, hipMemcpyHostToDevice, c->stream));
    // the bases pass through one staging buffer sized for the longest contig and are packed to one bit each
    DevBuf stage;
    if ((rc = dev_alloc(c, stage, (size_t)longest + 64, false))) return rc;
    for (int i = 0; i < ref->n; ++i) {
        if (!ref->length[i]) continue;
        HIP_TRY(c, hipMemcpyAsync(stage.p, ref->sequence[i], (size_t)ref->length[i], hipMemcpyHostToDevice, c->stream));
        launch_gc_pack(c->stream, (const uint8_t *)stage.p, ref->length[i], (unsigned long long *)c->d_ref_bits.p + off[(size_t)ref->contig[i]]);
        HIP_TRY(c, hipStreamSynchronize(c->stream));          // the caller's string and the staging buffer are reused
    }
    stage.release();
    c->dref = DevReference{(const unsigned long long *)c->d_ref_bits.p, (const unsigned long long *)c->d_ref_off.p,
                           (const unsigned long long *)c->d_ref_len.p};
    launch_exon_gc(c->stream, c->dann, c->dref, (double *)c->d_exon_gc.p);
    c->h_exon_gc.assign((size_t)std::max(c->n_exons, 1), -1.0);
    HIP_TRY(c, hipMemcpyAsync(c->h_exon_gc.data(), c->d_exon_gc.p, (size_t)c->n_exons * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_gc_bins.p, 0, (RSQC_GC_BINS + 1) * 8, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    c->h_gc.assign(RSQC_GC_BINS + 1, 0);
    c->have_ref = true;
    return RSQC_OK;
}

int rsqc_set_bed(rsqc_ctx *c, const rsqc_bed *bed) {
    if (!c || !bed || !c->have_ann) return RSQC_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const int nc = c->n_contigs, n = bed->n_intervals;
    std::vector<uint32_t> range((size_t)nc + 1, 0);
    std::vector<int32_t> pmax((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (bed->contig[i] < 0 || bed->contig[i] >= nc) return fail(c, RSQC_ERR_ARG, "BED contig out of range");
        if (i && (bed->contig[i] < bed->contig[i - 1] ||
                  (bed->contig[i] == bed->contig[i - 1] && bed->start[i] < bed->start[i - 1])))
            return fail(c, RSQC_ERR_ARG, "BED intervals must be grouped by contig id and ascending by start");
        range[(size_t)bed->contig[i] + 1]++;
    }
    for (int k = 0; k < nc; ++k) range[(size_t)k + 1] += range[(size_t)k];
    for (int k = 0; k < nc; ++k) {
        int32_t m = INT32_MIN;
        for (uint32_t i = range[(size_t)k]; i < range[(size_t)k + 1]; ++i) { m = std::max(m, bed->end[i]); pmax[i] = m; }
    }
    int rc;
    if ((rc = upload(c, c->ann_bufs, bed->start, (size_t)n, &c->dann.bed_start))) return rc;
    if ((rc = upload(c, c->ann_bufs, bed->end, (size_t)n, &c->dann.bed_end))) return rc;
    if ((rc = upload(c, c->ann_bufs, pmax.data(), pmax.size(), &c->dann.bed_pmax))) return rc;
    if ((rc = upload(c, c->ann_bufs, range.data(), range.size(), &c->dann.bed_range))) return rc;
    {   // bin table (DevAnnotation::bed_binhi): a block's upper bound is one load and a short step down
        std::vector<uint32_t> bin_base((size_t)nc + 1, 0), binhi;
        for (int k = 0; k < nc; ++k) {
            const uint32_t lo = range[(size_t)k], hi = range[(size_t)k + 1];
            const int32_t top = hi > lo ? std::max(bed->start[hi - 1], 0) : 0;
            const uint32_t nb = hi > lo ? ((uint32_t)top >> RSQC_BED_BIN_SHIFT) + 1u : 1u;
            bin_base[(size_t)k + 1] = bin_base[(size_t)k] + nb;
            uint32_t row = lo;
            for (uint32_t b = 0; b < nb; ++b) {
                const int64_t limit = ((int64_t)b + 1) << RSQC_BED_BIN_SHIFT;
                while (row < hi && (int64_t)bed->start[row] < limit) ++row;
                binhi.push_back(row);
            }
        }
        if ((rc = upload(c, c->ann_bufs, binhi.data(), binhi.size(), &c->dann.bed_binhi))) return rc;
        if ((rc = upload(c, c->ann_bufs, bin_base.data(), bin_base.size(), &c->dann.bed_bin_base))) return rc;
    }
    c->dann.have_bed = 1;
    c->have_bed = true;
    c->frag_remaining = c->params.fragment_samples;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RSQC_OK;
}

int rsqc_reset(rsqc_ctx *c) {
    if (!c || !c->have_ann) return RSQC_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    RSQC_TRACE("reset: enter");
    if (c->sort.active || c->sort.core.p) sort_drop(c);
    markdup_drop(c);
    junction_drop(c, false);                           // (the columns stay for the next pass)
    track_drop(c, false);                              // (and so does the difference array)
    genebody_drop(c, false);
    tin_drop(c, false);
    window_stages_drop(c, false, false);               // (the tables stay allocated, the packed reference and the sites' buffers too; the next begin uploads its own sites)
    const int rc = zero_accumulators(c);
    RSQC_TRACE("reset: enqueued");
    return rc;
}

int rsqc_clear_inputs(rsqc_ctx *c) {
    if (!c) return RSQC_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    // everything in flight: the batches on the main stream, the end-of-file stage's side streams, the decode's copy stream
    for (hipStream_t s : {c->dec.copy_stream, c->stream, c->stream2, c->stream3, c->stream4})
        if (s) HIP_TRY(c, hipStreamSynchronize(s));
    if (int rc = resolve_events(c)) return rc;
    if (c->fin_e0) { c->event_pool.push_back(c->fin_e0); c->event_pool.push_back(c->fin_e1); c->fin_e0 = c->fin_e1 = nullptr; }
    for (auto *u : c->transient) retire_batch(c, u);
    c->transient.clear();
    free_parked(c);
    sort_drop(c);
    markdup_drop(c);
    junction_drop(c, false);
    track_drop(c, false);
    genebody_drop(c, false);
    tin_drop(c, false);
    window_stages_drop(c, false, true);                // (the reference and the sites go with the inputs, and those stages' tables with them)
    // an open decode stream is dropped with its carried-over bytes; its window buffers stay
    c->dec.active = false; c->dec.pending = false; c->dec.tail = 0;
    // the batches in flight hand their buffers back to the pools; what the pass has emitted so far goes with the arenas
    for (auto &pb : c->pair_pool) pb.used = false;
    for (auto &fb : c->frag_pool) fb.used = false;
    for (auto &gb : c->gc_pool) gb.used = false;
    c->pairs_in_flight.clear(); c->frags_in_flight.clear(); c->gcs_in_flight.clear();
    for (Arena *a : {&c->pair_arena, &c->frag_arena, &c->gc_arena}) {
        for (int k = 0; k < a->n_col; ++k) a->col[k].release();
        a->used = a->cap = 0;
    }
    // the annotation, the BED and the reference, and everything sized from them
    for (auto &b : c->ann_bufs) b.release();
    c->ann_bufs.clear();
    for (DevBuf *b : {&c->d_arena, &c->d_cov, &c->d_ei_rank, &c->d_ovf_index, &c->d_table, &c->d_tab_off, &c->d_tab_cap,
                      &c->d_ref_bits, &c->d_ref_off, &c->d_ref_len, &c->d_gc_bins, &c->d_exon_gc,
                      &c->d_rl_summary}) b->release();          // (the per-batch Read-Length summaries, 17 MB: made again by the next pass's first batch)
    if (c->h_arena) { (void)hipHostFree(c->h_arena); c->h_arena = nullptr; }
    c->arena_bytes = 0;
    c->dann = DevAnnotation{}; c->dref = DevReference{};
    uint32_t *const tile_span = c->acc.tile_span;          // (d_tiles is sized by the batches, not by the annotation: kept)
    c->acc = DevAccum{}; c->acc.tile_span = tile_span;
    c->d_ge_off = c->d_ge_row = c->d_gene_cov_off = c->d_gene_coding = c->d_gene_order = nullptr;
    c->d_gene_flags = c->d_gene_owned = nullptr;
    c->n_ref = c->n_contigs = c->n_genes = c->n_listed = c->n_exons = 0;
    c->k3_large = c->k3_medium = c->k3_xlarge = c->k3_le6144 = c->k3_le3072 = c->k3_le2048 = c->k3_le1024 = 0;
    c->cov_entries = 0; c->n_exons_outside_gene = 0;
    std::vector<uint32_t>().swap(c->exon_row_id);
    std::vector<double>().swap(c->h_exon_gc);
    c->h_gc.clear();
    c->have_ann = c->have_bed = c->have_ref = false;
    // the pass that was open, as rsqc_reset leaves it
    free_sort_scratch(c->gc_scratch); free_sort_scratch(c->frag_scratch);
    c->h_fsize.clear(); c->h_fcount.clear(); c->frag_remaining = 0; c->frag_kept = 0;
    c->finalized = false; c->early_copied = false;
    c->next_record_base = 0; c->name_mode = -1; c->have_ranges = false; c->have_composed_rl = false;
    c->batch_file_index.clear(); c->batch_records.clear();
    c->h_rl_offset.clear(); c->h_rl_span.clear(); c->h_rl_state.clear();
    c->h_sample_file.clear(); c->h_sample_size.clear();
    c->results = rsqc_results{};
    c->sticky = 0;
    c->last_error.clear();
    return RSQC_OK;
}

void *rsqc_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
void rsqc_host_free(void *p) { if (p) (void)hipHostFree(p); }

const char *rsqc_strerror(int code) {
    switch (code) {
    case RSQC_OK: return "ok";
    case RSQC_ERR_ARG: return "bad argument or call order";
    case RSQC_ERR_HIP: return "HIP runtime error";
    case RSQC_ERR_BAD_CIGAR: return "Unrecognized Cigar Op";
    case RSQC_ERR_CAPACITY: return "device-side capacity exceeded";
    case RSQC_ERR_NO_DEVICE: return "no usable HIP device (this library has no CPU path)";
    case RSQC_ERR_EMPTY_MEDIAN: return "Cannot compute median of an empty list";
    case RSQC_ERR_INPUT: return "corrupt or truncated BAM input";
    default: return "unknown error";
    }
}

const char *rsqc_last_error(rsqc_ctx *c) { return c ? c->last_error.c_str() : ""; }

static const char *const kCounterNames[RSQC_N_COUNTERS] = {
    "Alternative Alignments", "Supplementary Alignments", "Failed Vendor QC", "Low Mapping Quality",
    "Chimeric Fragments_auto", "Chimeric Fragments_tag", "Unique Mapping, Vendor QC Passed Reads",
    "Unpaired Reads", "Mapped Reads", "Mapped Duplicate Reads", "Mapped Unique Reads",
    "Total Mapped Pairs", "End 1 Mapped Reads", "End 1 Mismatches", "End 1 Bases", "Duplicate Pairs",
    "Unique Fragments", "End 2 Mapped Reads", "End 2 Mismatches", "End 2 Bases", "Mismatched Bases",
    "Total Bases", "High Quality Reads", "Low Quality Reads", "Reads used for Intron/Exon counts",
    "Alignment Blocks", "Non-Globin Reads", "Non-Globin Duplicate Reads", "Intronic Reads",
    "Intragenic Reads", "HQ Intronic Reads", "HQ Intragenic Reads", "Intergenic Reads",
    "HQ Intergenic Reads", "Exonic Reads", "HQ Exonic Reads", "Ambiguous Reads", "HQ Ambiguous Reads",
    "rRNA Reads", "End 1 Sense", "End 1 Antisense", "End 2 Sense", "End 2 Antisense",
    "Total Alignments", "Filtered by tag: 0", "Filtered by tag: 1", "Filtered by tag: 2",
    "Filtered by tag: 3", "Filtered by tag: 4", "Split Reads",
};
static_assert(sizeof(kCounterNames) / sizeof(kCounterNames[0]) == RSQC_N_COUNTERS, "one name per counter");

const char *rsqc_counter_name(int counter) {
    return (counter >= 0 && counter < RSQC_N_COUNTERS) ? kCounterNames[counter] : "";
}

const char *rsqc_version(void) { return "RNASeQC 2.4.3 (rnaseqc_amd 0.1, MI355X/gfx950)"; }

uint64_t rsqc_qname_hash(const char *name, size_t len) {
    uint64_t h = 0xCBF29CE484222325ull;                    // FNV-1a 64
    for (size_t i = 0; i < len; ++i) { h ^= (uint8_t)name[i]; h *= 0x100000001B3ull; }
    h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull; h ^= h >> 33;   // fmix64
    return h;
}

uint32_t rsqc_qname_hash2(const char *name, size_t len) { return rsqc::bam_qname_hash2((const uint8_t *)name, (uint32_t)len); }
uint64_t rsqc_umi_pack(const char *umi, uint32_t len) { return umi ? rsqc::umi_pack((const uint8_t *)umi, len) : 0ull; }
