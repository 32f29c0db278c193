// rsqc_finalize.cpp -- end of file: the coverage / fragment / GC kernels, the read-back of the result vectors, shard summaries, timing.
#include "rsqc_ctx.h"
#include "rsqc_rl_compose.h"

// The device holds every result vector in its final order (genes by listed id, exons by exon id), so the read-back
// is ONE D2H of the arena into the page-locked mirror; the results struct points straight into the mirror.
static int read_back(rsqc_ctx *c) {
    const int G = c->n_genes, L = c->n_listed, E = c->n_exons;
    char *A = (char *)c->d_arena.p;
    if (c->early_copied) {                           // (run_finalize_kernels sent the rest ahead, beside the fragment kernels)
        const size_t frag_lo = c->off_u64 + (size_t)2 * (size_t)G * 8;
        HIP_TRY(c, hipMemcpyAsync(c->h_arena + frag_lo, (char *)c->d_arena.p + frag_lo, (size_t)G * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->h_arena + c->off_misc, (char *)c->d_arena.p + c->off_misc, c->arena_bytes - c->off_misc, hipMemcpyDeviceToHost, c->stream));
        c->early_copied = false;
        RSQC_TRACE("read_back: copies enqueued");
    } else {
        launch_pack_results(c->stream, (const double *)(A + c->off_exon), (uint8_t *)(A + c->off_ehit), (uint32_t)E);
        HIP_TRY(c, hipMemcpyAsync(c->h_arena, c->d_arena.p, c->arena_bytes, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    RSQC_TRACE("read_back: stream idle");
    char *H = c->h_arena;
    uint64_t *u = (uint64_t *)(H + c->off_u64);
    rsqc_results &R = c->results;
    for (int k = 0; k < RSQC_N_COUNTERS; ++k) R.counters[k] = u[3 * (size_t)G + (size_t)k];
    R.n_genes_listed = L; R.n_exons = E;
    R.gene_reads = u; R.gene_unique = u + G; R.gene_fragments = u + 2 * (size_t)G;
    R.exon_reads = (double *)(H + c->off_exon); R.exon_hit = (uint8_t *)(H + c->off_ehit);
    R.read_length = c->have_composed_rl ? c->composed_rl : *(const int32_t *)(H + c->off_misc + 8);
    R.gene_cov_mean = (double *)(H + c->off_gmean); R.gene_cov_std = (double *)(H + c->off_gstd); R.gene_cov_cv = (double *)(H + c->off_gcv);
    R.gene_cov_valid = (uint8_t *)(H + c->off_gvalid); R.exon_cv = (double *)(H + c->off_ecv); R.exon_cv_valid = (uint8_t *)(H + c->off_ecvv);
    R.bias_three = (uint64_t *)(H + c->off_bias3); R.bias_five = (uint64_t *)(H + c->off_bias5);
    R.n_fragment_sizes = (uint32_t)c->h_fsize.size();
    R.fragment_size = c->h_fsize.data(); R.fragment_count = c->h_fcount.data();
    R.fragment_samples_remaining = c->frag_remaining;
    R.have_reference = c->have_ref ? 1 : 0;
    R.gc_bins = c->have_ref ? c->h_gc.data() : nullptr;
    R.gc_out_of_range = c->have_ref ? c->h_gc[RSQC_GC_BINS] : 0;
    R.exon_gc = c->have_ref ? c->h_exon_gc.data() : nullptr;
    R.exons_outside_gene_row = c->n_exons_outside_gene;
    c->timing.slow_records = *(const uint32_t *)(H + c->off_misc + 4);
    const int err = *(const int *)(H + c->off_misc + 16);
    if (err) {
        c->sticky = err;
        return fail(c, err, device_error_message(c, err));
    }
    return 0;
}

// end-of-file kernels (K3 beside K4, K5 for BED runs); results stay on the device
static int run_finalize_kernels(rsqc_ctx *c, bool early_readback = false) {
    int rc;
    c->early_copied = false;
    const int G = c->n_genes, L = c->n_listed;
    char *A = (char *)c->d_arena.p;
    hipEvent_t e0 = get_event(c), e1 = get_event(c);
        HIP_TRY(c, hipEventRecord(e0, c->stream));
        // the side streams start from here (recorded BEFORE the K4 kernels are enqueued on the main stream)
        HIP_TRY(c, hipEventRecord(c->ev_fork, c->stream));
        // ---- K3 on the side streams: coverage scan + per-gene statistics + bias.  Enqueued BEFORE the fragment stage: with several batches
        //      in flight that stage begins with a host-side wait (retire_completed below), and the coverage kernels -- which depend on
        //      the fork event only -- would otherwise not even be queued while the host sleeps -----------------------
        HIP_TRY(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
        HIP_TRY(c, hipStreamWaitEvent(c->stream3, c->ev_fork, 0));
        HIP_TRY(c, hipStreamWaitEvent(c->stream4, c->ev_fork, 0));
        GeneCovArgs Ga{};
        Ga.ge_off = c->d_ge_off; Ga.ge_row = c->d_ge_row;
        Ga.ex = c->dann.ex; Ga.ex_cov = c->dann.ex_cov; Ga.ex_id = c->dann.ex_id;
        Ga.gene_cov_off = c->d_gene_cov_off; Ga.gene_coding = c->d_gene_coding;
        Ga.gene_flags = c->d_gene_flags; Ga.gene_owned = c->d_gene_owned;
        Ga.gene_order = c->d_gene_order;
        Ga.gene_reads = c->acc.gene_reads; Ga.cov = c->acc.cov_diff; Ga.n_listed = L;
        Ga.mask = c->params.coverage_mask; Ga.bias_offset = c->params.bias_offset; Ga.bias_window = c->params.bias_window;
        Ga.bias_gene_length = c->params.bias_gene_length;
        Ga.g_mean = (double *)(A + c->off_gmean); Ga.g_std = (double *)(A + c->off_gstd); Ga.g_cv = (double *)(A + c->off_gcv);
        Ga.g_valid = (uint8_t *)(A + c->off_gvalid); Ga.e_cv = (double *)(A + c->off_ecv); Ga.e_cv_valid = (uint8_t *)(A + c->off_ecvv);
        Ga.bias3 = (unsigned long long *)(A + c->off_bias3); Ga.bias5 = (unsigned long long *)(A + c->off_bias5);
        Ga.error = c->acc.error;
        {
            uint32_t nl = c->k3_large, nm = c->k3_medium, nx = c->k3_xlarge;
            if (const char *e = RSQC_DIAG("RSQC_K3_FORCE")) {        // diagnostic build only: 1 = all 1024-thread, 2 = all 256, 3 = all one-wave
                const int f = atoi(e);
                if (f == 1) { nl = (uint32_t)L; nm = 0; } else if (f == 2) { nl = 0; nm = (uint32_t)L; nx = 0; } else if (f == 3) { nl = 0; nm = 0; nx = 0; } else if (f == 4) { nl = (uint32_t)L; nm = 0; nx = (uint32_t)L; }
            }
            if (!RSQC_DIAG("RSQC_DIAG_SKIP_K3")) launch_gene_coverage(c->stream2, c->stream3, c->stream4, Ga, nl, nm, nx, c->k3_le6144, c->k3_le3072, c->k3_le2048, c->k3_le1024);   // (diagnostic build only: results incomplete)
        }
        // ---- K4 on the main stream: per-gene distinct QNAMEs -------------------------------------------------
        // Several batches still in flight (a host that enqueued its batches faster than the device ran them -- bench.py's resident
        // batches, one per contig of a sharded run): they are retired into the arena first, so that the fragment stage runs ONE pass
        // over one dense list instead of one launch per batch over worst-case chunk tables (26 batches: 2.0 ms of frag_local
        // instead of 1.1).  Costs one wait for the batches' kernels here; a single batch in flight is used in place, uncopied.
        // (That retire also queues the batches' fragment-size candidates into frag_arena ON THE MAIN STREAM, behind the fork event: K5, which
        //  runs beside on a stream that waits for the fork only, must wait for `ev_retired` as well -- ADVICE r6.)
        bool retired_here = false;
        if (c->pairs_in_flight.size() > 1) {
            if ((rc = retire_completed(c, true))) return rc;
            if (c->have_bed) { HIP_TRY(c, hipEventRecord(c->ev_retired, c->stream)); retired_here = true; }
        }
        uint64_t pair_bound = c->pair_arena.used;
        for (size_t idx : c->pairs_in_flight) pair_bound += c->pair_pool[idx].pairs_bound;
        {
            // streaming form: survivors appended to per-partition key lists, then counted per partition in LDS.
            // bounds from the host's pair bound: partitions <= pairs / PART_READS + G, keys <= 2 x pairs + SUB_CAP x parts
            const uint64_t Gz = (uint64_t)std::max(G, 1);
            const uint64_t parts_bound = pair_bound / RSQC_K4_PART_READS + Gz + 1;
            const uint64_t keys_bound = 2 * pair_bound + RSQC_K4_SUB_CAP * std::min<uint64_t>(parts_bound, pair_bound / RSQC_K4_PART_READS + 1) + 16 * Gz + 16;   // (+ the round-up of every gene's space to 16 entries)
            if (parts_bound > 0xFFFFFFF0ull) return fail(c, RSQC_ERR_CAPACITY, "too many fragment partitions");
            const uint64_t lay_blocks = (Gz + 1023) / 1024;
            if ((rc = dev_alloc(c, c->d_tab_off, (Gz + 2) * 28 + 64 + lay_blocks * 12 + 64, false))) return rc;  // per-gene rows | part_first | layout totals
            if ((rc = dev_alloc(c, c->d_tab_cap, parts_bound * 24 + 128, false))) return rc;                  // per-partition rows | cursor | list of the fuller ones + its counter
            if (c->d_table.bytes < (size_t)keys_bound * sizeof(FragKey)) { if ((rc = dev_alloc(c, c->d_table, (size_t)keys_bound * sizeof(FragKey) + (1u << 20), false))) return rc; }
            FragPlan P;
            P.ginfo = (uint4 *)c->d_tab_off.p;
            P.part_first = (uint32_t *)(P.ginfo + Gz + 1);
            P.blk_space = (unsigned long long *)(((uintptr_t)(P.part_first + Gz + 2) + 15) & ~(uintptr_t)15);
            P.blk_parts = (uint32_t *)(P.blk_space + lay_blocks);
            P.part_info = (uint4 *)c->d_tab_cap.p; P.cursor = (uint32_t *)(P.part_info + parts_bound);
            P.full_list = P.cursor + parts_bound; P.full_n = P.full_list + parts_bound;
            P.list = (FragKey *)c->d_table.p;
            launch_frag_layout(c->stream, c->acc.gene_reads, (uint32_t)G, P, c->acc.error);
            if (c->pair_arena.used && !RSQC_DIAG("RSQC_DIAG_SKIP_K4")) {     // the retired batches: one dense list, cut into pieces
                if ((rc = dev_alloc(c, c->d_arena_count, 16, false))) return rc;
                const uint32_t used32 = (uint32_t)c->pair_arena.used;
                HIP_TRY(c, hipMemcpyAsync(c->d_arena_count.p, &used32, 4, hipMemcpyHostToDevice, c->stream));
                DevAccum acc = c->acc;
                acc.pairs = (PairRec *)c->pair_arena.col[0].p;
                acc.pair_chunk_cap = 0; acc.pair_chunk_count = (uint32_t *)c->d_arena_count.p;
                acc.pair_slow_base = 0; acc.pair_slow_cap = used32;
                launch_frag_local(c->stream, acc, 0, P, (uint32_t)std::min<uint64_t>(4096, c->pair_arena.used / 1024 + 1));
            }
            for (size_t idx : c->pairs_in_flight) {
                if (RSQC_DIAG("RSQC_DIAG_SKIP_K4")) break;                // (diagnostic build only: results incomplete)
                PairBuf &pb = c->pair_pool[idx];
                DevAccum acc = c->acc;
                acc.pairs = (PairRec *)pb.rec.p;
                acc.pair_chunk_cap = pb.chunk_cap; acc.pair_chunk_count = (uint32_t *)pb.counts.p;
                acc.pair_slow_base = pb.slow_base; acc.pair_slow_cap = pb.slow_cap;
                acc.pair_slow_count = (uint32_t *)pb.counts.p + pb.n_chunks;
                // (--legacy: all the batch's pairs sit in its dense region -- shared by as many workgroups as a list of that size gets below,
                //  not by the 32 that serve the default rules' few thousand slow-path pairs: 9.3 -> ~1 ms per 100 M records)
                launch_frag_local(c->stream, acc, pb.n_chunks, P, c->dparams.legacy ? (uint32_t)std::min<uint64_t>(4096, pb.slow_cap / 8192 + 32) : 0u);
            }
            if (!RSQC_DIAG("RSQC_DIAG_SKIP_K4")) launch_frag_count(c->stream, (uint32_t)G, P, (uint32_t)parts_bound, c->acc.gene_frag, c->acc.error);
        }
        RSQC_TRACE("finalize: K3 + K4 enqueued");
        {   // per-batch Read-Length transfer functions (rsqc_shard_info): final since the last batch's read_length_kernel; the copy
            // goes out on a side stream behind its coverage kernel (behind frag_count on the main stream it cost a queue hand-over:
            // ~40 us) and is covered by that stream's join below; the destination is page-locked, the call returns at once
            const size_t nb = c->batch_file_index.size();
            if (nb * RSQC_RL_SUMMARY_WORDS > c->h_rl_raw_cap) {
                if (c->h_rl_raw) { (void)hipHostFree(c->h_rl_raw); c->h_rl_raw = nullptr; c->h_rl_raw_cap = 0; }
                const size_t want = std::max<size_t>(2 * nb, 64) * RSQC_RL_SUMMARY_WORDS;
                HIP_TRY(c, hipHostMalloc((void **)&c->h_rl_raw, want * 4, hipHostMallocDefault));
                c->h_rl_raw_cap = want;
            }
            RSQC_TRACE("finalize: K3 enqueued");
            if (nb) HIP_TRY(c, hipMemcpyAsync(c->h_rl_raw, c->d_rl_summary.p, nb * RSQC_RL_SUMMARY_WORDS * 4, hipMemcpyDeviceToHost, c->stream2));
            RSQC_TRACE("finalize: rl copy call returned");
        }
        HIP_TRY(c, hipEventRecord(c->ev_join3, c->stream3));
        HIP_TRY(c, hipEventRecord(c->ev_join4, c->stream4));
        if (early_readback) {
            // rsqc_finalize of ONE context: everything the fragment kernels (K4, still running on the main stream; K5 behind it) do not write --
            // all of the arena but geneFragmentCounts and the status words -- crosses PCIe NOW, behind the coverage kernels on their
            // stream, instead of behind K4 (the 9 MB copy was 0.17 ms at the end of every pass); read_back then fetches the rest
            const size_t frag_lo = c->off_u64 + (size_t)2 * (size_t)c->n_genes * 8, frag_hi = frag_lo + (size_t)c->n_genes * 8;
            HIP_TRY(c, hipStreamWaitEvent(c->stream2, c->ev_join3, 0));
            HIP_TRY(c, hipStreamWaitEvent(c->stream2, c->ev_join4, 0));
            launch_pack_results(c->stream2, (const double *)(A + c->off_exon), (uint8_t *)(A + c->off_ehit), (uint32_t)c->n_exons);
            if (frag_lo) HIP_TRY(c, hipMemcpyAsync(c->h_arena, c->d_arena.p, frag_lo, hipMemcpyDeviceToHost, c->stream2));
            HIP_TRY(c, hipMemcpyAsync(c->h_arena + frag_hi, (char *)c->d_arena.p + frag_hi, c->off_misc - frag_hi, hipMemcpyDeviceToHost, c->stream2));
            c->early_copied = true;
        }
        HIP_TRY(c, hipEventRecord(c->ev_join, c->stream2));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join3, 0));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join4, 0));
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(e1, c->stream));
        // ---- K5: fragment-size sampler (BED runs) ---------------------------------------------------
        if (c->have_bed) {
            // the batches still in flight join the retired ones in the candidate arena (file order), then one pairing pass.
            // K5 depends on the per-record kernels only (their candidates, and the counts copied behind them), not on K3 / K4: it runs BESIDE the
            // end-of-file kernels, on the side stream whose coverage class ends first (the 64 KB class: ~0.5 ms), from the moment the fork event
            // has fired -- rounds 4-6 waited for the whole stage here and ran it behind (1.3 ms of every --bed pass).  Only when the arena must
            // grow while it holds retired batches (its old columns are copied on the main stream) does the old order apply.
            uint64_t incoming = 0;
            bool beside = true;
#ifdef RSQC_K5_SERIAL
            beside = false;                                   // (A/B build: the order of rounds 4-6)
#endif
            HIP_TRY(c, hipEventSynchronize(c->ev_fork));      // every batch's kernels are done, the mirrors of the candidate counts are valid
            for (size_t k = 0; k < c->frags_in_flight.size(); ++k) incoming += *c->frag_pool[c->frags_in_flight[k]].h_count;
            if (c->frag_arena.used && c->frag_arena.used + incoming > c->frag_arena.cap) beside = false;
            hipStream_t ks = beside ? c->stream4 : c->stream;
            if (!beside) HIP_TRY(c, hipStreamSynchronize(c->stream));
            else if (retired_here) HIP_TRY(c, hipStreamWaitEvent(ks, c->ev_retired, 0));      // the arena copies of the retire above (a few small copies: the overlap with K3 / K4 stays)
            for (size_t k = 0; k < c->frags_in_flight.size(); ++k) {
                FragBuf &fb = c->frag_pool[c->frags_in_flight[k]];
                const uint32_t n = *fb.h_count;               // (copied when the batch was submitted; the stream has been synchronised)
                if (n > fb.cap) return fail(c, RSQC_ERR_CAPACITY, "fragment candidate overflow");
                const void *src[6] = {fb.file.p, fb.qhash.p, fb.name.p, fb.endpos.p, fb.fs.p, fb.h2.p};
                if ((rc = arena_append(c, c->frag_arena, src, n, ks))) return rc;
                fb.used = false;
            }
            c->frags_in_flight.clear();
            const uint64_t total = c->frag_arena.used;
            if (total > 0xFFFFFFF0ull) return fail(c, RSQC_ERR_CAPACITY, "too many fragment-size candidates");
            FragCandidates fc{(uint64_t *)c->frag_arena.col[0].p, (uint64_t *)c->frag_arena.col[1].p, (int32_t *)c->frag_arena.col[2].p,
                              (int32_t *)c->frag_arena.col[3].p, (uint32_t *)c->frag_arena.col[4].p, nullptr, (uint32_t)total, nullptr, (uint32_t *)c->frag_arena.col[5].p};
            const auto tf0 = std::chrono::steady_clock::now();
            rc = run_fragment_sizes(ks, fc, (uint32_t)total, c->params.fragment_samples, c->h_fsize, c->h_fcount,
                                    c->frag_remaining, c->frag_scratch, c->frag_kept, c->acc.error);
            if (beside && !rc) HIP_TRY(c, hipStreamSynchronize(ks));      // (run_fragment_sizes returns without a wait when it keeps no samples)
            c->timing.fragment_sizes_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tf0).count();
            if (rc) return fail(c, rc, "fragment-size stage failed");
        }
        // ---- fragment GC content (--fasta runs): the same mate pairing, no cut-off --------------------------
        if (c->have_ref && (!c->gcs_in_flight.empty() || c->gc_arena.used)) {
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            GcCandidates gc{};
            uint64_t total = 0;
            if (c->gc_arena.used == 0 && c->gcs_in_flight.size() == 1) {          // one batch: its candidate arrays are used in place
                GcBuf &gb = c->gc_pool[c->gcs_in_flight[0]];
                total = *gb.h_count;
                if (total > gb.cap) return fail(c, RSQC_ERR_CAPACITY, "GC candidate overflow");
                gc = GcCandidates{(uint64_t *)gb.file.p, (uint64_t *)gb.qhash.p, (uint32_t *)gb.row.p, (int32_t *)gb.endpos.p,
                                  (uint32_t *)gb.flag_lq.p, (int32_t *)gb.tid.p, nullptr, (uint32_t)total, (uint32_t *)gb.h2.p};
            } else {
                for (size_t k = 0; k < c->gcs_in_flight.size(); ++k) {
                    GcBuf &gb = c->gc_pool[c->gcs_in_flight[k]];
                    const uint32_t n = *gb.h_count;
                    if (n > gb.cap) return fail(c, RSQC_ERR_CAPACITY, "GC candidate overflow");
                    const void *src[7] = {gb.file.p, gb.qhash.p, gb.row.p, gb.endpos.p, gb.flag_lq.p, gb.tid.p, gb.h2.p};
                    if ((rc = arena_append(c, c->gc_arena, src, n, c->stream))) return rc;
                    gb.used = false;
                }
                c->gcs_in_flight.clear();
                total = c->gc_arena.used;
                gc = GcCandidates{(uint64_t *)c->gc_arena.col[0].p, (uint64_t *)c->gc_arena.col[1].p, (uint32_t *)c->gc_arena.col[2].p,
                                  (int32_t *)c->gc_arena.col[3].p, (uint32_t *)c->gc_arena.col[4].p, (int32_t *)c->gc_arena.col[5].p, nullptr, (uint32_t)total, (uint32_t *)c->gc_arena.col[6].p};
            }
            if (total > 0xFFFFFFF0ull) return fail(c, RSQC_ERR_CAPACITY, "too many GC candidates");
            if (total) {
                rc = run_gc_content(c->stream, gc, (uint32_t)total, c->dref, (unsigned long long *)c->d_gc_bins.p, c->gc_scratch, c->acc.error);
                if (rc) return fail(c, rc, "GC content stage failed");
            }
            HIP_TRY(c, hipMemcpyAsync(c->h_gc.data(), c->d_gc_bins.p, (RSQC_GC_BINS + 1) * 8, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
    c->fin_e0 = e0; c->fin_e1 = e1;
    return 0;
}
static void unpack_rl_summaries(rsqc_ctx *c) {           // after the stream has been synchronised
    const size_t nb = c->batch_file_index.size();
    c->h_rl_offset.assign(nb + 1, 0); c->h_rl_span.clear(); c->h_rl_state.clear();
    for (size_t k = 0; k < nb; ++k) {
        const uint32_t *w = c->h_rl_raw + k * RSQC_RL_SUMMARY_WORDS;
        const uint32_t P = std::min<uint32_t>(w[0], 128u);
        for (uint32_t j = 0; j < P; ++j) { c->h_rl_span.push_back(w[2 + 2 * j]); c->h_rl_state.push_back((int32_t)w[3 + 2 * j]); }
        c->h_rl_offset[k + 1] = (uint32_t)c->h_rl_span.size();
    }
}
// "Read Length" of a pass that held batches of several file ranges: the summaries (one transfer function per batch or range) applied in
// ascending file index from state 0 -- what read_length_kernel does on the device for a pass of plain batches (src/RNASeQC.cpp:275-278)
static int32_t compose_read_length(const rsqc_ctx *c) {
    std::vector<rsqc::RlTable> tables(c->batch_file_index.size());
    for (size_t k = 0; k < tables.size(); ++k)
        tables[k] = rsqc::RlTable{c->batch_file_index[k], c->h_rl_span.data() + c->h_rl_offset[k], c->h_rl_state.data() + c->h_rl_offset[k],
                                  c->h_rl_offset[k + 1] - c->h_rl_offset[k]};
    return rsqc::rl_compose(tables);                     // (rsqc_rl_compose.h: the loop the command line's shard merge runs too)
}
static void finish_finalize_bookkeeping(rsqc_ctx *c) {
    float ms = 0.f;
    if (c->fin_e0 && hipEventElapsedTime(&ms, c->fin_e0, c->fin_e1) == hipSuccess) c->timing.finalize_ms += ms;
    if (c->fin_e0) { c->event_pool.push_back(c->fin_e0); c->event_pool.push_back(c->fin_e1); c->fin_e0 = c->fin_e1 = nullptr; }
    resolve_events(c);
    for (auto *u : c->transient) retire_batch(c, u);
    c->transient.clear();
    unpack_rl_summaries(c);
    if (c->have_ranges) { c->composed_rl = compose_read_length(c); c->have_composed_rl = true; c->results.read_length = c->composed_rl; }
    free_parked(c);
    c->finalized = true;
}

int rsqc_finalize(rsqc_ctx *c, rsqc_results *out) {
    if (!c || !out || !c->have_ann) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (c->sort.active) return fail(c, RSQC_ERR_ARG, "rsqc_sort_end must precede rsqc_finalize (a collection of rsqc_sort_begin is open)");
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if (!c->finalized) {
        RSQC_TRACE("finalize: enter");
        if ((rc = run_finalize_kernels(c, /*early_readback=*/true))) return rc;
        RSQC_TRACE("finalize: kernels enqueued");
        // ---- one read-back of every result vector (also carries the device error flag) ----------------
        if ((rc = read_back(c))) return rc;
        finish_finalize_bookkeeping(c);
        RSQC_TRACE("finalize: bookkeeping done");
    } else if ((rc = read_back(c))) return rc;
    *out = c->results;
    return RSQC_OK;
}

int rsqc_finalize_device(rsqc_ctx *c) {
    if (!c || !c->have_ann) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (c->sort.active) return fail(c, RSQC_ERR_ARG, "rsqc_sort_end must precede rsqc_finalize_device (a collection of rsqc_sort_begin is open)");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->finalized) return RSQC_OK;
    int rc;
    if ((rc = run_finalize_kernels(c))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    finish_finalize_bookkeeping(c);
    return RSQC_OK;
}

int rsqc_device_accumulators(rsqc_ctx *c, void **u64_base, uint64_t *u64_count, void **f64_base, uint64_t *f64_count) {
    if (!c || !c->have_ann || !u64_base || !u64_count || !f64_base || !f64_count) return RSQC_ERR_ARG;
    *u64_base = (char *)c->d_arena.p + c->off_u64; *u64_count = (uint64_t)c->n_genes * 3 + RSQC_N_COUNTERS;
    *f64_base = (char *)c->d_arena.p + c->off_exon; *f64_count = (uint64_t)c->n_exons;
    return RSQC_OK;
}

int rsqc_shard_summary(rsqc_ctx *c, rsqc_shard_info *out) {
    if (!c || !out || !c->have_ann || !c->finalized) return RSQC_ERR_ARG;
    out->n_batches = (uint32_t)c->batch_file_index.size();
    out->batch_file_index = c->batch_file_index.data(); out->batch_records = c->batch_records.data();
    out->rl_offset = c->h_rl_offset.data(); out->rl_span = c->h_rl_span.data(); out->rl_state = c->h_rl_state.data();
    if (c->frag_kept && c->h_sample_file.size() != c->frag_kept) {      // fetched on demand: only sharded runs look at the samples
        HIP_TRY(c, hipSetDevice(c->device));
        c->h_sample_file.resize(c->frag_kept); c->h_sample_size.resize(c->frag_kept);
        HIP_TRY(c, hipMemcpy(c->h_sample_file.data(), c->frag_scratch.k1, (size_t)c->frag_kept * 8, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(c->h_sample_size.data(), c->frag_scratch.v1, (size_t)c->frag_kept * 4, hipMemcpyDeviceToHost));
    }
    out->n_samples = (uint32_t)c->h_sample_file.size();
    out->sample_file_index = c->h_sample_file.data(); out->sample_size = c->h_sample_size.data();
    return RSQC_OK;
}

int rsqc_device_vectors(rsqc_ctx *c, rsqc_device_range out[3]) {
    if (!c || !c->have_ann || !out) return RSQC_ERR_ARG;
    char *A = (char *)c->d_arena.p;
    out[0].base = A + c->off_u64;    out[0].count = (c->off_exon - c->off_u64) / 8;
    out[1].base = A + c->off_exon;   out[1].count = (c->off_gvalid - c->off_exon) / 8;
    out[2].base = A + c->off_gvalid; out[2].count = c->off_ehit - c->off_gvalid;
    return RSQC_OK;
}

int rsqc_refresh_results(rsqc_ctx *c, rsqc_results *out) {
    if (!c || !out || !c->have_ann || !c->finalized) return RSQC_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = read_back(c);
    if (rc) return rc;
    *out = c->results;
    return RSQC_OK;
}

int rsqc_get_timing(rsqc_ctx *c, rsqc_timing *out) {
    if (!c || !out) return RSQC_ERR_ARG;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    resolve_events(c);
    *out = c->timing;
    return RSQC_OK;
}

int rsqc_reset_timing(rsqc_ctx *c) {
    if (!c) return RSQC_ERR_ARG;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    resolve_events(c);
    c->timing = rsqc_timing{};
    return RSQC_OK;
}
