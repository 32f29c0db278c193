// rsqc_submit.cpp -- a batch on its way through the context: upload, buffer pools, the per-record kernels, retirement into the arenas.
#include "rsqc_ctx.h"
#include "rsqc_rl_compose.h"

namespace rsqc {

const char *device_error_text(int err) {
    return err == RSQC_ERR_BAD_CIGAR ? "Unrecognized Cigar Op" :
           err == RSQC_ERR_CAPACITY ? "a device-side capacity was exceeded" :
           err == RSQC_ERR_EMPTY_MEDIAN ? "Cannot compute median of an empty list" : "device error";
}
// The text of a device error word.  RSQC_ERR_CAPACITY is raised by several kernels; the one limit a caller can run into with ordinary
// input -- more than 128 prefix maxima of span in one batch or file range (read_length_kernel, rsqc_kr.h) -- is named: the kernel
// leaves the cause in the flag word of the batch's summary slot, read here (error path only; the stream is idle), and the text is
// rsqc_rl_compose.h's.
std::string device_error_message(rsqc_ctx *c, int err) {
    const size_t nb = c->batch_file_index.size();
    if (err == RSQC_ERR_CAPACITY && nb && c->d_rl_summary.p) {
        std::vector<uint32_t> flags(nb, 0u);
        if (hipMemcpy2D(flags.data(), 4, (const uint32_t *)c->d_rl_summary.p + 1, (size_t)RSQC_RL_SUMMARY_WORDS * 4, 4, nb, hipMemcpyDeviceToHost) == hipSuccess) {
            const std::string msg = rl_limit_message(flags.data(), 1, nb, c->batch_file_index.data(), c->batch_records.data());
            if (!msg.empty()) return msg;
        }
    }
    return device_error_text(err);
}
hipEvent_t get_event(rsqc_ctx *c) {
    if (!c->event_pool.empty()) { hipEvent_t e = c->event_pool.back(); c->event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}
int resolve_events(rsqc_ctx *c) {
    auto add = [&](std::vector<std::pair<hipEvent_t, hipEvent_t>> &events, auto &total, bool recycle_first) {
        for (auto &pr : events) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) total += ms;
            if (recycle_first) c->event_pool.push_back(pr.first);
            c->event_pool.push_back(pr.second);
        }
        events.clear();
    };
    add(c->k1_events, c->timing.classify_ms, true);
    add(c->long_events, c->timing.classify_long_ms, false);          // (.first is the K1 pair's second event, recycled above)
    add(c->h2d_events, c->timing.h2d_ms, true);
    return 0;
}
DevBuf take_pooled(rsqc_ctx *c, size_t bytes) {
    size_t best = (size_t)-1;
    for (size_t i = 0; i < c->upload_pool.size(); ++i)
        if (c->upload_pool[i].bytes >= bytes && (best == (size_t)-1 || c->upload_pool[i].bytes < c->upload_pool[best].bytes)) best = i;
    DevBuf b;
    if (best != (size_t)-1) { b = c->upload_pool[best]; c->upload_pool.erase(c->upload_pool.begin() + (long)best); }
    return b;
}
void free_batch(UploadedBatch *u) {
    for (auto &b : u->bufs) b.release();
    delete u;
}
void retire_batch(rsqc_ctx *c, UploadedBatch *u) {
    if (!u->pooled) { free_batch(u); return; }
    for (auto &b : u->bufs) {
        if (c->upload_pool.size() < 64) c->upload_pool.push_back(b); else b.release();
    }
    u->bufs.clear();
    delete u;
}
static int arena_reserve(rsqc_ctx *c, Arena &a, uint64_t extra) {
    if (a.used + extra <= a.cap) return 0;
    // doubling, from a floor of 16 M entries: a handful of growth steps for any input.  The old columns are not freed here
    // (hipFree synchronises the device, in the middle of the decode / kernel pipeline): they are parked until the next
    // point where the stream has been synchronised anyway.
    const uint64_t ncap = std::max<uint64_t>(std::max<uint64_t>(a.used + extra, 2 * a.cap), 1ull << 24);
    for (int k = 0; k < a.n_col; ++k) {
        DevBuf nb;
        HIP_TRY(c, hipMalloc(&nb.p, ncap * a.width[k] + 64));
        nb.bytes = ncap * a.width[k] + 64;
        if (a.used) HIP_TRY(c, hipMemcpyAsync(nb.p, a.col[k].p, a.used * a.width[k], hipMemcpyDeviceToDevice, c->stream));
        if (a.col[k].p) c->parked.push_back(a.col[k]);
        a.col[k] = nb;
    }
    a.cap = ncap;
    return 0;
}
int arena_append(rsqc_ctx *c, Arena &a, const void *const *src, uint32_t n, hipStream_t s) {
    if (int rc = arena_reserve(c, a, n)) return rc;
    for (int f = 0; f < a.n_col && n; ++f)
        HIP_TRY(c, hipMemcpyAsync((char *)a.col[f].p + a.used * a.width[f], src[f], (size_t)n * a.width[f], hipMemcpyDeviceToDevice, s));
    a.used += n;
    return 0;
}
void free_parked(rsqc_ctx *c) {                 // caller: the stream has been synchronised
    for (auto &b : c->parked) b.release();
    c->parked.clear();
}
// Retires every in-flight batch whose kernels have completed -- all of them when `all`, waiting for each batch's `done` event
// (the caller need NOT have synchronised: `done` is recorded on the side stream behind the copy of the batch's pair counts, which
// waits for `kernels`, recorded on the main stream behind the batch's last kernel AND behind the copies of its fragment-size / GC
// candidate counts -- so those mirrors are valid too once `done` has fired).
int retire_completed(rsqc_ctx *c, bool all) {
    size_t keep = 0;
    for (size_t k = 0; k < c->pairs_in_flight.size(); ++k) {
        const size_t idx = c->pairs_in_flight[k];
        PairBuf &pb = c->pair_pool[idx];
        // in submission order only: the arena keeps file order, which the fragment de-dup's LDS pass relies on for locality
        const bool done = keep == k && (all || hipEventQuery(pb.done) == hipSuccess);
        if (!done) { c->pairs_in_flight[keep++] = idx; continue; }
        if (all) HIP_TRY(c, hipEventSynchronize(pb.done));          // (the counts travel on a side stream)
        uint64_t total = 0;
        for (uint32_t j = 0; j < pb.n_chunks; ++j) total += std::min(pb.h_counts[j], pb.chunk_cap);
        total += std::min(pb.h_counts[pb.n_chunks], pb.slow_cap);
        if (c->pair_arena.used + total > 0xFFFFFFF0ull) return fail(c, RSQC_ERR_CAPACITY, "more than 2^32 (gene, name) pairs in one pass");
        int rc = arena_reserve(c, c->pair_arena, total);
        if (rc) return rc;
        if (total) launch_pairs_append(c->stream, (const PairRec *)pb.rec.p, pb.chunk_cap, (const uint32_t *)pb.counts.p,
                                       pb.n_chunks, pb.slow_base, pb.slow_cap, (PairRec *)c->pair_arena.col[0].p + c->pair_arena.used);
        c->pair_arena.used += total;
        pb.used = false;                       // (stream order: the append reads the buffer before a later batch writes it)
    }
    c->pairs_in_flight.resize(keep);
    // candidate lists are dense [0, count): plain device-to-device copies.  They are retired together with their batch's
    // pairs: a candidate buffer is in flight exactly as long as the pair buffer submitted with it.
    auto retire_list = [&](std::vector<size_t> &in_flight, size_t n_keep, Arena &arena, auto &&buf_of) -> int {
        const size_t n_retire = in_flight.size() > n_keep ? in_flight.size() - n_keep : 0;
        for (size_t k = 0; k < n_retire; ++k) {
            uint32_t count = 0; uint32_t cap = 0; const void *src[8]; bool *used = nullptr;
            buf_of(in_flight[k], count, cap, src, used);
            if (count > cap) return fail(c, RSQC_ERR_CAPACITY, "candidate overflow");
            if (int rc = arena_append(c, arena, src, count, c->stream)) return rc;
            *used = false;
        }
        in_flight.erase(in_flight.begin(), in_flight.begin() + (long)n_retire);
        return 0;
    };
    int rc = retire_list(c->frags_in_flight, c->have_bed ? keep : c->frags_in_flight.size(), c->frag_arena,
                         [&](size_t i, uint32_t &count, uint32_t &cap, const void **src, bool *&used) {
                             FragBuf &fb = c->frag_pool[i]; count = *fb.h_count; cap = fb.cap; used = &fb.used;
                             src[0] = fb.file.p; src[1] = fb.qhash.p; src[2] = fb.name.p; src[3] = fb.endpos.p; src[4] = fb.fs.p; src[5] = fb.h2.p;
                         });
    if (rc) return rc;
    return retire_list(c->gcs_in_flight, (c->have_ref && !c->dparams.legacy) ? keep : c->gcs_in_flight.size(), c->gc_arena,
                       [&](size_t i, uint32_t &count, uint32_t &cap, const void **src, bool *&used) {
                           GcBuf &gb = c->gc_pool[i]; count = *gb.h_count; cap = gb.cap; used = &gb.used;
                           src[0] = gb.file.p; src[1] = gb.qhash.p; src[2] = gb.row.p; src[3] = gb.endpos.p; src[4] = gb.flag_lq.p; src[5] = gb.tid.p; src[6] = gb.h2.p;
                       });
}
static int check_device_error(rsqc_ctx *c) {
    int err = 0;
    HIP_TRY(c, hipMemcpyAsync(&err, c->acc.error, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (err) {
        c->sticky = err;
        return fail(c, err, device_error_message(c, err));
    }
    return 0;
}
static int upload_batch(rsqc_ctx *c, const rsqc_batch *b, UploadedBatch *u, bool pooled = false) {
    u->pooled = pooled;
    if (b->n > 0xFFFFFFF0ull || b->n_cigar_total >= (1ull << 30)) return fail(c, RSQC_ERR_ARG, "batch too large");
    DevBatch &d = u->d;
    d.n = b->n; d.n_seg = b->n_seg; d.n_wide = b->n_wide;
    u->n = b->n; u->n_cigar_total = b->n_cigar_total; u->file_index_base = b->file_index_base;
    int rc;
#define UP(field, count) if ((rc = upload(c, u->bufs, b->field, (size_t)(count), &d.field, pooled))) return rc
    UP(core, b->n); UP(aux, b->n);
    UP(cigar, b->n_cigar_total);
    UP(seg_tid, b->n_seg); UP(seg_start, (size_t)b->n_seg + 1);
    UP(wide_index, b->n_wide); UP(wide_nm, b->n_wide); UP(wide_l_qseq, b->n_wide); UP(wide_n_cigar, b->n_wide);
    d.qhash2 = nullptr;
    if (b->qhash2) UP(qhash2, b->n);
    // rsqc_batch.umi: read only while the context marks duplicates by UMI (rsqc_markdup_use_umi); never dereferenced otherwise
    u->umi = nullptr;
    if (b->umi && c->markdup.use_umi && (rc = upload(c, u->bufs, b->umi, (size_t)b->n, &u->umi, pooled))) return rc;
    d.seg_file_index = nullptr;
    u->seg_file_index.clear(); u->seg_records.clear();
    if (b->seg_file_index && b->n_seg) {
        UP(seg_file_index, b->n_seg);
        u->seg_file_index.assign(b->seg_file_index, b->seg_file_index + b->n_seg);
        for (uint32_t k = 0; k < b->n_seg; ++k) u->seg_records.push_back(b->seg_start[k + 1] - b->seg_start[k]);
        for (uint32_t k = 0; k + 1 < b->n_seg; ++k)
            if (u->seg_file_index[k + 1] < u->seg_file_index[k] + u->seg_records[k]) return fail(c, RSQC_ERR_ARG, "rsqc_batch.seg_file_index: the ranges must ascend and not overlap");
        DevBuf rs = pooled ? take_pooled(c, (size_t)b->n_seg * 12 + 32) : DevBuf{};
        if (!rs.p) { HIP_TRY(c, hipMalloc(&rs.p, (size_t)b->n_seg * 12 + 32)); rs.bytes = (size_t)b->n_seg * 12 + 32; }
        u->bufs.push_back(rs); u->rl_seg = rs;           // (owned through bufs)
        u->file_index_base = u->seg_file_index[0];
    }
#undef UP
    return 0;
}
static PairBuf *acquire_pairs(rsqc_ctx *c, uint64_t cap, uint32_t n_counts, size_t *index) {
    for (size_t i = 0; i < c->pair_pool.size(); ++i)
        if (!c->pair_pool[i].used && c->pair_pool[i].cap >= cap && c->pair_pool[i].counts_cap >= n_counts) {
            c->pair_pool[i].used = true; *index = i; return &c->pair_pool[i];
        }
    PairBuf pb;
    if (hipMalloc(&pb.rec.p, (size_t)cap * sizeof(PairRec)) != hipSuccess) return nullptr;
    if (hipMalloc(&pb.counts.p, (size_t)n_counts * 4) != hipSuccess) return nullptr;
    pb.rec.bytes = (size_t)cap * sizeof(PairRec); pb.counts.bytes = (size_t)n_counts * 4;
    if (hipHostMalloc((void **)&pb.h_counts, (size_t)n_counts * 4, hipHostMallocDefault) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&pb.done, hipEventDisableTiming) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&pb.kernels, hipEventDisableTiming) != hipSuccess) return nullptr;
    pb.cap = cap; pb.counts_cap = n_counts; pb.used = true;
    c->pair_pool.push_back(pb);
    *index = c->pair_pool.size() - 1;
    return &c->pair_pool.back();
}
// fragment-size candidates of a batch of n records run by `grid` workgroups: an unused buffer of the pool or a new one, its counter armed
static int acquire_frags(rsqc_ctx *c, uint64_t n, int grid, FragBuf **out) {
    size_t fidx = c->frag_pool.size();
    for (size_t i = 0; i < c->frag_pool.size(); ++i) if (!c->frag_pool[i].used && c->frag_pool[i].cap >= n && (c->dparams.legacy || c->frag_pool[i].grid_cap >= (uint32_t)grid)) { fidx = i; break; }
    if (fidx == c->frag_pool.size()) {
        FragBuf fb; fb.cap = (uint32_t)n;
        int rc2;
        if ((rc2 = dev_alloc(c, fb.file, n * 8, false)) || (rc2 = dev_alloc(c, fb.qhash, n * 8, false)) ||
            (rc2 = dev_alloc(c, fb.name, n * 4, false)) || (rc2 = dev_alloc(c, fb.endpos, n * 4, false)) ||
            (rc2 = dev_alloc(c, fb.fs, n * 4, false)) || (rc2 = dev_alloc(c, fb.h2, n * 4, false)) || (rc2 = dev_alloc(c, fb.count, 16, false))) return rc2;
        if (!c->dparams.legacy) {
            fb.grid_cap = (uint32_t)grid;
            if ((rc2 = dev_alloc(c, fb.r_file, n * 8, false)) || (rc2 = dev_alloc(c, fb.r_qhash, n * 8, false)) ||
                (rc2 = dev_alloc(c, fb.r_name, n * 4, false)) || (rc2 = dev_alloc(c, fb.r_endpos, n * 4, false)) ||
                (rc2 = dev_alloc(c, fb.r_fs, n * 4, false)) || (rc2 = dev_alloc(c, fb.r_h2, n * 4, false)) || (rc2 = dev_alloc(c, fb.r_counts, (size_t)grid * 4, false))) return rc2;
        }
        HIP_TRY(c, hipHostMalloc((void **)&fb.h_count, 16, hipHostMallocDefault));
        c->frag_pool.push_back(fb);
    }
    FragBuf &fb = c->frag_pool[fidx];
    fb.used = true;
    c->frags_in_flight.push_back(fidx);
    HIP_TRY(c, hipMemsetAsync(fb.count.p, 0, 16, c->stream));
    *out = &fb;
    return 0;
}
// fragment GC candidates of a batch of n records, likewise
static int acquire_gc(rsqc_ctx *c, uint64_t n, GcBuf **out) {
    size_t gidx = c->gc_pool.size();
    for (size_t i = 0; i < c->gc_pool.size(); ++i) if (!c->gc_pool[i].used && c->gc_pool[i].cap >= n) { gidx = i; break; }
    if (gidx == c->gc_pool.size()) {
        GcBuf gb; gb.cap = (uint32_t)n;
        int rc2;
        if ((rc2 = dev_alloc(c, gb.file, n * 8, false)) || (rc2 = dev_alloc(c, gb.qhash, n * 8, false)) ||
            (rc2 = dev_alloc(c, gb.row, n * 4, false)) || (rc2 = dev_alloc(c, gb.endpos, n * 4, false)) ||
            (rc2 = dev_alloc(c, gb.flag_lq, n * 4, false)) || (rc2 = dev_alloc(c, gb.tid, n * 4, false)) || (rc2 = dev_alloc(c, gb.h2, n * 4, false)) ||
            (rc2 = dev_alloc(c, gb.count, 16, false))) return rc2;
        HIP_TRY(c, hipHostMalloc((void **)&gb.h_count, 16, hipHostMallocDefault));
        c->gc_pool.push_back(gb);
    }
    GcBuf &gb = c->gc_pool[gidx];
    gb.used = true;
    c->gcs_in_flight.push_back(gidx);
    HIP_TRY(c, hipMemsetAsync(gb.count.p, 0, 16, c->stream));
    *out = &gb;
    return 0;
}

int run_batch(rsqc_ctx *c, UploadedBatch *u) {
    // record indices ride in 32 bits inside the per-record kernel (31 in its overflow list): checked before anything is recorded for the batch
    if (u->n >= (1ull << 31)) return fail(c, RSQC_ERR_ARG, "batch too large (split it)");
    if (!c->have_ann) return fail(c, RSQC_ERR_ARG, "rsqc_set_annotation must precede rsqc_submit");
    if (c->finalized) return fail(c, RSQC_ERR_ARG, "rsqc_reset required after rsqc_finalize");
    if (u->n == 0) return 0;
    if (c->sort.active && c->markdup.use_umi && !u->umi)       // (refused for what it is: the collection stays as it was)
        return fail(c, RSQC_ERR_ARG, "rsqc_batch.umi must be given for every batch of a pass behind rsqc_markdup_use_umi");
    // one name identity per pass: a fragment whose mates carry (qhash, h2) and (qhash, 0) would count as two names
    {
        const int mode = u->d.qhash2 ? 1 : 0;
        if (c->name_mode < 0) c->name_mode = mode;
        else if (c->name_mode != mode)
            return fail(c, RSQC_ERR_ARG, "rsqc_batch.qhash2 must be given for every batch of a pass or for none (the name identity is 96 or 64 bits for the whole pass)");
    }
    if (c->sort.active) return sort_append(c, u);   // rsqc_sort_begin: collected now, run by rsqc_sort_end
    const uint64_t tiles = (u->n + RSQC_K1_THREADS - 1) / RSQC_K1_THREADS;
    const uint64_t wave_tiles = (u->n + 63) / 64 + 64;
    if (wave_tiles > c->tile_cap) {
        c->tile_cap = wave_tiles + wave_tiles / 4 + 64;
        int rc = dev_alloc(c, c->d_tiles, c->tile_cap * sizeof(uint32_t), false);
        if (rc) return rc;
        c->acc.tile_span = (uint32_t *)c->d_tiles.p;
    }
    // (gene, qname-hash) pairs of this batch: every K1 block owns a private chunk sized for the
    // worst case of its tiles (FAST_SET pairs per record); 1 M extra slots serve the slow path
    // Workgroups: the context's grid for a batch that fills it; a smaller batch gets one round of the chip (256 CUs x 5) or 2048
    // records per workgroup, whichever is more -- with a workgroup per 256 records (round 4) a 0.8 M-record batch ran three rounds of
    // workgroups that each initialised and flushed their LDS tables for ONE tile per wave (profiles/r5_kernel_stats_dist_selftest_before.txt)
    const int grid = (int)std::min<uint64_t>(tiles, std::min<uint64_t>((uint64_t)c->k1_grid, std::max<uint64_t>(1280, u->n / 2048)));
    const uint64_t total_waves = (uint64_t)grid * (RSQC_K1_THREADS / 64);
    const uint64_t per_wave = (((u->n + total_waves - 1) / total_waves) + 63ull) & ~63ull;   // as in the kernel
    if (!c->dparams.legacy) {                  // the deferred list: a slot per record (a workgroup's region is its record range) + the dense list (whole calls of 64 per workgroup)
        const size_t region_words = u->n + 64, list_words = u->n + 64 * (size_t)grid + 64;
        if (c->d_defer.bytes < (region_words + list_words) * 4) { int rc = dev_alloc(c, c->d_defer, (region_words + list_words + u->n / 2) * 4, false); if (rc) return rc; }
        c->acc.defer_index = (uint32_t *)c->d_defer.p; c->acc.defer_list = c->acc.defer_index + region_words;
    }
    const uint64_t chunk_cap = per_wave * (RSQC_K1_THREADS / 64) * FAST_SET;
    // --legacy: every pair comes from the general kernel (one per gene a record is counted to; 4 per record is far
    // above what annotations produce -- beyond it the run fails with RSQC_ERR_CAPACITY)
    const uint64_t slow_cap = c->dparams.legacy ? std::max<uint64_t>(1ull << 20, 4ull * u->n) + (uint64_t)RSQC_SLOW_LEGACY_GRID * RSQC_SLOW_RES : 1ull << 20;
    // chunks: one per K1 workgroup, then one per workgroup of classify_long_kernel (the records K1 defers; none under --legacy)
    const int n_chunks = grid + (c->dparams.legacy ? 0 : rsqc_long_grid(grid));
    const uint64_t want = chunk_cap * (uint64_t)n_chunks + slow_cap;
    if (want > 0xFFFFFFF0ull) return fail(c, RSQC_ERR_ARG, "batch too large (split it)");
    { int rcr = retire_completed(c, false); if (rcr) return rcr; }     // completed batches hand their buffers back first
    size_t pidx = 0;
    PairBuf *pb = acquire_pairs(c, want, (uint32_t)n_chunks + 1, &pidx);
    if (!pb) return fail(c, RSQC_ERR_HIP, "hipMalloc(pair buffer) failed");
    pb->n_chunks = (uint32_t)n_chunks; pb->chunk_cap = (uint32_t)chunk_cap;
    pb->pairs_bound = std::min<uint64_t>(want, u->n * (uint64_t)FAST_SET + slow_cap);
    pb->slow_base = (uint32_t)(chunk_cap * (uint64_t)n_chunks); pb->slow_cap = (uint32_t)slow_cap;
    c->pairs_in_flight.push_back(pidx);
    // (no per-batch memsets: every K1 workgroup writes its own chunk count, workgroup 0 zeroes the slow-path pair
    //  counter, and the overflow counter is re-armed by the last kernel of the previous batch / the reset kernel)
    DevAccum acc = c->acc;
    acc.pairs = (PairRec *)pb->rec.p;
    acc.pair_chunk_cap = pb->chunk_cap; acc.pair_chunk_count = (uint32_t *)pb->counts.p;
    acc.pair_slow_base = pb->slow_base; acc.pair_slow_cap = pb->slow_cap;
    acc.pair_slow_count = (uint32_t *)pb->counts.p + n_chunks;
    FragCandidates frag_dense{};
    if (c->have_bed) {
        FragBuf *fbp = nullptr; if (int rc2 = acquire_frags(c, u->n, grid, &fbp)) return rc2;
        FragBuf &fb = *fbp;
        acc.frag.file_index = (uint64_t *)fb.file.p; acc.frag.qhash = (uint64_t *)fb.qhash.p;
        acc.frag.name = (int32_t *)fb.name.p; acc.frag.endpos = (int32_t *)fb.endpos.p;
        acc.frag.flag_size = (uint32_t *)fb.fs.p; acc.frag.count = (uint32_t *)fb.count.p; acc.frag.cap = fb.cap; acc.frag.chunk_count = nullptr;
        acc.frag.h2 = (uint32_t *)fb.h2.p;
        frag_dense = acc.frag;
        if (!c->dparams.legacy) {                 // the per-record kernel writes workgroup regions; frag_compact_kernel packs them (below)
            acc.frag.file_index = (uint64_t *)fb.r_file.p; acc.frag.qhash = (uint64_t *)fb.r_qhash.p; acc.frag.name = (int32_t *)fb.r_name.p;
            acc.frag.endpos = (int32_t *)fb.r_endpos.p; acc.frag.flag_size = (uint32_t *)fb.r_fs.p; acc.frag.chunk_count = (uint32_t *)fb.r_counts.p;
            acc.frag.h2 = (uint32_t *)fb.r_h2.p;
        }
    }
    // file order is part of the boundary: the index of record 0 in the whole file comes from the caller (it decides the
    // first-N cut-off of the fragment-size sampler and the order in which shards are composed); batches arrive in file order
    if (u->file_index_base < c->next_record_base)
        return fail(c, RSQC_ERR_ARG, "batches must be submitted in file order (file_index_base below the end of the previous batch)");
    constexpr size_t kMaxBatches = 1u << 14;
    const bool ranges = !u->seg_file_index.empty();
    if (ranges && c->dparams.legacy) return fail(c, RSQC_ERR_ARG, "rsqc_batch.seg_file_index is not supported with --legacy");
    const size_t n_entries = ranges ? u->seg_file_index.size() : 1;          // order-dependent summaries: one per batch, or one per range
    if (c->batch_file_index.size() + n_entries > kMaxBatches) return fail(c, RSQC_ERR_CAPACITY, "more than 16384 batches / file ranges in one pass");
    if (!c->d_rl_summary.p) { int rc3 = dev_alloc(c, c->d_rl_summary, kMaxBatches * RSQC_RL_SUMMARY_WORDS * 4, true); if (rc3) return rc3; }
    uint32_t *rl_slot = (uint32_t *)c->d_rl_summary.p + c->batch_file_index.size() * RSQC_RL_SUMMARY_WORDS;
    DevBatch d = u->d;
    d.record_base = u->file_index_base;
    acc.rl_seg = nullptr;
    if (ranges) {
        // the per-segment Read-Length inputs, armed {max span 0, min l_qseq UINT_MAX, max l_qseq 0}
        c->h_rl_arm.resize(3 * n_entries);
        for (size_t k = 0; k < n_entries; ++k) { c->h_rl_arm[3 * k] = 0u; c->h_rl_arm[3 * k + 1] = 0xFFFFFFFFu; c->h_rl_arm[3 * k + 2] = 0u; }
        HIP_TRY(c, hipMemcpyAsync(u->rl_seg.p, c->h_rl_arm.data(), n_entries * 12, hipMemcpyHostToDevice, c->stream));
        acc.rl_seg = (uint32_t *)u->rl_seg.p;
    }
    hipEvent_t e0 = get_event(c), e1 = get_event(c);
    HIP_TRY(c, hipEventRecord(e0, c->stream));
    launch_classify(c->stream, grid, c->dparams.legacy ? -1 : c->k1_variant, c->dann, c->dparams, d, acc);
    HIP_TRY(c, hipEventRecord(e1, c->stream));
    c->k1_events.emplace_back(e0, e1);
    if (!c->dparams.legacy) {                       // the records it deferred: timed on its own (rsqc_timing.classify_long_ms)
        hipEvent_t e2 = get_event(c);
        launch_classify_long(c->stream, grid, c->dann, c->dparams, d, acc);
        HIP_TRY(c, hipEventRecord(e2, c->stream));
        c->long_events.emplace_back(e1, e2);
    }
    if (c->have_bed && !c->dparams.legacy) launch_frag_compact(c->stream, acc.frag, frag_dense, u->n, grid);
    launch_classify_slow(c->stream, c->dann, c->dparams, d, acc);
    launch_read_length(c->stream, c->dann, c->dparams, d, acc, rl_slot);
    // the batch's entries are listed only now that the kernel which writes their summary slots is enqueued: a submit that fails
    // above leaves no entry whose slot -- its flag word is read by device_error_message -- was never written in this pass
    if (ranges) {
        for (size_t k = 0; k < n_entries; ++k) { c->batch_file_index.push_back(u->seg_file_index[k]); c->batch_records.push_back(u->seg_records[k]); }
        c->next_record_base = u->seg_file_index.back() + u->seg_records.back();
        c->have_ranges = true;
    } else {
        c->batch_file_index.push_back(u->file_index_base); c->batch_records.push_back(u->n);
        c->next_record_base = u->file_index_base + u->n;
    }
    if (c->have_ref && !c->dparams.legacy) {          // --fasta: fragment GC candidates, a separate pass over the batch
        GcBuf *gbp = nullptr; if (int rc2 = acquire_gc(c, u->n, &gbp)) return rc2;
        GcBuf &gb = *gbp;
        GcCandidates gc{(uint64_t *)gb.file.p, (uint64_t *)gb.qhash.p, (uint32_t *)gb.row.p, (int32_t *)gb.endpos.p,
                        (uint32_t *)gb.flag_lq.p, (int32_t *)gb.tid.p, (uint32_t *)gb.count.p, gb.cap, (uint32_t *)gb.h2.p};
        launch_gc_candidates(c->stream, c->dann, c->dparams, d, c->dref, gc, acc.error);
    }
    // --junctions: the batch's splice-junction instances, in front of the event that retires the batch (its buffers are read)
    if (c->junc.active) { if (int rc2 = junction_extract(c, u, d)) return rc2; }
    // --bedgraph: the batch's coverage events, likewise
    if (c->track.active) { if (int rc2 = track_events(c, u, d)) return rc2; }
    // the batch's counts, for its retirement: page-locked mirrors + an event that tells when they are valid.  The copy of the
    // pair counts rides on a side stream: a copy between two kernels of the main stream costs ~40 us of queue hand-over there
    // (profiles/r4_step_timeline.txt), and nothing on the main stream reads what it brings
    if (c->have_bed) { FragBuf &fb = c->frag_pool[c->frags_in_flight.back()]; HIP_TRY(c, hipMemcpyAsync(fb.h_count, fb.count.p, 4, hipMemcpyDeviceToHost, c->stream)); }
    if (c->have_ref && !c->dparams.legacy) { GcBuf &gb = c->gc_pool[c->gcs_in_flight.back()]; HIP_TRY(c, hipMemcpyAsync(gb.h_count, gb.count.p, 4, hipMemcpyDeviceToHost, c->stream)); }
    HIP_TRY(c, hipEventRecord(pb->kernels, c->stream));
    HIP_TRY(c, hipStreamWaitEvent(c->stream2, pb->kernels, 0));
    HIP_TRY(c, hipMemcpyAsync(pb->h_counts, pb->counts.p, ((size_t)n_chunks + 1) * 4, hipMemcpyDeviceToHost, c->stream2));
    HIP_TRY(c, hipEventRecord(pb->done, c->stream2));
    HIP_TRY(c, hipGetLastError());
    c->timing.classify_launches += 1;
    c->timing.classify_records += u->n;
    c->timing.classify_bytes += 32ull * u->n + 4ull * u->n_cigar_total;
    return 0;
}

}  // namespace rsqc

int rsqc_submit(rsqc_ctx *c, const rsqc_batch *b) {
    if (!c || !b) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    HIP_TRY(c, hipSetDevice(c->device));
    UploadedBatch *u = new UploadedBatch();
    hipEvent_t e0 = get_event(c), e1 = get_event(c);
    (void)hipEventRecord(e0, c->stream);
    int rc = upload_batch(c, b, u, /*pooled=*/true);
    (void)hipEventRecord(e1, c->stream);
    c->h2d_events.emplace_back(e0, e1);           // resolved at rsqc_wait / rsqc_finalize
    if (rc) { free_batch(u); return rc; }
    c->transient.push_back(u);
    // asynchronous from here on: with pinned source arrays (rsqc_host_alloc) the copies are DMA transfers the
    // call does not wait for; the caller keeps the arrays alive and unmodified until rsqc_wait
    return run_batch(c, u);
}

int rsqc_wait(rsqc_ctx *c) {
    if (!c) return RSQC_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    resolve_events(c);
    for (auto *u : c->transient) retire_batch(c, u);
    c->transient.clear();
    free_parked(c);
    if (c->have_ann) {
        int rc = retire_completed(c, true);      // everything submitted so far has completed
        if (rc) return rc;
        return check_device_error(c);
    }
    return RSQC_OK;
}

int rsqc_upload(rsqc_ctx *c, const rsqc_batch *b, int *handle_out) {
    if (!c || !b || !handle_out) return RSQC_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    UploadedBatch *u = new UploadedBatch();
    int rc = upload_batch(c, b, u);
    if (rc) { free_batch(u); return rc; }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->resident.push_back(u);
    *handle_out = (int)c->resident.size() - 1;
    return RSQC_OK;
}

int rsqc_submit_resident(rsqc_ctx *c, int handle) {
    if (!c || handle < 0 || handle >= (int)c->resident.size() || !c->resident[(size_t)handle]) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    HIP_TRY(c, hipSetDevice(c->device));
    RSQC_TRACE("submit_resident: enter");
    const int rc = run_batch(c, c->resident[(size_t)handle]);
    RSQC_TRACE("submit_resident: enqueued");
    return rc;
}

int rsqc_release(rsqc_ctx *c, int handle) {
    if (!c || handle < 0 || handle >= (int)c->resident.size() || !c->resident[(size_t)handle]) return RSQC_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    free_batch(c->resident[(size_t)handle]);
    c->resident[(size_t)handle] = nullptr;
    return RSQC_OK;
}
