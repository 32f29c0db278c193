// rsqc_track_api.cpp -- rsqc_track_begin / rsqc_track_end / rsqc_track_rows / rsqc_track_text: every batch that run_batch runs adds
// its coverage events to a device-resident difference array (one extra kernel per batch, rsqc_track.hip); at the end of the pass ONE
// prefix sum (the scan of --sort, rsqc_sort.hip) turns it into depths, two kernels over chunks of it into rows, and the rows are
// formatted as bedGraph text on the device, a window at a time.
#include "rsqc_ctx.h"
#include "rsqc_sort.h"
#include "rsqc_track.h"

namespace {

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

int alloc_or_capacity(rsqc_ctx *c, DevBuf &b, size_t bytes, const char *who, const char *what) {
    if (dev_reserve(b, bytes)) return 0;
    return fail(c, RSQC_ERR_CAPACITY, std::string(who) + ": no device memory for " + what + " (" + std::to_string(bytes) + " bytes)");
}

TrackRows rows_of(const TrackState &T) {
    const uint64_t n = T.info.n_rows;
    TrackRows R{};
    R.tid = (int32_t *)T.rows.p; R.start = (uint32_t *)(R.tid + n); R.end = R.start + n; R.depth = R.end + n;
    return R;
}

int track_end_run(rsqc_ctx *c) {
    TrackState &T = c->track;
    rsqc_track_info &I = T.info;
    unsigned long long sums[3] = {0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(sums, T.sums.p, 24, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    for (auto &pr : T.events) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) I.events_ms += ms;
        c->event_pool.push_back(pr.first); c->event_pool.push_back(pr.second);
    }
    T.events.clear();
    I.population = sums[0]; I.aligned_bases = sums[1]; I.clipped_bases = sums[2];
    I.n_rows = 0;
    if (!T.total) return 0;
    int rc;
    const uint64_t m = T.total + 1;                    // (the exclusive scan's extra slot: the depth of slot i is read at i + 1)
    const uint64_t scan_chunks = (m + RSQC_SCAN_CHUNK - 1) / RSQC_SCAN_CHUNK + 1, row_chunks = (T.total + RSQC_TRACK_CHUNK - 1) / RSQC_TRACK_CHUNK;
    if ((rc = alloc_or_capacity(c, T.chunk_sum, scan_chunks * 8, "rsqc_track_end", "the scan's chunk sums")) ||
        (rc = alloc_or_capacity(c, T.totals, 64, "rsqc_track_end", "the scan totals")) ||
        (rc = alloc_or_capacity(c, T.counts, row_chunks * 4 + 64, "rsqc_track_end", "the heads per chunk"))) return rc;
    unsigned long long *d_tot = (unsigned long long *)T.totals.p;
    // ---- (1) the depths
    auto t0 = std::chrono::steady_clock::now();
    launch_sort_scan(c->stream, (uint32_t *)T.diff.p, m, (unsigned long long *)T.chunk_sum.p, d_tot);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    I.scan_ms = ms_since(t0);
    // ---- (2) the rows: heads per chunk, their prefix sum, the row count read back, the columns at exactly that size
    t0 = std::chrono::steady_clock::now();
    launch_track_count(c->stream, (const uint32_t *)T.diff.p, T.total, (uint32_t *)T.counts.p);
    launch_sort_scan(c->stream, (uint32_t *)T.counts.p, row_chunks, (unsigned long long *)T.chunk_sum.p, d_tot);
    unsigned long long rows = 0;
    HIP_TRY(c, hipMemcpyAsync(&rows, d_tot, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (rows >= RSQC_TRACK_MAX_ROWS)
        return fail(c, RSQC_ERR_CAPACITY, "rsqc_track_end: " + std::to_string(rows) + " rows over " + std::to_string(I.positions) + " positions (the limit of a pass is 2^32 - 16)");
    if (rows) {
        if ((rc = alloc_or_capacity(c, T.rows, (size_t)rows * 16 + 64, "rsqc_track_end", ("the " + std::to_string(rows) + " rows of the track").c_str()))) return rc;
        I.n_rows = rows;
        launch_track_rows(c->stream, (const uint32_t *)T.diff.p, T.total, (const uint32_t *)T.counts.p, (const uint64_t *)T.off.p, T.n, rows, rows_of(T));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
    }
    I.rows_ms = ms_since(t0);
    return 0;
}

int window_check(rsqc_ctx *c, const char *who, uint64_t first, uint64_t n) {
    if (c->sticky) return c->sticky;
    if (!c->track.active || !c->track.done) return fail(c, RSQC_ERR_ARG, std::string("rsqc_track_end must precede ") + who);
    if (first > c->track.info.n_rows || n > c->track.info.n_rows - first)
        return fail(c, RSQC_ERR_ARG, std::string(who) + ": rows [" + std::to_string(first) + ", + " + std::to_string(n) + ") of " + std::to_string(c->track.info.n_rows));
    return 0;
}

}  // namespace

namespace rsqc {

void track_drop(rsqc_ctx *c, bool free_buffers) {
    TrackState &T = c->track;
    for (auto &pr : T.events) { c->event_pool.push_back(pr.first); c->event_pool.push_back(pr.second); }
    T.events.clear();
    T.active = T.done = T.have_names = false;
    T.n = 0; T.total = 0;
    T.info = rsqc_track_info{};
    T.h_tid.clear(); T.h_start.clear(); T.h_end.clear(); T.h_depth.clear();
    if (free_buffers) {
        for (DevBuf *b : {&T.diff, &T.off, &T.length, &T.sums, &T.names, &T.name_off, &T.counts, &T.chunk_sum, &T.totals, &T.rows, &T.linelen, &T.text}) b->release();
        T.h_text.release();
    }
}

// called by run_batch for every batch it runs, on the main stream in front of the event that retires the batch
int track_events(rsqc_ctx *c, const UploadedBatch *u, const DevBatch &d) {
    TrackState &T = c->track;
    TrackBatch B{};
    B.core = d.core; B.aux = d.aux; B.cigar = d.cigar; B.n = d.n; B.n_ops = u->n_cigar_total;
    B.seg_tid = d.seg_tid; B.seg_start = d.seg_start; B.n_seg = d.n_seg;
    B.wide_index = d.wide_index; B.wide_n_cigar = d.wide_n_cigar; B.n_wide = d.n_wide;
    TrackArray A{(uint32_t *)T.diff.p, (const uint64_t *)T.off.p, (const uint32_t *)T.length.p, T.n, (unsigned long long *)T.sums.p};
    hipEvent_t e0 = get_event(c), e1 = get_event(c);
    T.events.emplace_back(e0, e1);
    HIP_TRY(c, hipEventRecord(e0, c->stream));
    launch_track_events(c->stream, B, A, T.merge_later);
    HIP_TRY(c, hipEventRecord(e1, c->stream));
    return 0;
}

}  // namespace rsqc

int rsqc_track_begin(rsqc_ctx *c, int32_t n, const uint64_t *length, const char *const *name) {
    if (!c) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (n < 0 || (n && !length)) return fail(c, RSQC_ERR_ARG, "rsqc_track_begin: n contigs with their lengths");
    if (!c->have_ann) return fail(c, RSQC_ERR_ARG, "rsqc_set_annotation must precede rsqc_track_begin");
    if (c->finalized) return fail(c, RSQC_ERR_ARG, "rsqc_reset required after rsqc_finalize");
    if (c->track.active) return fail(c, RSQC_ERR_ARG, "rsqc_track_begin: the context is building a track already");
    if (c->name_mode >= 0 || !c->batch_file_index.empty() || c->next_record_base)
        return fail(c, RSQC_ERR_ARG, "rsqc_track_begin must precede the first submit of the pass");
    std::vector<uint64_t> off((size_t)n + 1, 0);
    std::vector<uint32_t> len32((size_t)n, 0), name_off((size_t)n + 1, 0);
    std::string names;
    uint64_t positions = 0;
    for (int32_t t = 0; t < n; ++t) {
        if (length[t] > 0x7FFFFFFFull) return fail(c, RSQC_ERR_ARG, "rsqc_track_begin: contig " + std::to_string(t) + " has " + std::to_string(length[t]) + " positions (at most 2^31 - 1)");
        if (name) {
            if (!name[t]) return fail(c, RSQC_ERR_ARG, "rsqc_track_begin: contig " + std::to_string(t) + " has no name");
            const size_t l = strlen(name[t]);
            if (l > RSQC_TRACK_NAME_MAX) return fail(c, RSQC_ERR_ARG, "rsqc_track_begin: the name of contig " + std::to_string(t) + " has " + std::to_string(l) + " bytes (at most 255)");
            names.append(name[t], l);
        }
        name_off[(size_t)t + 1] = (uint32_t)names.size();
        len32[(size_t)t] = (uint32_t)length[t];
        off[(size_t)t + 1] = off[(size_t)t] + length[t] + 1;
        positions += length[t];
    }
    const uint64_t total = off[(size_t)n];
    const uint64_t bytes = (total + 1) * 4 + 64;
    if (const char *e = getenv("RSQC_TRACK_MAX_BYTES")) {
        const unsigned long long bound = strtoull(e, nullptr, 10);
        if (bytes > bound)
            return fail(c, RSQC_ERR_CAPACITY, "rsqc_track_begin: the difference array of " + std::to_string(positions) + " positions takes " + std::to_string(bytes) + " bytes, RSQC_TRACK_MAX_BYTES allows " + std::to_string(bound));
    }
    HIP_TRY(c, hipSetDevice(c->device));
    track_drop(c, false);
    TrackState &T = c->track;
    int rc;
    if ((rc = alloc_or_capacity(c, T.diff, bytes, "rsqc_track_begin", ("the difference array of " + std::to_string(positions) + " positions").c_str())) ||
        (rc = alloc_or_capacity(c, T.off, ((size_t)n + 1) * 8, "rsqc_track_begin", "the contig offsets")) ||
        (rc = alloc_or_capacity(c, T.length, (size_t)n * 4 + 4, "rsqc_track_begin", "the contig lengths")) ||
        (rc = alloc_or_capacity(c, T.name_off, ((size_t)n + 1) * 4, "rsqc_track_begin", "the name offsets")) ||
        (rc = alloc_or_capacity(c, T.names, names.size() + 4, "rsqc_track_begin", "the contig names")) ||
        (rc = alloc_or_capacity(c, T.sums, 64, "rsqc_track_begin", "the sums"))) return rc;
    // (pageable sources: the copies have left these vectors when the calls return)
    HIP_TRY(c, hipMemsetAsync(T.diff.p, 0, (size_t)(total + 1) * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(T.sums.p, 0, 64, c->stream));
    HIP_TRY(c, hipMemcpyAsync(T.off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, c->stream));
    if (n) HIP_TRY(c, hipMemcpyAsync(T.length.p, len32.data(), len32.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(T.name_off.p, name_off.data(), name_off.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (!names.empty()) HIP_TRY(c, hipMemcpyAsync(T.names.p, names.data(), names.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    T.n = n; T.total = total; T.have_names = name != nullptr;
    T.info.positions = positions;
    const char *m = getenv("RSQC_TRACK_MERGE");        // 0: later events lane by lane; 1: merged like the first (the table is the same)
    T.merge_later = m ? atoi(m) != 0 : RSQC_TRACK_MERGE_LATER_DEFAULT;
    T.active = true;
    return RSQC_OK;
}

int rsqc_track_end(rsqc_ctx *c, rsqc_track_info *out) {
    if (!c || !out) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (!c->track.active) return fail(c, RSQC_ERR_ARG, "rsqc_track_begin must precede rsqc_track_end");
    if (!c->finalized) return fail(c, RSQC_ERR_ARG, "rsqc_finalize (or rsqc_finalize_device) must precede rsqc_track_end");
    if (!c->track.done) {
        HIP_TRY(c, hipSetDevice(c->device));
        const int rc = track_end_run(c);
        if (rc) { (void)hipStreamSynchronize(c->stream); c->sticky = rc; return rc; }      // never a partial table: the pass is void until rsqc_reset
        c->track.done = true;
    }
    *out = c->track.info;
    return RSQC_OK;
}

int rsqc_track_rows(rsqc_ctx *c, uint64_t first, uint64_t n, const int32_t **tid, const uint32_t **start, const uint32_t **end, const uint32_t **depth) {
    if (!c || !tid || !start || !end || !depth) return RSQC_ERR_ARG;
    if (int rc = window_check(c, "rsqc_track_rows", first, n)) return rc;
    TrackState &T = c->track;
    T.h_tid.resize(n); T.h_start.resize(n); T.h_end.resize(n); T.h_depth.resize(n);
    if (n) {
        HIP_TRY(c, hipSetDevice(c->device));
        const TrackRows R = rows_of(T);
        HIP_TRY(c, hipMemcpyAsync(T.h_tid.data(), R.tid + first, n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(T.h_start.data(), R.start + first, n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(T.h_end.data(), R.end + first, n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(T.h_depth.data(), R.depth + first, n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    *tid = T.h_tid.data(); *start = T.h_start.data(); *end = T.h_end.data(); *depth = T.h_depth.data();
    return RSQC_OK;
}

int rsqc_track_text(rsqc_ctx *c, uint64_t first, uint64_t n, const char **text, uint64_t *bytes) {
    if (!c || !text || !bytes) return RSQC_ERR_ARG;
    if (int rc = window_check(c, "rsqc_track_text", first, n)) return rc;
    TrackState &T = c->track;
    if (!T.have_names) return fail(c, RSQC_ERR_ARG, "rsqc_track_text: rsqc_track_begin was given no contig names");
    if (n > RSQC_TRACK_WINDOW) return fail(c, RSQC_ERR_ARG, "rsqc_track_text: " + std::to_string(n) + " rows in one call (at most 4194304)");
    *text = T.h_text.p ? (const char *)T.h_text.p : ""; *bytes = 0;
    if (!n) return RSQC_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = alloc_or_capacity(c, T.linelen, (size_t)n * 4 + 64, "rsqc_track_text", "the line lengths")) ||
        (rc = alloc_or_capacity(c, T.chunk_sum, ((size_t)n / RSQC_SCAN_CHUNK + 2) * 8, "rsqc_track_text", "the scan's chunk sums")) ||
        (rc = alloc_or_capacity(c, T.totals, 64, "rsqc_track_text", "the scan totals"))) return rc;
    const TrackRows R = rows_of(T);
    launch_track_linelen(c->stream, R, first, (uint32_t)n, (const uint32_t *)T.name_off.p, (uint32_t *)T.linelen.p);
    launch_sort_scan(c->stream, (uint32_t *)T.linelen.p, n, (unsigned long long *)T.chunk_sum.p, (unsigned long long *)T.totals.p);
    unsigned long long total = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, T.totals.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if ((rc = alloc_or_capacity(c, T.text, (size_t)total + 64, "rsqc_track_text", "the text of a window"))) return rc;
    if (T.h_text.bytes < total) {
        const size_t cap = std::max<size_t>((size_t)total + (size_t)total / 4, 1u << 20);
        if (!host_reserve(T.h_text, cap)) return fail(c, RSQC_ERR_CAPACITY, "rsqc_track_text: no page-locked memory for a window of " + std::to_string(cap) + " bytes");
    }
    launch_track_format(c->stream, R, first, (uint32_t)n, (const uint32_t *)T.name_off.p, (const char *)T.names.p, (const uint32_t *)T.linelen.p, (char *)T.text.p);
    HIP_TRY(c, hipMemcpyAsync(T.h_text.p, T.text.p, (size_t)total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    *text = (const char *)T.h_text.p; *bytes = total;
    return RSQC_OK;
}
