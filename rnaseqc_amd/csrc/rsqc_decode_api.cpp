// rsqc_decode_api.cpp -- rsqc_decode_*: file bytes in, windows of records parsed on the device (BAM: rsqc_decode.hip, SAM: rsqc_sam.hip) and run as batches.
#include "rsqc_ctx.h"

namespace {

// every buffer a window of the window buffer (W bytes, for `cap` inflated bytes) is parsed into: capacities from dec_caps / sam_caps
int reserve_columns(rsqc_ctx *c, size_t W, size_t cap) {
    DecodeState &D = c->dec;
    const DecCaps bam = dec_caps(W);
    const SamCaps sam = sam_caps(W);
    const size_t n_seg = bam.seg, n_rec = D.sam ? sam.rec_alloc : bam.rec;
    int rc;
    if ((rc = dev_alloc(c, D.seg, n_seg * sizeof(BamSegment), false)) || (rc = dev_alloc(c, D.seg_rec0, n_seg * 4, false)) ||
        (rc = dev_alloc(c, D.seg_ops0, n_seg * 4, false)) || (rc = dev_alloc(c, D.rec_off, n_rec * 4, false)) ||
        (rc = dev_alloc(c, D.ops_at, n_rec * 4, false)) || (rc = dev_alloc(c, D.mark, n_rec, false)) ||
        (rc = dev_alloc(c, D.core, n_rec * 16 + 64, false)) || (rc = dev_alloc(c, D.aux, n_rec * 16 + 64, false)) || (rc = dev_alloc(c, D.qh2, n_rec * 4 + 64, false)) ||
        (rc = dev_alloc(c, D.cigar, D.sam ? std::max<size_t>(bam.cigar_bytes, (size_t)sam.cigar_alloc * 4) : bam.cigar_bytes, false)) ||
        (rc = dev_alloc(c, D.seg_tid, n_rec * 4 + 64, false)) ||
        (rc = dev_alloc(c, D.seg_start, (n_rec + 1) * 8 + 64, false)) || (rc = dev_alloc(c, D.wide_index, n_rec * 8 + 64, false)) ||
        (rc = dev_alloc(c, D.wide_nm, n_rec * 4 + 64, false)) || (rc = dev_alloc(c, D.wide_lq, n_rec * 4 + 64, false)) ||
        (rc = dev_alloc(c, D.wide_nc, n_rec * 4 + 64, false))) return rc;
    D.out_cap = cap;
    if (!D.sam) return 0;
    const size_t n_words = W / 64 + 8, n_sseg = n_words / SAM_SEG_WORDS + 2;
    if ((rc = dev_alloc(c, D.sam_ebits, n_words * 8, false)) || (rc = dev_alloc(c, D.sam_tbits, n_words * 8, false)) ||
        (rc = dev_alloc(c, D.sam_segcnt, n_sseg * 4, false)) || (rc = dev_alloc(c, D.sam_segk0, n_sseg * 4, false)) ||
        (rc = dev_alloc(c, D.sam_rtid, n_rec * 4 + 64, false)) || (rc = dev_alloc(c, D.sam_nops, n_rec * 4 + 64, false)) ||
        (rc = dev_alloc(c, D.sam_scratch, sam_scratch_words((uint32_t)n_rec, (uint32_t)n_sseg) * 4, false))) return rc;
    D.sam_cap = cap; D.sam_rec_cap = sam.rec_alloc;
    return 0;
}
// buffers for a window of `out_bytes` inflated bytes behind the head room
int decode_reserve(rsqc_ctx *c, size_t out_bytes, size_t comp_bytes, size_t n_blocks) {
    DecodeState &D = c->dec;
    int rc;
    if (comp_bytes + 64 > D.comp_cap) {                        // (two halves: the call in flight and the one being copied)
        D.comp_cap = (comp_bytes + comp_bytes / 4 + 64 + 255) & ~(size_t)255;
        if ((rc = dev_alloc(c, D.comp, 2 * D.comp_cap, false))) return rc;
    }
    if (n_blocks > D.blk_cap) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        D.blk_cap = n_blocks + n_blocks / 4 + 64;
        if ((rc = dev_alloc(c, D.blocks, 2 * D.blk_cap * sizeof(DevBgzfBlock), false))) return rc;
        if (D.h_blocks) (void)hipHostFree(D.h_blocks);
        HIP_TRY(c, hipHostMalloc((void **)&D.h_blocks, 2 * D.blk_cap * sizeof(DevBgzfBlock), hipHostMallocDefault));
    }
    if (out_bytes <= D.out_cap && (!D.sam || D.sam_cap == D.out_cap)) return 0;
    const size_t cap = std::max<size_t>(std::max<size_t>(out_bytes + out_bytes / 8, 64u << 20), D.out_cap);
    const size_t W = (size_t)D.head + cap;
    // the window buffer keeps the carried-over bytes
    DevBuf nu;
    HIP_TRY(c, hipMalloc(&nu.p, W + 256)); nu.bytes = W + 256;
    if (D.tail) HIP_TRY(c, hipMemcpyAsync((char *)nu.p + D.head - D.tail, (char *)D.ubuf.p + D.head - D.tail, D.tail, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    D.ubuf.release(); D.ubuf = nu;
    return reserve_columns(c, W, cap);
}
// the UMI column of a window, only for a stream with a UMI source: as many entries as the qh2 column has (twice its bytes)
int reserve_umi(rsqc_ctx *c) {
    DecodeState &D = c->dec;
    return D.tags.umi_src ? dev_alloc(c, D.umi, D.qh2.bytes * 2, false) : 0;
}
// a SAM window the device stages refused: the first malformed line, found again on the host with the same functions, and its
// line number in the stream (rare path: the window's text is copied back)
void sam_window_error(rsqc_ctx *c, const DecodeWindow &W, std::string &msg) {
    DecodeState &D = c->dec;
    std::vector<uint8_t> t((size_t)(W.end - W.start) + 1, 0);
    if (W.end > W.start && hipMemcpy(t.data(), (const char *)D.ubuf.p + W.start, W.end - W.start, hipMemcpyDeviceToHost) != hipSuccess)
        { msg = "malformed SAM line (the window could not be read back)"; return; }
    uint64_t line = 0; uint32_t code = 0;
    if (sam_find_bad_line(t.data(), W.end - W.start, D.records > 0, D.tags, D.sam_line0, line, code)) {
        msg = "malformed SAM line " + std::to_string(line) + ": " + sam_error_text(code);
        return;
    }
    msg = "malformed SAM line (window from line " + std::to_string(D.sam_line0) + ")";
}
// the name of the record whose first `room` bytes are at raw, per format (a SAM line: the name is its first field)
std::string sam_record_name(const char *raw, size_t room) { return std::string(raw, std::find(raw, raw + room, '\t')); }
std::string bam_record_name(const char *raw, size_t room) {
    return std::string(raw + 36, strnlen(raw + 36, std::min<size_t>((uint8_t)raw[12], room > 36 ? room - 36 : 0)));
}
// the columns of the batch a parsed window holds: the same names in rsqc_batch (rsqc_decode_window::device_batch) and DevBatch
template <class Batch> void window_columns(Batch &b, const DecodeWindow &W, const DecodeSummary &S) {
    b.n = S.n_rec; b.core = W.core; b.aux = W.aux; b.qhash2 = W.qh2; b.cigar = W.cigar;
    b.n_seg = S.n_seg; b.seg_tid = W.seg_tid; b.seg_start = W.seg_start;
    b.n_wide = S.n_wide; b.wide_index = W.wide_index; b.wide_nm = W.wide_nm; b.wide_l_qseq = W.wide_lq; b.wide_n_cigar = W.wide_nc;
}
// second half of a call: wait for the window's kernels, read its summary, submit its records as a batch, park what is left
int decode_finish(rsqc_ctx *c, rsqc_decode_window *out) {
    DecodeState &D = c->dec;
    if (!D.pending) return RSQC_OK;
    D.pending = false;
    const DecodeWindow &W = D.pend_w;
    int rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (D.profile) {
        float a = 0, b = 0, d = 0;
        (void)hipEventElapsedTime(&a, D.pe[0], D.pe[1]); (void)hipEventElapsedTime(&b, D.pe[1], D.pe[2]); (void)hipEventElapsedTime(&d, D.pe[2], D.pe[3]);
        D.ms_copy += a; D.ms_inflate += b; D.ms_parse += d;
        D.ms_call += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - D.pend_wall0).count();
        D.prof_calls++;
    }
    HIP_TRY(c, hipGetLastError());
    const DecodeSummary &S = *D.h_sum;
    if (S.status & DEC_ST_INFLATE) {
        c->sticky = RSQC_ERR_INPUT;
        return fail(c, RSQC_ERR_INPUT, "BGZF inflate failed (corrupt block " + std::to_string((S.inflate_fail >> 4) - 1) + " of the call, code " + std::to_string(S.inflate_fail & 15u) + ")");
    }
    if (S.status & DEC_ST_BAD_RECORD) {
        c->sticky = RSQC_ERR_INPUT;
        if (!D.sam) return fail(c, RSQC_ERR_INPUT, "bad BAM record");
        std::string msg;
        sam_window_error(c, W, msg);
        return fail(c, RSQC_ERR_INPUT, msg);
    }
    // the reference's stderr diagnostics
    if (S.unsorted) D.unsorted = true;
    for (uint32_t k = 0; k < S.n_bad && k < DEC_MAX_BAD && D.bad_names.size() < DEC_MAX_BAD; ++k) {
        char raw[36 + 256] = {0};
        const size_t room = std::min<size_t>(D.sam ? 256 : sizeof raw, (size_t)W.end - S.bad_off[k]);
        HIP_TRY(c, hipMemcpy(raw, (const char *)D.ubuf.p + S.bad_off[k], room, hipMemcpyDeviceToHost));
        D.bad_names.push_back(D.sam ? sam_record_name(raw, room) : bam_record_name(raw, room));
    }
    D.n_bad += S.n_bad;
    // what is left of the window: an incomplete record stays in front of the next one
    const uint32_t left = D.pend_limited ? 0u : W.end - S.consumed_end;
    if (left) {
        if ((rc = dev_alloc(c, D.tailtmp, left, false))) return rc;
        HIP_TRY(c, hipMemcpyAsync(D.tailtmp.p, (const char *)D.ubuf.p + S.consumed_end, left, hipMemcpyDeviceToDevice, c->stream));
        if (left <= D.head) HIP_TRY(c, hipMemcpyAsync((char *)D.ubuf.p + D.head - left, D.tailtmp.p, left, hipMemcpyDeviceToDevice, c->stream));
    }
    if (D.sam) D.sam_line0 += D.h_sam_st->n_nl;
    D.run_tid.assign(S.n_seg, 0);
    if (S.n_seg) HIP_TRY(c, hipMemcpy(D.run_tid.data(), D.seg_tid.p, (size_t)S.n_seg * 4, hipMemcpyDeviceToHost));
    if (out) { out->n_records = S.n_rec; out->n_runs = S.n_seg; out->run_tid = D.run_tid.data(); out->device_batch = rsqc_batch{}; }
    if (S.n_rec) {
        window_columns(D.last, W, S);
        D.last.file_index_base = D.next_file_index; D.last.n_cigar_total = S.n_ops; D.last.umi = W.umi;
        if (out && !D.pipelined) out->device_batch = D.last;     // (pipelined: the next call's kernels are already queued into these buffers)
        UploadedBatch *u = new UploadedBatch();
        u->pooled = false;
        u->n = S.n_rec; u->n_cigar_total = S.n_ops; u->file_index_base = D.next_file_index;
        window_columns(u->d, W, S);
        u->umi = W.umi;
        c->transient.push_back(u);
        D.next_file_index += S.n_rec; D.records += S.n_rec;
        window_stages_seen(c, S.n_rec);
        if ((rc = run_batch(c, u))) return rc;
    }
    if (left > D.head) {
        // a record larger than the head room: every window buffer is rebuilt around a larger one (the per-read kernels of
        // this window finish first: releasing device memory waits for them)
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        uint32_t nh = D.head; while (nh < left) nh <<= 1;
        const size_t keep = D.out_cap;
        D.head = nh; D.out_cap = 0; D.tail = 0;
        if ((rc = decode_reserve(c, keep, 0, 0))) return rc;
        HIP_TRY(c, hipMemcpyAsync((char *)D.ubuf.p + D.head - left, D.tailtmp.p, left, hipMemcpyDeviceToDevice, c->stream));
    }
    D.tail = left;
    return RSQC_OK;
}
// a call's bytes and the head room in front of them are addressed with 31 bits
int check_window_limit(rsqc_ctx *c, uint64_t total) {
    if (total + c->dec.head > (1ull << 31)) return fail(c, RSQC_ERR_ARG, "too much inflated data in one rsqc_decode_submit (2 GiB with the bytes carried over)");
    return 0;
}
// where the stages of a window [W.start, W.end) read and write: the buffers of reserve_columns
void window_buffers(DecodeWindow &W, const DecodeState &D) {
    W.seg = (BamSegment *)D.seg.p; W.seg_rec0 = (uint32_t *)D.seg_rec0.p; W.seg_ops0 = (uint32_t *)D.seg_ops0.p;
    W.rec_off = (uint32_t *)D.rec_off.p; W.ops_at = (uint32_t *)D.ops_at.p; W.mark = (uint8_t *)D.mark.p;
    W.core = (rsqc_rec_core *)D.core.p; W.aux = (rsqc_rec_aux *)D.aux.p; W.qh2 = (uint32_t *)D.qh2.p; W.cigar = (uint32_t *)D.cigar.p;
    W.seg_tid = (int32_t *)D.seg_tid.p; W.seg_start = (uint64_t *)D.seg_start.p;
    W.wide_index = (uint64_t *)D.wide_index.p; W.wide_nm = (int32_t *)D.wide_nm.p; W.wide_lq = (int32_t *)D.wide_lq.p; W.wide_nc = (uint32_t *)D.wide_nc.p;
    W.sum = (DecodeSummary *)D.sum.p; W.carry = (DecodeCarry *)D.carry.p; W.tags = D.tags;
    W.umi = D.tags.umi_src ? (uint64_t *)D.umi.p : nullptr;
}
void sam_window_buffers(SamWindow &S, const DecodeState &D, const DecodeWindow &W) {
    S.W = W;
    S.base = W.start & ~63u;
    S.n_words = (W.end - S.base + 63u) / 64u;
    S.n_seg = (S.n_words + SAM_SEG_WORDS - 1) / SAM_SEG_WORDS;
    S.rec_cap = sam_window_rec_cap(D.sam_rec_cap, W.end - W.start, D.records > 0);
    S.cigar_cap = (uint32_t)std::min<size_t>(D.cigar.bytes / 4, 0xFFFFFFF0u);
    S.ebits = (uint64_t *)D.sam_ebits.p; S.tbits = (uint64_t *)D.sam_tbits.p;
    S.seg_cnt = (uint32_t *)D.sam_segcnt.p; S.seg_k0 = (uint32_t *)D.sam_segk0.p;
    S.rtid = (int32_t *)D.sam_rtid.p; S.nops = (uint32_t *)D.sam_nops.p;
    S.refs = D.sam_refs; S.st = (SamStatus *)D.sam_st.p; S.sc = (SamCarry *)D.sam_sc.p;
}
// the second half of rsqc_decode_submit / rsqc_decode_submit_text: `total` bytes for the window, of which the blocks [0, n_gpu)
// are inflated on the device and the last raw_total bytes arrive as they are, at raw_src of `compressed`
int decode_enqueue(rsqc_ctx *c, const void *compressed, uint64_t compressed_bytes, const rsqc_bgzf_block *blocks, uint32_t n_blocks, uint32_t n_gpu,
                   uint64_t total, uint64_t raw_total, uint64_t raw_src, uint32_t skip_bytes, uint64_t limit_bytes, rsqc_decode_window *out) {
    DecodeState &D = c->dec;
    int rc;
    if ((rc = check_window_limit(c, total))) return rc;
    if (skip_bytes > total) return fail(c, RSQC_ERR_ARG, "skip_bytes beyond the inflated data");
    // buffers that have to grow are in use by the call in flight: it is finished first (rare: rsqc_decode_params.reserve_inflated_bytes)
    const int slot = D.slot ^ 1;
    if (D.pending && ((size_t)total > D.out_cap || (size_t)compressed_bytes + 64 > D.comp_cap || n_blocks > D.blk_cap)) {
        if ((rc = decode_finish(c, out))) return rc;
        // (finishing the call in flight may have enlarged the head room for a carried-over record: the limit is about THIS origin)
        if ((rc = check_window_limit(c, total))) return rc;
    }
    if ((rc = decode_reserve(c, (size_t)total, (size_t)compressed_bytes, n_blocks)) || (rc = reserve_umi(c))) return rc;
    DevBgzfBlock *hb = D.h_blocks + (size_t)slot * D.blk_cap;
    uint32_t raw_at = D.head;                                           // where the caller-inflated run goes in the window
    uint32_t head_used = D.head;                                        // the window origin the table below was laid out for
    auto lay_out_blocks = [&]() {
        head_used = D.head;
        uint32_t at = D.head;
        for (uint32_t k = 0; k < n_gpu; ++k) { hb[k] = DevBgzfBlock{blocks[k].in_offset, blocks[k].in_bytes, blocks[k].out_bytes, at, blocks[k].crc32}; at += blocks[k].out_bytes; }
        raw_at = at;
    };
    lay_out_blocks();
    // the file bytes go up on the copy stream, beside the kernels of the call before this one (pipelined streams)
    uint8_t *dcomp = (uint8_t *)D.comp.p + (size_t)slot * D.comp_cap;
    DevBgzfBlock *dblk = (DevBgzfBlock *)D.blocks.p + (size_t)slot * D.blk_cap;
    if (compressed_bytes) HIP_TRY(c, hipMemcpyAsync(dcomp, compressed, (size_t)compressed_bytes, hipMemcpyHostToDevice, D.copy_stream));
    if (n_gpu) HIP_TRY(c, hipMemcpyAsync(dblk, hb, (size_t)n_gpu * sizeof(DevBgzfBlock), hipMemcpyHostToDevice, D.copy_stream));
    HIP_TRY(c, hipEventRecord(D.ev_copy, D.copy_stream));
    // the call before this one: its kernels have had the time of this call's preparation
    // (an error from here on leaves with the copy drained: the caller's buffer is the caller's again when the call returns)
    if (D.pending) { if ((rc = decode_finish(c, out))) { (void)hipStreamSynchronize(D.copy_stream); return rc; } }
    if (D.head != head_used) {
        // the call just finished left a partial record larger than the head room, and decode_finish moved the window origin to
        // make room for it: the block table above was laid out for the old origin -- lay it out again and send it once more
        // (inflating to the old places would overwrite the carried bytes and shift the window)
        if ((rc = check_window_limit(c, total))) { (void)hipStreamSynchronize(D.copy_stream); return rc; }
        HIP_TRY(c, hipStreamSynchronize(D.copy_stream));               // (the first copy of the table reads hb)
        if ((rc = decode_reserve(c, (size_t)total, (size_t)compressed_bytes, n_blocks)) || (rc = reserve_umi(c))) return rc;
        lay_out_blocks();
        if (n_gpu) HIP_TRY(c, hipMemcpyAsync(dblk, hb, (size_t)n_gpu * sizeof(DevBgzfBlock), hipMemcpyHostToDevice, D.copy_stream));
        HIP_TRY(c, hipEventRecord(D.ev_copy, D.copy_stream));
    }
    if (skip_bytes && D.tail) { (void)hipStreamSynchronize(D.copy_stream); return fail(c, RSQC_ERR_ARG, "skip_bytes in the middle of a record"); }
    D.slot = slot;
    D.pend_wall0 = std::chrono::steady_clock::now();
    if (D.profile) HIP_TRY(c, hipEventRecord(D.pe[0], c->stream));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, D.ev_copy, 0));
    HIP_TRY(c, hipMemsetAsync(D.sum.p, 0, sizeof(DecodeSummary), c->stream));
    if (D.profile) HIP_TRY(c, hipEventRecord(D.pe[1], c->stream));
    // the inflate kernel's form follows the call's compression ratio: below 5x the rounds are short matches and literals and the
    // one-pass commit pays; above, long matches dominate and it only costs (RSQC_INFLATE_ONE_PASS=0/1 forces a form)
    static const int force_one_pass = getenv("RSQC_INFLATE_ONE_PASS") ? atoi(getenv("RSQC_INFLATE_ONE_PASS")) : -1;
    const bool one_pass = force_one_pass >= 0 ? force_one_pass != 0 : total < 5 * (uint64_t)std::max<uint64_t>(compressed_bytes - raw_total, 1);
    launch_bgzf_inflate(c->stream, dcomp, dblk, n_gpu, (uint8_t *)D.ubuf.p, (DecodeSummary *)D.sum.p, one_pass);
    if (raw_total)                                                      // the caller-inflated run: staged with the file bytes, now moved into the window
        HIP_TRY(c, hipMemcpyAsync((char *)D.ubuf.p + raw_at, dcomp + raw_src, (size_t)raw_total, hipMemcpyDeviceToDevice, c->stream));
    const bool limited = limit_bytes && limit_bytes < total;
    DecodeWindow &W = D.pend_w;
    W = DecodeWindow{};
    W.buf = (const uint8_t *)D.ubuf.p;
    W.start = D.head - D.tail + skip_bytes;
    W.end = D.head + (uint32_t)(limited ? limit_bytes : total);
    if (W.start > W.end) W.start = W.end;
    W.n_seg = (W.end - W.start + DEC_SEG_BYTES - 1) / DEC_SEG_BYTES;
    window_buffers(W, D);
    if (D.profile) HIP_TRY(c, hipEventRecord(D.pe[2], c->stream));
    if (D.sam) {
        SamWindow &S = D.pend_s;
        S = SamWindow{};
        sam_window_buffers(S, D, W);
        HIP_TRY(c, hipMemsetAsync(D.sam_st.p, 0, sizeof(SamStatus), c->stream));
        HIP_TRY(c, hipMemsetAsync(&S.st->hdr_end, 0xff, 4, c->stream));
        HIP_TRY(c, hipMemsetAsync(&S.st->first_bad, 0xff, 4, c->stream));
        launch_sam_window(c->stream, S, (uint32_t *)D.sam_scratch.p);
    } else
    launch_decode_window(c->stream, W, (uint32_t *)D.scratch.p);
    if (D.profile) HIP_TRY(c, hipEventRecord(D.pe[3], c->stream));
    if ((rc = window_stages_launch(c, W, D.sam ? &D.pend_s : nullptr))) return rc;      // --cycles, --mismatches, --alleles: a kernel each over the window's records
    HIP_TRY(c, hipMemcpyAsync(D.h_sum, D.sum.p, sizeof(DecodeSummary), hipMemcpyDeviceToHost, c->stream));
    if (D.sam) HIP_TRY(c, hipMemcpyAsync(D.h_sam_st, D.sam_st.p, sizeof(SamStatus), hipMemcpyDeviceToHost, c->stream));
    D.pending = true; D.pend_limited = limited;
    if (D.profile) { D.prof_in += compressed_bytes; D.prof_out += total; }
    // the caller's buffer is free again once the copy is through (the copy engine works beside the kernels)
    HIP_TRY(c, hipStreamSynchronize(D.copy_stream));
    if (!D.pipelined) return decode_finish(c, out);
    return RSQC_OK;
}

int decode_begin_common(rsqc_ctx *c, const rsqc_decode_params *p, bool sam) {
    if (!c || !p || p->n_ref < 0) return RSQC_ERR_ARG;
    if (!c->have_ann) return fail(c, RSQC_ERR_ARG, "rsqc_set_annotation must precede rsqc_decode_begin");
    HIP_TRY(c, hipSetDevice(c->device));
    DecodeState &D = c->dec;
    D.tags = BamTagSpec{};
    D.tags.n_ref = p->n_ref;
    if (p->has_chimeric_tag) { D.tags.have_ch = 1; D.tags.ch0 = (uint8_t)p->chimeric_tag[0]; D.tags.ch1 = (uint8_t)p->chimeric_tag[1]; }
    D.tags.n_filter = (uint8_t)c->params.n_filter_tags;
    for (int k = 0; k < c->params.n_filter_tags; ++k) { D.tags.f0[k] = (uint8_t)p->filter_tag[k][0]; D.tags.f1[k] = (uint8_t)p->filter_tag[k][1]; }
    if (p->umi_source > RSQC_UMI_SOURCE_QNAME) return fail(c, RSQC_ERR_ARG, "rsqc_decode_params.umi_source: 0 (none), 1 (tag) or 2 (read name)");
    D.tags.umi_src = p->umi_source; D.tags.umi_t0 = (uint8_t)p->umi_tag[0]; D.tags.umi_t1 = (uint8_t)p->umi_tag[1]; D.tags.umi_sep = (uint8_t)p->umi_sep;
    D.next_file_index = p->file_index_base; D.records = 0; D.tail = 0;
    D.unsorted = false; D.n_bad = 0; D.bad_names.clear();
    D.pipelined = p->pipelined != 0; D.pending = false; D.slot = 0;
    D.sam = sam; D.sam_line0 = 1;
    if (!D.copy_stream) { HIP_TRY(c, hipStreamCreateWithFlags(&D.copy_stream, hipStreamNonBlocking)); HIP_TRY(c, hipEventCreateWithFlags(&D.ev_copy, hipEventDisableTiming)); }
    D.profile = getenv("RSQC_DECODE_PROFILE") != nullptr;
    D.ms_copy = D.ms_inflate = D.ms_parse = D.ms_call = 0; D.prof_in = D.prof_out = D.prof_calls = 0;
    D.prof_t0 = std::chrono::steady_clock::now();
    if (D.profile && !D.pe[0]) for (auto &e : D.pe) HIP_TRY(c, hipEventCreate(&e));
    int rc;
    if ((rc = dev_alloc(c, D.sum, sizeof(DecodeSummary), false)) || (rc = dev_alloc(c, D.carry, sizeof(DecodeCarry), true)) ||
        (rc = dev_alloc(c, D.scratch, DEC_SCRATCH_WORDS * 4, false))) return rc;
    if (!D.h_sum) HIP_TRY(c, hipHostMalloc((void **)&D.h_sum, sizeof(DecodeSummary), hipHostMallocDefault));
    if (p->reserve_inflated_bytes) {
        const size_t want = (size_t)std::min<uint64_t>(p->reserve_inflated_bytes, (1ull << 31) - D.head);
        if ((rc = decode_reserve(c, want, want / 2, want / 32768 + 64))) return rc;
    }
    D.active = true;
    return RSQC_OK;
}

}  // namespace

int rsqc_decode_begin(rsqc_ctx *c, const rsqc_decode_params *p) { return decode_begin_common(c, p, false); }

int rsqc_decode_begin_sam(rsqc_ctx *c, const rsqc_decode_params *p, const char *const *ref_names) {
    if (!c || !p || p->n_ref < 0 || (p->n_ref > 0 && !ref_names)) return RSQC_ERR_ARG;
    if (!c->have_ann) return fail(c, RSQC_ERR_ARG, "rsqc_set_annotation must precede rsqc_decode_begin_sam");
    HIP_TRY(c, hipSetDevice(c->device));
    DecodeState &D = c->dec;
    // the @SQ names: an open-addressed table on their FNV-1a hash, at least twice as many slots as names (first name wins)
    D.sam_ref_names.assign(ref_names, ref_names + p->n_ref);
    uint32_t slots = 16;
    while (slots < 2u * (uint32_t)p->n_ref) slots <<= 1;
    std::vector<SamRefSlot> tab(slots, SamRefSlot{0, 0, 0, -1, 0});
    std::vector<uint8_t> names;
    for (int32_t r = 0; r < p->n_ref; ++r) {
        const std::string &nm = D.sam_ref_names[(size_t)r];
        const uint64_t h = bam_qname_hash((const uint8_t *)nm.data(), (uint32_t)nm.size());
        uint32_t k = (uint32_t)h & (slots - 1);
        bool dup = false;
        for (; tab[k].idx >= 0; k = (k + 1) & (slots - 1))
            if (tab[k].hash == h && tab[k].len == nm.size() && !memcmp(names.data() + tab[k].off, nm.data(), nm.size())) { dup = true; break; }
        if (dup) continue;
        tab[k] = SamRefSlot{h, (uint32_t)names.size(), (uint32_t)nm.size(), r, 0};
        names.insert(names.end(), nm.begin(), nm.end());
    }
    int rc;
    if ((rc = dev_alloc(c, D.sam_slots, tab.size() * sizeof(SamRefSlot), false)) || (rc = dev_alloc(c, D.sam_names, names.size() + 16, false)) ||
        (rc = dev_alloc(c, D.sam_st, sizeof(SamStatus), false)) || (rc = dev_alloc(c, D.sam_sc, sizeof(SamCarry), true))) return rc;
    HIP_TRY(c, hipMemcpyAsync(D.sam_slots.p, tab.data(), tab.size() * sizeof(SamRefSlot), hipMemcpyHostToDevice, c->stream));
    if (!names.empty()) HIP_TRY(c, hipMemcpyAsync(D.sam_names.p, names.data(), names.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    D.sam_refs = SamRefTable{(const SamRefSlot *)D.sam_slots.p, (const uint8_t *)D.sam_names.p, slots - 1, p->n_ref};
    if (!D.h_sam_st) HIP_TRY(c, hipHostMalloc((void **)&D.h_sam_st, sizeof(SamStatus), hipHostMallocDefault));
    return decode_begin_common(c, p, true);
}

int rsqc_decode_submit(rsqc_ctx *c, const void *compressed, uint64_t compressed_bytes, const rsqc_bgzf_block *blocks, uint32_t n_blocks,
                       uint32_t skip_bytes, uint64_t limit_bytes, rsqc_decode_window *out) {
    if (!c || (!compressed && compressed_bytes) || (!blocks && n_blocks)) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    DecodeState &D = c->dec;
    if (!D.active) return fail(c, RSQC_ERR_ARG, "rsqc_decode_begin must precede rsqc_decode_submit");
    if (out) { out->n_records = 0; out->n_runs = 0; out->run_tid = nullptr; out->device_batch = rsqc_batch{}; }
    D.last = rsqc_batch{};
    HIP_TRY(c, hipSetDevice(c->device));
    uint64_t total = 0, raw_total = 0;
    uint32_t n_gpu = n_blocks;                                          // blocks [n_gpu, n_blocks) arrive inflated (RSQC_BGZF_INFLATED)
    for (uint32_t k = 0; k < n_blocks; ++k) {
        const rsqc_bgzf_block &b = blocks[k];
        if (b.out_bytes > 65536u || b.in_offset > compressed_bytes || b.in_bytes > compressed_bytes - b.in_offset)
            return fail(c, RSQC_ERR_ARG, "BGZF block outside the compressed buffer or with ISIZE above 64 KiB");
        if (b.flags & RSQC_BGZF_INFLATED) {
            if (n_gpu == n_blocks) n_gpu = k;
            if (b.in_bytes != b.out_bytes || b.in_offset != blocks[n_gpu].in_offset + raw_total)
                return fail(c, RSQC_ERR_ARG, "inflated blocks must lie one after the other in the buffer, in_bytes == out_bytes");
            raw_total += b.out_bytes;
        } else if (n_gpu != n_blocks) return fail(c, RSQC_ERR_ARG, "inflated blocks must form one run at the end of the call");
        total += b.out_bytes;
    }
    return decode_enqueue(c, compressed, compressed_bytes, blocks, n_blocks, n_gpu, total, raw_total, n_gpu < n_blocks ? blocks[n_gpu].in_offset : 0,
                          skip_bytes, limit_bytes, out);
}

int rsqc_decode_submit_text(rsqc_ctx *c, const void *text, uint64_t bytes, rsqc_decode_window *out) {
    if (!c || (!text && bytes)) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    DecodeState &D = c->dec;
    if (!D.active) return fail(c, RSQC_ERR_ARG, "rsqc_decode_begin_sam must precede rsqc_decode_submit_text");
    if (!D.sam) return fail(c, RSQC_ERR_ARG, "rsqc_decode_submit_text needs a SAM stream (rsqc_decode_begin_sam)");
    if (out) { out->n_records = 0; out->n_runs = 0; out->run_tid = nullptr; out->device_batch = rsqc_batch{}; }
    D.last = rsqc_batch{};
    HIP_TRY(c, hipSetDevice(c->device));
    // the text crosses PCIe like a run of caller-inflated blocks: staged on the copy stream, then moved into the window
    return decode_enqueue(c, text, bytes, nullptr, 0, 0, bytes, bytes, 0, 0, 0, out);
}

int rsqc_decode_end(rsqc_ctx *c, rsqc_decode_info *out) {
    if (!c) return RSQC_ERR_ARG;
    DecodeState &D = c->dec;
    if (!D.active) return fail(c, RSQC_ERR_ARG, "rsqc_decode_begin must precede rsqc_decode_end");
    rsqc_decode_window last{};
    if (D.pending) { const int rcf = decode_finish(c, &last); if (rcf) { D.active = false; return rcf; } }
    if (D.sam && D.tail && !c->sticky) {
        // a last line without its '\n' (htslib reads it): ended here, in one more (non-pipelined) window
        D.sam_last_runs.assign(last.run_tid, last.run_tid + last.n_runs);
        const uint64_t na = last.n_records;
        const bool pl = D.pipelined;
        D.pipelined = false;
        rsqc_decode_window b{};
        const int rcb = rsqc_decode_submit_text(c, "\n", 1, &b);
        D.pipelined = pl;
        if (rcb) { D.active = false; return rcb; }
        D.sam_last_runs.insert(D.sam_last_runs.end(), b.run_tid, b.run_tid + b.n_runs);
        last = b;
        last.n_records += na; last.n_runs = (uint32_t)D.sam_last_runs.size(); last.run_tid = D.sam_last_runs.data();
        if (pl || na) last.device_batch = rsqc_batch{};
    }
    D.active = false;
    if (out) out->last = last;
    if (D.profile)
        fprintf(stderr, "[decode] %llu calls, %.1f MB in, %.1f MB inflated: copy %.1f ms, inflate %.1f ms (%.2f GB/s out), frame+parse %.1f ms, in the calls %.1f ms of %.1f ms between begin and end\n",
                (unsigned long long)D.prof_calls, D.prof_in / 1e6, D.prof_out / 1e6, D.ms_copy, D.ms_inflate, D.ms_inflate > 0 ? D.prof_out / D.ms_inflate / 1e6 : 0.0,
                D.ms_parse, D.ms_call, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - D.prof_t0).count());
    if (out) {
        D.bad_ptrs.clear();
        for (auto &n : D.bad_names) D.bad_ptrs.push_back(n.c_str());
        out->records = D.records; out->unsorted = D.unsorted ? 1 : 0;
        out->n_bad_refid = (int32_t)std::min<uint64_t>(D.n_bad, 0x7fffffff);
        out->bad_refid = D.bad_ptrs.data();
    }
    if (D.tail) {
        D.tail = 0;
        if (D.sam && c->sticky) return c->sticky;                      // (the malformed line's message stays the last error)
        return fail(c, RSQC_ERR_INPUT, D.sam ? "truncated SAM line" : "truncated BAM record");
    }
    return RSQC_OK;
}
