// sam_emu.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// Compiles the product's SAM text decode (rnaseqc_amd/csrc/rsqc_samrec.h: one line -> the batch columns; rsqc_sam.h: the
// per-lane bodies of the device stages) with g++ and runs a stream of windows through the stages as a wave of ONE lane,
// so that what the HIP kernels execute can be diffed against the BAM decode of the same records in the GPU-less build
// container.  The exclusive sums between the stages are plain loops here.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../rnaseqc_amd/csrc/rsqc_sam.h"

using namespace rsqc;

#define EMU_API extern "C" __attribute__((visibility("default")))

namespace {
struct Stream {
    BamTagSpec tags{};
    std::vector<SamRefSlot> slots; std::vector<uint8_t> names; SamRefTable refs{};
    std::vector<uint8_t> carry;
    DecodeCarry dc{}; SamCarry sc{};
    uint64_t line0 = 1, records = 0;
    // the stream's columns, whole-stream numbering
    std::vector<rsqc_rec_core> core; std::vector<rsqc_rec_aux> aux; std::vector<uint32_t> qh2, cigar;
    std::vector<int32_t> seg_tid; std::vector<uint64_t> seg_start;
    std::vector<uint64_t> wide_index; std::vector<int32_t> wide_nm, wide_lq; std::vector<uint32_t> wide_nc;
    int unsorted = 0; uint64_t n_bad = 0; std::vector<std::string> bad_names;
    uint64_t err_line = 0; uint32_t err_code = 0;
    uint64_t windows = 0;
    size_t buf_bytes = 0;            // the window buffer the ABI would have (0: just the window: the tightest it ever is)
};
Stream g;
}  // namespace

EMU_API void emu_sam_begin(int32_t n_ref, const char *const *names, const BamTagSpec *tags, uint64_t buf_bytes) {
    g = Stream{};
    g.buf_bytes = (size_t)buf_bytes;
    g.tags = *tags; g.tags.n_ref = n_ref;
    uint32_t slots = 16;
    while (slots < 2u * (uint32_t)n_ref) slots <<= 1;
    g.slots.assign(slots, SamRefSlot{0, 0, 0, -1, 0});
    for (int32_t r = 0; r < n_ref; ++r) {
        const uint32_t len = (uint32_t)strlen(names[r]);
        const uint64_t h = bam_qname_hash((const uint8_t *)names[r], len);
        uint32_t k = (uint32_t)h & (slots - 1);
        bool dup = false;
        for (; g.slots[k].idx >= 0; k = (k + 1) & (slots - 1))
            if (g.slots[k].hash == h && g.slots[k].len == len && !memcmp(g.names.data() + g.slots[k].off, names[r], len)) { dup = true; break; }
        if (dup) continue;
        g.slots[k] = SamRefSlot{h, (uint32_t)g.names.size(), len, r, 0};
        g.names.insert(g.names.end(), names[r], names[r] + len);
    }
    g.names.push_back(0);
    g.refs = SamRefTable{g.slots.data(), g.names.data(), slots - 1, n_ref};
}

// one call: the carried bytes + `len` bytes of text as one window.  list_threads: how many records one lists "thread" takes
// (the chunking of the kernels' list step).  Returns 0, or the SAM_ERR_* of the first malformed line (emu_sam_error: its line).
EMU_API int emu_sam_submit(const uint8_t *text, uint32_t len, uint32_t per_thread) {
    std::vector<uint8_t> buf(g.carry);
    buf.insert(buf.end(), text, text + len);
    const uint32_t end = (uint32_t)buf.size();
    // every array exactly as large as the ABI makes it for a window buffer of max(buf_bytes, end) bytes (the record columns,
    // the operation column and the bitmaps by sam_caps / sam_window_rec_cap), the text with the 63 bytes the bitmap's last word
    // reads past its end: the sanitizers of tests/hostemu/sam_fuzz.cpp see any access the device would make outside them
    buf.resize(buf.size() + 63, 0);
    const size_t wb = std::max<size_t>(g.buf_bytes, end);
    const SamCaps caps = sam_caps(wb);
    const uint32_t n_words = (end + 63u) / 64u, rec_cap = sam_window_rec_cap(caps.rec_alloc, end, g.records > 0), n_rec = caps.rec_alloc;
    std::vector<uint64_t> eb(wb / 64 + 8, 0), tb(wb / 64 + 8, 0);
    std::vector<uint32_t> rec_off(n_rec), ops_at(n_rec), nops(n_rec);
    std::vector<int32_t> rtid(n_rec);
    std::vector<uint8_t> mark(n_rec);
    std::vector<rsqc_rec_core> core(n_rec); std::vector<rsqc_rec_aux> aux(n_rec); std::vector<uint32_t> qh2(n_rec);
    std::vector<int32_t> seg_tid(n_rec); std::vector<uint64_t> seg_start(n_rec + 1);
    std::vector<uint64_t> wide_index(n_rec); std::vector<int32_t> wide_nm(n_rec), wide_lq(n_rec); std::vector<uint32_t> wide_nc(n_rec);
    DecodeSummary sum{}; SamStatus st{}; st.hdr_end = SAM_NONE; st.first_bad = SAM_NONE;
    std::vector<uint32_t> cigar(caps.cigar_alloc);
    SamWindow S{};
    DecodeWindow &W = S.W;
    W.buf = buf.data(); W.start = 0; W.end = end;
    W.rec_off = rec_off.data(); W.ops_at = ops_at.data(); W.mark = mark.data();
    W.core = core.data(); W.aux = aux.data(); W.qh2 = qh2.data(); W.cigar = cigar.data();
    W.seg_tid = seg_tid.data(); W.seg_start = seg_start.data();
    W.wide_index = wide_index.data(); W.wide_nm = wide_nm.data(); W.wide_lq = wide_lq.data(); W.wide_nc = wide_nc.data();
    W.sum = &sum; W.carry = &g.dc; W.tags = g.tags;
    S.ebits = eb.data(); S.tbits = tb.data(); S.base = 0; S.n_words = n_words; S.n_seg = (n_words + SAM_SEG_WORDS - 1) / SAM_SEG_WORDS;
    S.rec_cap = rec_cap; S.cigar_cap = caps.cigar_alloc; S.rtid = rtid.data(); S.nops = nops.data(); S.refs = g.refs; S.st = &st; S.sc = &g.sc;
    // bitmap + lines (the segment sums as a running count)
    std::vector<uint32_t> wc(n_words);
    for (uint32_t w = 0; w < n_words; ++w) {
        const SamWordCounts c = sam_bitmap_word(S, w);
        wc[w] = c.rec; st.n_nl += c.nl; if (c.last_nl1 > st.last_nl1) st.last_nl1 = c.last_nl1;
    }
    uint32_t k = 0;
    for (uint32_t w = 0; w < n_words; ++w) { if (wc[w]) sam_lines_word(S, w, k); k += wc[w]; }
    st.n_lines = k;
    if (!g.sc.records_seen)
        for (uint32_t i = 0; i < std::min(k, rec_cap); ++i) if (!sam_is_header_line(S, i)) { st.hdr_end = i; break; }
    sam_settle(S);
    const uint32_t n = sum.n_rec;
    auto fail_here = [&]() {
        uint64_t line = 0; uint32_t code = 0;
        g.err_line = 0; g.err_code = SAM_ERR_FIELDS;
        if (sam_find_bad_line(buf.data(), end, g.records > 0, g.tags, g.line0, line, code)) { g.err_line = line; g.err_code = code; }
        return (int)g.err_code;
    };
    if (sum.status) return fail_here();
    uint32_t ops = 0;
    for (uint32_t j = 0; j < n; ++j) { nops[j] = sam_fields_one(S, j); ops_at[j] = ops; ops += nops[j]; }
    sum.n_ops = ops;
    for (uint32_t j = 0; j < n; ++j) if (sam_parse_one(S, j) != SAM_OK) return fail_here();
    bool uns = false;
    for (uint32_t j = 0; j < n; ++j) sam_mark_one(S, j, uns);
    // lists: per "thread" counts, exclusive sums, writes
    const uint32_t per = per_thread ? per_thread : 32;
    DecodeListCounts tot{0, 0, 0, -1};
    std::vector<DecodeListCounts> base;
    for (uint32_t lo = 0; lo < n; lo += per) {
        DecodeListCounts c;
        decode_lists_count(W, lo, std::min(n, lo + per), c);
        base.push_back(DecodeListCounts{tot.seg, tot.wide, tot.bad, -1});
        tot.seg += c.seg; tot.wide += c.wide; tot.bad += c.bad; if (c.last_judged >= 0) tot.last_judged = c.last_judged;
    }
    for (uint32_t lo = 0, t = 0; lo < n; lo += per, ++t) sam_lists_write(S, lo, std::min(n, lo + per), base[t]);
    sam_lists_finish(S, n, tot);
    // the window's output, appended to the stream's
    const uint64_t at = g.core.size(), ops0 = g.cigar.size();
    for (uint32_t j = 0; j < n; ++j) { rsqc_rec_core c = core[j]; c.cigar_off += (uint32_t)ops0; g.core.push_back(c); g.aux.push_back(aux[j]); g.qh2.push_back(qh2[j]); }
    g.cigar.insert(g.cigar.end(), cigar.begin(), cigar.begin() + ops);
    for (uint32_t s = 0; s < sum.n_seg; ++s)
        if (g.seg_tid.empty() || g.seg_tid.back() != seg_tid[s] || s > 0) { g.seg_tid.push_back(seg_tid[s]); g.seg_start.push_back(at + seg_start[s]); }
    for (uint32_t w = 0; w < sum.n_wide; ++w) { g.wide_index.push_back(at + wide_index[w]); g.wide_nm.push_back(wide_nm[w]); g.wide_lq.push_back(wide_lq[w]); g.wide_nc.push_back(wide_nc[w]); }
    for (uint32_t b = 0; b < sum.n_bad && b < DEC_MAX_BAD; ++b) {
        uint32_t l = sum.bad_off[b];
        std::string nm;
        while (l < end && buf[l] != '\t') nm.push_back((char)buf[l++]);
        g.bad_names.push_back(nm);
    }
    g.n_bad += sum.n_bad;
    if (uns) g.unsorted = 1;
    g.records += n; g.line0 += st.n_nl; ++g.windows;
    g.carry.assign(buf.begin() + sum.consumed_end, buf.begin() + end);
    return 0;
}
// end of the stream: a last line without '\n' is ended
EMU_API int emu_sam_end() {
    if (g.carry.empty()) return 0;
    const uint8_t nl = '\n';
    return emu_sam_submit(&nl, 1, 32);
}
EMU_API void emu_sam_error(uint64_t *line, uint32_t *code) { *line = g.err_line; *code = g.err_code; }
EMU_API void emu_sam_counts(uint64_t *out /* [8] */) {
    out[0] = g.core.size(); out[1] = g.cigar.size(); out[2] = g.seg_tid.size(); out[3] = g.wide_index.size();
    out[4] = (uint64_t)g.unsorted; out[5] = g.n_bad; out[6] = g.windows; out[7] = g.carry.size();
}
EMU_API void emu_sam_fetch(rsqc_rec_core *core, rsqc_rec_aux *aux, uint32_t *qh2, uint32_t *cigar, int32_t *seg_tid, uint64_t *seg_start,
                           uint64_t *wide_index, int32_t *wide_nm, int32_t *wide_lq, uint32_t *wide_nc) {
    memcpy(core, g.core.data(), g.core.size() * sizeof(rsqc_rec_core)); memcpy(aux, g.aux.data(), g.aux.size() * sizeof(rsqc_rec_aux));
    memcpy(qh2, g.qh2.data(), g.qh2.size() * 4); memcpy(cigar, g.cigar.data(), g.cigar.size() * 4);
    memcpy(seg_tid, g.seg_tid.data(), g.seg_tid.size() * 4); memcpy(seg_start, g.seg_start.data(), g.seg_start.size() * 8);
    memcpy(wide_index, g.wide_index.data(), g.wide_index.size() * 8); memcpy(wide_nm, g.wide_nm.data(), g.wide_nm.size() * 4);
    memcpy(wide_lq, g.wide_lq.data(), g.wide_lq.size() * 4); memcpy(wide_nc, g.wide_nc.data(), g.wide_nc.size() * 4);
}
EMU_API const char *emu_sam_bad_name(uint32_t k) { return k < g.bad_names.size() ? g.bad_names[k].c_str() : ""; }

// one line through sam_parse_line (the refs of the last emu_sam_begin): out = {code, tid, pos, mpos, isize, flag, mapq,
// l_seq, nm, n_ops, tagbits, wide, qname_len, qhash2, qhash lo, qhash hi}; ops (may be null, room for max_ops)
EMU_API uint32_t emu_sam_parse_line(const uint8_t *s, uint32_t len, int64_t *out, uint32_t *ops, uint32_t max_ops) {
    BamRecOut o{};
    const uint32_t rc = sam_parse_line(s, len, g.tags, g.refs, o, ops, max_ops);
    const int64_t v[16] = {rc, o.tid, o.core.pos, o.core.mpos, o.core.isize, o.aux.flag, o.aux.mapq, o.l_seq, o.nm, o.n_ops,
                           o.aux.tagbits, o.wide, o.qname_len, o.qhash2, (int64_t)(o.aux.qhash & 0xFFFFFFFFull), (int64_t)(o.aux.qhash >> 32)};
    memcpy(out, v, sizeof v);
    return rc;
}
// one BAM record (block_size first) through bam_parse_record, the same `out` layout; ops copied out
EMU_API uint32_t emu_bam_parse_record(const uint8_t *rec, int64_t *out, uint32_t *ops, uint32_t max_ops) {
    BamRecOut o{};
    uint32_t bs; memcpy(&bs, rec, 4);
    const bool ok = bam_parse_record(rec, bs, g.tags, o);
    const int64_t v[16] = {ok ? 0 : 1, o.tid, o.core.pos, o.core.mpos, o.core.isize, o.aux.flag, o.aux.mapq, o.l_seq, o.nm, o.n_ops,
                           o.aux.tagbits, o.wide, o.qname_len, o.qhash2, (int64_t)(o.aux.qhash & 0xFFFFFFFFull), (int64_t)(o.aux.qhash >> 32)};
    memcpy(out, v, sizeof v);
    if (ok && ops) for (uint32_t k = 0; k < o.n_ops && k < max_ops; ++k) memcpy(ops + k, rec + o.ops_off + 4u * k, 4);
    return ok ? 0 : 1;
}
