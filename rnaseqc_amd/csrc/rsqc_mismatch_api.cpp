// rsqc_mismatch_api.cpp -- rsqc_mismatch_begin / rsqc_mismatch_add / rsqc_mismatch_end: the reference goes to the device once, four bits
// per base; the counts of the records' walk over SEQ, QUAL and that reference (the kernel of rsqc_mismatch.hip behind every window),
// checked at the end against each other and against the device's own sum of lengths.  What the stage shares with the other two behind a
// window is in rsqc_window_stage_api.cpp.
#include "rsqc_ctx.h"
#include "rsqc_mismatch.h"

namespace {

constexpr size_t TABLE_BYTES = (size_t)MM_TABLE_WORDS * 8;
constexpr WindowNames NAMES{"rsqc_mismatch_begin", "rsqc_mismatch_add", "rsqc_mismatch_end", "mismatches"};
constexpr size_t AT_SUBST = MM_CYC_CELLS, AT_BYQ = AT_SUBST + MM_SUBST_CELLS, AT_SCAL = AT_BYQ + MM_BYQ_CELLS;

MismatchTables device_tables(const MismatchState &M) {
    unsigned long long *p = (unsigned long long *)M.tab.p;
    return MismatchTables{p, p + AT_SUBST, p + AT_BYQ, p + AT_SCAL};
}
MismatchPackedRef device_ref(const MismatchState &M) {
    return MismatchPackedRef{(const uint32_t *)M.ref_words.p, (const unsigned long long *)M.ref_off.p, (const unsigned long long *)M.ref_len.p, (int32_t)M.ref_length.size()};
}

void drop_reference(MismatchState &M) {
    M.ref_words.release(); M.ref_off.release(); M.ref_len.release();
    M.ref_length.clear(); M.have_ref = false;
}

// the contigs' bases through one staging buffer (the longest contig) into 4 bits each
int pack_reference(rsqc_ctx *c, int32_t n, const uint64_t *length, const char *const *sequence) {
    MismatchState &M = c->mm;
    drop_reference(M);
    std::vector<unsigned long long> off((size_t)n, ~0ull), len((size_t)n, 0ull);
    uint64_t words = 0, longest = 0;
    for (int32_t i = 0; i < n; ++i) {
        len[(size_t)i] = length[i];
        if (!sequence[i]) continue;
        off[(size_t)i] = words;
        words += (length[i] + 7) / 8;
        longest = std::max<uint64_t>(longest, length[i]);
    }
    const std::string sizes = std::to_string(words * 4) + " bytes for the packed reference, " + std::to_string(longest + 64) + " while staging its longest contig, " +
                              std::to_string((size_t)n * 16) + " for its offsets and lengths";
    DevBuf stage;
    if (!dev_reserve(M.ref_words, (size_t)(words + 2) * 4) || !dev_reserve(M.ref_off, (size_t)std::max(n, 1) * 8) || !dev_reserve(M.ref_len, (size_t)std::max(n, 1) * 8) ||
        !dev_reserve(stage, (size_t)longest + 64)) {
        stage.release(); drop_reference(M);
        return fail(c, RSQC_ERR_CAPACITY, "rsqc_mismatch_begin: no device memory for the reference (" + sizes + ")");
    }
    auto failed = [&](hipError_t e, const char *what) {
        (void)hipStreamSynchronize(c->stream);
        stage.release(); drop_reference(M);
        return fail(c, RSQC_ERR_HIP, std::string("rsqc_mismatch_begin: ") + what + ": " + hipGetErrorString(e));
    };
    hipError_t e;
    if (n && (e = hipMemcpyAsync(M.ref_off.p, off.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream)) != hipSuccess) return failed(e, "offsets");
    if (n && (e = hipMemcpyAsync(M.ref_len.p, len.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream)) != hipSuccess) return failed(e, "lengths");
    for (int32_t i = 0; i < n; ++i) {
        if (!sequence[i] || !length[i]) continue;
        if ((e = hipMemcpyAsync(stage.p, sequence[i], (size_t)length[i], hipMemcpyHostToDevice, c->stream)) != hipSuccess) return failed(e, "bases");
        launch_mismatch_pack(c->stream, (const uint8_t *)stage.p, length[i], (uint32_t *)M.ref_words.p + off[(size_t)i]);
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return failed(e, "pack");          // the caller's string and the staging buffer are reused
    }
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess || (e = hipGetLastError()) != hipSuccess) return failed(e, "pack");
    stage.release();
    M.ref_length.assign(length, length + n);
    M.have_ref = true;
    return 0;
}

int mismatch_finish(rsqc_ctx *c, double ms) {
    MismatchState &M = c->mm;
    uint64_t *h = (uint64_t *)M.h_tab.p;
    rsqc_mismatch_info &I = M.info;
    I = rsqc_mismatch_info{};
    I.mismatch_ms = ms;
    window_sum_added(M, h, MM_TABLE_WORDS);
    const uint64_t *cyc = h, *subst = h + AT_SUBST, *byq = h + AT_BYQ, *s = h + AT_SCAL;
    I.seen_records = M.seen + M.added_seen;
    I.records = s[MM_S_RECORDS]; I.no_reference_records = s[MM_S_NO_REF]; I.low_mapq_records = s[MM_S_LOW_MAPQ]; I.no_seq_records = s[MM_S_NO_SEQ];
    I.inconsistent_records = s[MM_S_INCONSISTENT]; I.no_qual_records = s[MM_S_NO_QUAL];
    I.insertion_events = s[MM_S_INS_EVENTS]; I.deletion_events = s[MM_S_DEL_EVENTS]; I.deleted_bases = s[MM_S_DEL_BASES];
    I.beyond_bases = s[MM_S_BEYOND]; I.clamped_quals = s[MM_S_CLAMPED];
    for (uint32_t e = 0; e < MM_ENDS; ++e) {
        uint64_t compared = 0, mismatched = 0, all = 0, off_diagonal = 0;
        for (uint32_t cy = 0; cy < MM_MAX; ++cy) {
            const uint64_t *cell = cyc + ((size_t)e * MM_MAX + cy) * MM_COLS;
            if (cell[MM_MISMATCH] > cell[MM_COMPARED])
                return fail(c, RSQC_ERR_HIP, "rsqc_mismatch_end: end " + std::to_string(e + 1) + " cycle " + std::to_string(cy + 1) + " holds " + std::to_string(cell[MM_MISMATCH]) +
                                                 " mismatches for " + std::to_string(cell[MM_COMPARED]) + " compared bases");
            compared += cell[MM_COMPARED]; mismatched += cell[MM_MISMATCH];
            I.uncompared += cell[MM_UNCOMPARED]; I.inserted += cell[MM_INSERTED]; I.clipped += cell[MM_CLIPPED]; I.deletions += cell[MM_DELETIONS];
        }
        for (uint32_t k = 0; k < 16u; ++k) { all += subst[e * 16u + k]; if (k / 4u != k % 4u) off_diagonal += subst[e * 16u + k]; }
        if (all != compared || off_diagonal != mismatched)
            return fail(c, RSQC_ERR_HIP, "rsqc_mismatch_end: end " + std::to_string(e + 1) + " has " + std::to_string(compared) + " compared bases and " + std::to_string(mismatched) +
                                             " mismatches by cycle, " + std::to_string(all) + " and " + std::to_string(off_diagonal) + " by substitution type");
        I.compared += compared; I.mismatched += mismatched;
    }
    uint64_t by_quality = 0;
    for (uint32_t v = 0; v < MM_QBINS; ++v) by_quality += byq[v * 2u];
    if (by_quality > I.compared)
        return fail(c, RSQC_ERR_HIP, "rsqc_mismatch_end: " + std::to_string(by_quality) + " compared bases by quality, " + std::to_string(I.compared) + " by cycle");
    if (I.compared + I.uncompared + I.inserted + I.clipped + I.beyond_bases != s[MM_S_LEN_SUM])
        return fail(c, RSQC_ERR_HIP, "rsqc_mismatch_end: the tables hold " + std::to_string(I.compared + I.uncompared + I.inserted + I.clipped) + " query bases and " +
                                         std::to_string(I.beyond_bases) + " lie beyond them, the records' lengths add up to " + std::to_string(s[MM_S_LEN_SUM]));
    return 0;
}

}  // namespace

namespace rsqc {

void mismatch_drop(rsqc_ctx *c, bool free_buffers) {
    window_drop(c, c->mm, free_buffers);
    if (free_buffers) drop_reference(c->mm);
}

void mismatch_launch(rsqc_ctx *c, const DecodeWindow &W, const SamWindow *S) {
    const MismatchState &M = c->mm;
    if (S) launch_mismatch_sam(c->stream, *S, device_ref(M), M.min_mapq, device_tables(M));
    else launch_mismatch_bam(c->stream, W, device_ref(M), M.min_mapq, device_tables(M));
}

}  // namespace rsqc

int rsqc_mismatch_begin(rsqc_ctx *c, int32_t n, const uint64_t *length, const char *const *sequence, uint32_t min_mapq) {
    if (!c) return RSQC_ERR_ARG;
    MismatchState &M = c->mm;
    if (int rc = window_begin_check(c, M, NAMES)) return rc;
    if (n < 0 || (n > 0 && !length)) return fail(c, RSQC_ERR_ARG, "rsqc_mismatch_begin: contigs without lengths");
    if (min_mapq > 255u) return fail(c, RSQC_ERR_ARG, "rsqc_mismatch_begin: min_mapq above 255");
    if (!sequence) {
        if (!M.have_ref) return fail(c, RSQC_ERR_ARG, "rsqc_mismatch_begin: sequence is NULL and the context keeps no packed reference");
        if ((size_t)n != M.ref_length.size() || !std::equal(M.ref_length.begin(), M.ref_length.end(), length))
            return fail(c, RSQC_ERR_ARG, "rsqc_mismatch_begin: sequence is NULL and the contigs differ from those of the packed reference");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    mismatch_drop(c, false);
    if (sequence) { if (int rc = pack_reference(c, n, length, sequence)) return rc; }
    const std::string sizes = std::to_string(TABLE_BYTES) + " bytes on the device and as many in page-locked host memory";
    if (int rc = window_tables(c, M, TABLE_BYTES, "rsqc_mismatch_begin: no device memory for the tables (" + sizes + ")",
                               "rsqc_mismatch_begin: no page-locked host memory for the tables (" + sizes + ")")) return rc;
    M.min_mapq = min_mapq;
    M.active = true;
    return RSQC_OK;
}

int rsqc_mismatch_add(rsqc_ctx *c, const uint64_t *cyc, const uint64_t *subst, const uint64_t *byq, const rsqc_mismatch_info *partial) {
    if (!c || !partial) return RSQC_ERR_ARG;
    MismatchState &M = c->mm;
    if (int rc = window_add_check(c, M, NAMES)) return rc;
    uint64_t col[MM_COLS] = {0, 0, 0, 0, 0, 0};
    if (cyc) for (size_t k = 0; k < MM_CYC_CELLS; ++k) col[k % MM_COLS] += cyc[k];
    if (col[MM_COMPARED] != partial->compared || col[MM_MISMATCH] != partial->mismatched || col[MM_UNCOMPARED] != partial->uncompared || col[MM_INSERTED] != partial->inserted ||
        col[MM_CLIPPED] != partial->clipped || col[MM_DELETIONS] != partial->deletions)
        return fail(c, RSQC_ERR_ARG, "rsqc_mismatch_add: compared .. deletions of partial are not the sums of the columns of cyc");
    uint64_t *a = window_added(M, MM_TABLE_WORDS), *s = a + AT_SCAL;
    if (cyc) for (size_t k = 0; k < MM_CYC_CELLS; ++k) a[k] += cyc[k];
    if (subst) for (size_t k = 0; k < MM_SUBST_CELLS; ++k) a[AT_SUBST + k] += subst[k];
    if (byq) for (size_t k = 0; k < MM_BYQ_CELLS; ++k) a[AT_BYQ + k] += byq[k];
    s[MM_S_RECORDS] += partial->records; s[MM_S_NO_REF] += partial->no_reference_records; s[MM_S_LOW_MAPQ] += partial->low_mapq_records;
    s[MM_S_NO_SEQ] += partial->no_seq_records; s[MM_S_INCONSISTENT] += partial->inconsistent_records; s[MM_S_NO_QUAL] += partial->no_qual_records;
    s[MM_S_INS_EVENTS] += partial->insertion_events; s[MM_S_DEL_EVENTS] += partial->deletion_events; s[MM_S_DEL_BASES] += partial->deleted_bases;
    s[MM_S_BEYOND] += partial->beyond_bases; s[MM_S_CLAMPED] += partial->clamped_quals;
    s[MM_S_LEN_SUM] += partial->compared + partial->uncompared + partial->inserted + partial->clipped + partial->beyond_bases;
    M.added_seen += partial->seen_records;
    return RSQC_OK;
}

int rsqc_mismatch_end(rsqc_ctx *c, rsqc_mismatch_info *out, const uint64_t **cyc, const uint64_t **subst, const uint64_t **byq) {
    if (!c || !out) return RSQC_ERR_ARG;
    MismatchState &M = c->mm;
    if (int rc = window_end(c, M, NAMES, TABLE_BYTES, mismatch_finish)) return rc;
    *out = M.info;
    const uint64_t *h = (const uint64_t *)M.h_tab.p;
    if (cyc) *cyc = h;
    if (subst) *subst = h + AT_SUBST;
    if (byq) *byq = h + AT_BYQ;
    return RSQC_OK;
}
