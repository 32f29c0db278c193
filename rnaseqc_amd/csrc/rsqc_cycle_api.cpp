// rsqc_cycle_api.cpp -- rsqc_cycles_begin / rsqc_cycles_add / rsqc_cycles_end: every window of the device decode leaves the counts of
// its records' SEQ and QUAL by read cycle in two device-resident tables (one extra kernel per window, rsqc_cycle.hip); at the end of the
// pass they are read back once, what the host added is summed in, and the tables are checked against the device's own sum of lengths.
#include "rsqc_ctx.h"
#include "rsqc_cycle.h"

namespace {

constexpr size_t TABLE_BYTES = (size_t)CYC_TABLE_WORDS * 8;

CycleTables device_tables(const CycleState &Y) {
    unsigned long long *p = (unsigned long long *)Y.tab.p;
    return CycleTables{p, p + CYC_BASE_CELLS, p + CYC_BASE_CELLS + CYC_QUAL_CELLS};
}

int cycles_end_run(rsqc_ctx *c) {
    CycleState &Y = c->cyc;
    uint64_t *h = (uint64_t *)Y.h_tab.p;
    HIP_TRY(c, hipMemcpyAsync(h, Y.tab.p, TABLE_BYTES, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    rsqc_cycle_info &I = Y.info;
    I = rsqc_cycle_info{};
    for (auto &pr : Y.events) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) I.cycles_ms += ms;
        c->event_pool.push_back(pr.first); c->event_pool.push_back(pr.second);
    }
    Y.events.clear();
    if (!Y.added.empty()) for (size_t k = 0; k < CYC_TABLE_WORDS; ++k) h[k] += Y.added[k];
    const uint64_t *base = h, *qual = h + CYC_BASE_CELLS, *s = qual + CYC_QUAL_CELLS;
    I.seen_records = Y.seen + Y.added_seen;
    I.records = s[CYC_S_RECORDS]; I.no_seq_records = s[CYC_S_NO_SEQ]; I.no_qual_records = s[CYC_S_NO_QUAL];
    I.beyond_bases = s[CYC_S_BEYOND]; I.clamped_quals = s[CYC_S_CLAMPED];
    for (uint32_t ec = 0; ec < CYC_ENDS * CYC_MAX; ++ec) {
        uint64_t nb = 0, nq = 0;
        for (uint32_t b = 0; b < CYC_BASES; ++b) nb += base[(size_t)ec * CYC_BASES + b];
        for (uint32_t q = 0; q < CYC_QBINS; ++q) nq += qual[(size_t)ec * CYC_QBINS + q];
        if (nq > nb)
            return fail(c, RSQC_ERR_HIP, "rsqc_cycles_end: end " + std::to_string(ec / CYC_MAX + 1) + " cycle " + std::to_string(ec % CYC_MAX + 1) + " holds " +
                                             std::to_string(nq) + " qualities for " + std::to_string(nb) + " bases");
        I.bases += nb;
    }
    if (I.bases + I.beyond_bases != s[CYC_S_LEN_SUM])
        return fail(c, RSQC_ERR_HIP, "rsqc_cycles_end: the tables hold " + std::to_string(I.bases) + " bases and " + std::to_string(I.beyond_bases) +
                                         " lie beyond them, the records' lengths add up to " + std::to_string(s[CYC_S_LEN_SUM]));
    return 0;
}

}  // namespace

namespace rsqc {

void cycle_drop(rsqc_ctx *c, bool free_buffers) {
    CycleState &Y = c->cyc;
    for (auto &pr : Y.events) { c->event_pool.push_back(pr.first); c->event_pool.push_back(pr.second); }
    Y.events.clear();
    Y.active = Y.done = false;
    Y.seen = Y.added_seen = 0;
    Y.added.clear();
    Y.info = rsqc_cycle_info{};
    if (free_buffers) { Y.tab.release(); Y.h_tab.release(); }
}

// called by the decode for every window it enqueues, behind the window's parse stage
int cycle_window(rsqc_ctx *c, const DecodeWindow &W, const SamWindow *S) {
    CycleState &Y = c->cyc;
    hipEvent_t e0 = get_event(c), e1 = get_event(c);
    Y.events.emplace_back(e0, e1);
    HIP_TRY(c, hipEventRecord(e0, c->stream));
    if (S) launch_cycle_sam(c->stream, *S, device_tables(Y));
    else launch_cycle_bam(c->stream, W, device_tables(Y));
    HIP_TRY(c, hipEventRecord(e1, c->stream));
    return 0;
}

}  // namespace rsqc

int rsqc_cycles_begin(rsqc_ctx *c) {
    if (!c) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    if (c->finalized) return fail(c, RSQC_ERR_ARG, "rsqc_reset required after rsqc_finalize");
    if (c->cyc.active) return fail(c, RSQC_ERR_ARG, "rsqc_cycles_begin: the context is counting cycles already");
    if (c->dec.active || c->name_mode >= 0 || !c->batch_file_index.empty() || c->next_record_base)
        return fail(c, RSQC_ERR_ARG, "rsqc_cycles_begin must precede the first submit and the rsqc_decode_begin of the pass");
    HIP_TRY(c, hipSetDevice(c->device));
    cycle_drop(c, false);
    CycleState &Y = c->cyc;
    const std::string sizes = std::to_string(TABLE_BYTES) + " bytes on the device and as many in page-locked host memory";
    if (!dev_reserve(Y.tab, TABLE_BYTES)) return fail(c, RSQC_ERR_CAPACITY, "rsqc_cycles_begin: no device memory for the tables (" + sizes + ")");
    if (!host_reserve(Y.h_tab, TABLE_BYTES)) return fail(c, RSQC_ERR_CAPACITY, "rsqc_cycles_begin: no page-locked host memory for the tables (" + sizes + ")");
    HIP_TRY(c, hipMemsetAsync(Y.tab.p, 0, TABLE_BYTES, c->stream));
    Y.active = true;
    return RSQC_OK;
}

int rsqc_cycles_add(rsqc_ctx *c, const uint64_t *base, const uint64_t *qual, const rsqc_cycle_info *partial) {
    if (!c || !partial) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    CycleState &Y = c->cyc;
    if (!Y.active) return fail(c, RSQC_ERR_ARG, "rsqc_cycles_begin must precede rsqc_cycles_add");
    if (Y.done) return fail(c, RSQC_ERR_ARG, "rsqc_cycles_add behind rsqc_cycles_end");
    uint64_t nb = 0;
    if (base) for (size_t k = 0; k < CYC_BASE_CELLS; ++k) nb += base[k];
    if (nb != partial->bases) return fail(c, RSQC_ERR_ARG, "rsqc_cycles_add: partial->bases is not the sum of the base table");
    if (Y.added.empty()) Y.added.assign(CYC_TABLE_WORDS, 0);
    uint64_t *a = Y.added.data(), *s = a + CYC_BASE_CELLS + CYC_QUAL_CELLS;
    if (base) for (size_t k = 0; k < CYC_BASE_CELLS; ++k) a[k] += base[k];
    if (qual) for (size_t k = 0; k < CYC_QUAL_CELLS; ++k) a[CYC_BASE_CELLS + k] += qual[k];
    s[CYC_S_RECORDS] += partial->records; s[CYC_S_NO_SEQ] += partial->no_seq_records; s[CYC_S_NO_QUAL] += partial->no_qual_records;
    s[CYC_S_BEYOND] += partial->beyond_bases; s[CYC_S_CLAMPED] += partial->clamped_quals;
    s[CYC_S_LEN_SUM] += partial->bases + partial->beyond_bases;
    Y.added_seen += partial->seen_records;
    return RSQC_OK;
}

int rsqc_cycles_end(rsqc_ctx *c, rsqc_cycle_info *out, const uint64_t **base, const uint64_t **qual) {
    if (!c || !out) return RSQC_ERR_ARG;
    if (c->sticky) return c->sticky;
    CycleState &Y = c->cyc;
    if (!Y.active) return fail(c, RSQC_ERR_ARG, "rsqc_cycles_begin must precede rsqc_cycles_end");
    if (c->dec.active) return fail(c, RSQC_ERR_ARG, "rsqc_decode_end must precede rsqc_cycles_end");
    if (!Y.done) {
        HIP_TRY(c, hipSetDevice(c->device));
        const int rc = cycles_end_run(c);
        if (rc) { (void)hipStreamSynchronize(c->stream); c->sticky = rc; return rc; }       // never partial tables: the pass is void until rsqc_reset
        Y.done = true;
    }
    *out = Y.info;
    const uint64_t *h = (const uint64_t *)Y.h_tab.p;
    if (base) *base = h;
    if (qual) *qual = h + CYC_BASE_CELLS;
    return RSQC_OK;
}
