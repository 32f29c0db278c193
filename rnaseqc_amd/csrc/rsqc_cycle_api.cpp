// rsqc_cycle_api.cpp -- rsqc_cycles_begin / rsqc_cycles_add / rsqc_cycles_end: the counts of the records' SEQ and QUAL by read cycle in two
// tables (the kernel of rsqc_cycle.hip behind every window), checked at the end against the device's own sum of lengths.  What the stage
// shares with the other two behind a window is in rsqc_window_stage_api.cpp.
#include "rsqc_ctx.h"
#include "rsqc_cycle.h"

namespace {

constexpr size_t TABLE_BYTES = (size_t)CYC_TABLE_WORDS * 8;
constexpr WindowNames NAMES{"rsqc_cycles_begin", "rsqc_cycles_add", "rsqc_cycles_end", "cycles"};

CycleTables device_tables(const CycleState &Y) {
    unsigned long long *p = (unsigned long long *)Y.tab.p;
    return CycleTables{p, p + CYC_BASE_CELLS, p + CYC_BASE_CELLS + CYC_QUAL_CELLS};
}

int cycles_finish(rsqc_ctx *c, double ms) {
    CycleState &Y = c->cyc;
    uint64_t *h = (uint64_t *)Y.h_tab.p;
    rsqc_cycle_info &I = Y.info;
    I = rsqc_cycle_info{};
    I.cycles_ms = ms;
    window_sum_added(Y, h, CYC_TABLE_WORDS);
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

void cycle_drop(rsqc_ctx *c, bool free_buffers) { window_drop(c, c->cyc, free_buffers); }

void cycle_launch(rsqc_ctx *c, const DecodeWindow &W, const SamWindow *S) {
    if (S) launch_cycle_sam(c->stream, *S, device_tables(c->cyc));
    else launch_cycle_bam(c->stream, W, device_tables(c->cyc));
}

}  // namespace rsqc

int rsqc_cycles_begin(rsqc_ctx *c) {
    if (!c) return RSQC_ERR_ARG;
    if (int rc = window_begin_check(c, c->cyc, NAMES)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    cycle_drop(c, false);
    const std::string sizes = std::to_string(TABLE_BYTES) + " bytes on the device and as many in page-locked host memory";
    if (int rc = window_tables(c, c->cyc, TABLE_BYTES, "rsqc_cycles_begin: no device memory for the tables (" + sizes + ")",
                               "rsqc_cycles_begin: no page-locked host memory for the tables (" + sizes + ")")) return rc;
    c->cyc.active = true;
    return RSQC_OK;
}

int rsqc_cycles_add(rsqc_ctx *c, const uint64_t *base, const uint64_t *qual, const rsqc_cycle_info *partial) {
    if (!c || !partial) return RSQC_ERR_ARG;
    CycleState &Y = c->cyc;
    if (int rc = window_add_check(c, Y, NAMES)) return rc;
    uint64_t nb = 0;
    if (base) for (size_t k = 0; k < CYC_BASE_CELLS; ++k) nb += base[k];
    if (nb != partial->bases) return fail(c, RSQC_ERR_ARG, "rsqc_cycles_add: partial->bases is not the sum of the base table");
    uint64_t *a = window_added(Y, CYC_TABLE_WORDS), *s = a + CYC_BASE_CELLS + CYC_QUAL_CELLS;
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
    CycleState &Y = c->cyc;
    if (int rc = window_end(c, Y, NAMES, TABLE_BYTES, cycles_finish)) return rc;
    *out = Y.info;
    const uint64_t *h = (const uint64_t *)Y.h_tab.p;
    if (base) *base = h;
    if (qual) *qual = h + CYC_BASE_CELLS;
    return RSQC_OK;
}
