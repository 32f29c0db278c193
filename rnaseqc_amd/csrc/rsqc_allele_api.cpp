// rsqc_allele_api.cpp -- rsqc_alleles_begin / rsqc_alleles_add / rsqc_alleles_end: the sorted site list goes to the device at every begin
// (a position per site, a first site per contig); the bases the records show at those sites (the kernel of rsqc_allele.hip behind every
// window) in cells [site][8], compacted to [site][7] at the end and checked against the device's own count of its observations.  What
// the stage shares with the other two behind a window is in rsqc_window_stage_api.cpp.
#include "rsqc_ctx.h"
#include "rsqc_allele.h"

namespace {

constexpr WindowNames NAMES{"rsqc_alleles_begin", "rsqc_alleles_add", "rsqc_alleles_end", "alleles"};

size_t device_words(uint32_t n_sites) { return (size_t)AL_S_WORDS + (size_t)n_sites * AL_STRIDE; }
size_t table_words(uint32_t n_sites) { return (size_t)AL_S_WORDS + (size_t)n_sites * AL_COLS; }

AlleleTables device_tables(const AlleleState &A) {
    unsigned long long *p = (unsigned long long *)A.tab.p;
    return AlleleTables{p, p + AL_S_WORDS};
}
AlleleSites device_sites(const AlleleState &A) { return AlleleSites{(const int32_t *)A.pos.p, (const uint32_t *)A.first.p, A.n_contigs}; }

int alleles_finish(rsqc_ctx *c, double ms) {
    AlleleState &A = c->al;
    uint64_t *h = (uint64_t *)A.h_tab.p;
    rsqc_allele_info &I = A.info;
    I = rsqc_allele_info{};
    I.alleles_ms = ms;
    // [site][8] -> [site][7], in place and forwards (7 k + col <= 8 k + col)
    uint64_t *cells = h + AL_S_WORDS;
    for (size_t k = 1; k < A.n_sites; ++k) for (uint32_t col = 0; col < AL_COLS; ++col) cells[k * AL_COLS + col] = cells[k * AL_STRIDE + col];
    window_sum_added(A, h, table_words(A.n_sites));
    const uint64_t *s = h;
    I.seen_records = A.seen + A.added_seen;
    I.records = s[AL_S_RECORDS]; I.off_contig_records = s[AL_S_OFF_CONTIG]; I.low_mapq_records = s[AL_S_LOW_MAPQ]; I.no_seq_records = s[AL_S_NO_SEQ];
    I.inconsistent_records = s[AL_S_INCONSISTENT]; I.no_qual_records = s[AL_S_NO_QUAL]; I.hit_records = s[AL_S_HIT]; I.observations = s[AL_S_OBS];
    I.n_sites = A.n_sites;
    uint64_t sum = 0;
    for (size_t k = 0; k < (size_t)A.n_sites * AL_COLS; ++k) sum += cells[k];
    if (sum != I.observations)
        return fail(c, RSQC_ERR_HIP, "rsqc_alleles_end: the table holds " + std::to_string(sum) + " observations, the records made " + std::to_string(I.observations));
    if (I.hit_records > I.records)
        return fail(c, RSQC_ERR_HIP, "rsqc_alleles_end: " + std::to_string(I.hit_records) + " records with an observation among " + std::to_string(I.records));
    return 0;
}

}  // namespace

namespace rsqc {

void alleles_drop(rsqc_ctx *c, bool free_buffers) {
    AlleleState &A = c->al;
    window_drop(c, A, free_buffers);
    A.n_sites = 0; A.n_contigs = 0;
    if (free_buffers) { A.pos.release(); A.first.release(); }
}

void alleles_launch(rsqc_ctx *c, const DecodeWindow &W, const SamWindow *S) {
    const AlleleState &A = c->al;
    if (S) launch_allele_sam(c->stream, *S, device_sites(A), A.min_mapq, A.min_baseq, device_tables(A), A.merge);
    else launch_allele_bam(c->stream, W, device_sites(A), A.min_mapq, A.min_baseq, device_tables(A), A.merge);
}

}  // namespace rsqc

int rsqc_alleles_begin(rsqc_ctx *c, int32_t n_contigs, uint32_t n_sites, const int32_t *tid, const int32_t *pos, uint32_t min_mapq, uint32_t min_baseq) {
    if (!c) return RSQC_ERR_ARG;
    AlleleState &A = c->al;
    if (int rc = window_begin_check(c, A, NAMES)) return rc;
    if (n_contigs < 0 || (n_sites > 0 && (!tid || !pos))) return fail(c, RSQC_ERR_ARG, "rsqc_alleles_begin: sites without tid or pos");
    if (min_mapq > 255u) return fail(c, RSQC_ERR_ARG, "rsqc_alleles_begin: min_mapq above 255");
    if (min_baseq > 93u) return fail(c, RSQC_ERR_ARG, "rsqc_alleles_begin: min_baseq above 93");
    std::vector<uint32_t> first((size_t)n_contigs + 1, 0);
    for (uint32_t k = 0; k < n_sites; ++k) {
        if (tid[k] < 0 || tid[k] >= n_contigs)
            return fail(c, RSQC_ERR_ARG, "rsqc_alleles_begin: site " + std::to_string(k) + " has tid " + std::to_string(tid[k]) + " outside the " + std::to_string(n_contigs) + " contigs");
        if (pos[k] < 0 || pos[k] == INT32_MAX) return fail(c, RSQC_ERR_ARG, "rsqc_alleles_begin: site " + std::to_string(k) + " has pos " + std::to_string(pos[k]) + " outside [0, 2^31 - 1)");
        if (k && (tid[k] < tid[k - 1] || (tid[k] == tid[k - 1] && pos[k] <= pos[k - 1])))
            return fail(c, RSQC_ERR_ARG, "rsqc_alleles_begin: site " + std::to_string(k) + " is not behind site " + std::to_string(k - 1) + ": the list is strictly ascending by (tid, pos)");
        first[(size_t)tid[k] + 1] += 1;
    }
    for (int32_t t = 0; t < n_contigs; ++t) first[(size_t)t + 1] += first[(size_t)t];
    HIP_TRY(c, hipSetDevice(c->device));
    alleles_drop(c, false);
    const size_t tab_bytes = device_words(n_sites) * 8;
    const std::string sizes = std::to_string((size_t)n_sites * 4) + " bytes for the positions, " + std::to_string(((size_t)n_contigs + 1) * 4) + " for the contigs, " +
                              std::to_string(tab_bytes) + " for the cells and as many in page-locked host memory";
    const std::string no_device = "rsqc_alleles_begin: no device memory for the sites (" + sizes + ")";      // (the positions, the contigs and the cells under one text)
    if (!dev_reserve(A.pos, (size_t)std::max(n_sites, 1u) * 4) || !dev_reserve(A.first, ((size_t)n_contigs + 1) * 4)) return fail(c, RSQC_ERR_CAPACITY, no_device);
    if (int rc = window_tables(c, A, tab_bytes, no_device, "rsqc_alleles_begin: no page-locked host memory for the table (" + sizes + ")")) return rc;
    if (n_sites) HIP_TRY(c, hipMemcpyAsync(A.pos.p, pos, (size_t)n_sites * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(A.first.p, first.data(), first.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));                      // (the caller's arrays and `first` are read until here)
    A.n_contigs = n_contigs; A.n_sites = n_sites; A.min_mapq = min_mapq; A.min_baseq = min_baseq;
    const char *m = getenv("RSQC_ALLELE_MERGE");       // 0: an atomic per observation; 1: merged across the wave first (the table is the same)
    A.merge = m ? atoi(m) != 0 : RSQC_ALLELE_MERGE_DEFAULT;
    A.active = true;
    return RSQC_OK;
}

int rsqc_alleles_add(rsqc_ctx *c, const uint64_t *counts, const rsqc_allele_info *partial) {
    if (!c || !partial) return RSQC_ERR_ARG;
    AlleleState &A = c->al;
    if (int rc = window_add_check(c, A, NAMES)) return rc;
    const size_t n_cells = (size_t)A.n_sites * AL_COLS;
    uint64_t sum = 0;
    if (counts) for (size_t k = 0; k < n_cells; ++k) sum += counts[k];
    if (sum != partial->observations)
        return fail(c, RSQC_ERR_ARG, "rsqc_alleles_add: counts add up to " + std::to_string(sum) + ", partial->observations is " + std::to_string(partial->observations));
    uint64_t *s = window_added(A, table_words(A.n_sites)), *a = s + AL_S_WORDS;
    if (counts) for (size_t k = 0; k < n_cells; ++k) a[k] += counts[k];
    s[AL_S_RECORDS] += partial->records; s[AL_S_OFF_CONTIG] += partial->off_contig_records; s[AL_S_LOW_MAPQ] += partial->low_mapq_records;
    s[AL_S_NO_SEQ] += partial->no_seq_records; s[AL_S_INCONSISTENT] += partial->inconsistent_records; s[AL_S_NO_QUAL] += partial->no_qual_records;
    s[AL_S_HIT] += partial->hit_records; s[AL_S_OBS] += partial->observations;
    A.added_seen += partial->seen_records;
    return RSQC_OK;
}

int rsqc_alleles_end(rsqc_ctx *c, rsqc_allele_info *out, const uint64_t **counts) {
    if (!c || !out) return RSQC_ERR_ARG;
    AlleleState &A = c->al;
    if (int rc = window_end(c, A, NAMES, device_words(A.n_sites) * 8, alleles_finish)) return rc;
    *out = A.info;
    if (counts) *counts = (const uint64_t *)A.h_tab.p + AL_S_WORDS;
    return RSQC_OK;
}
