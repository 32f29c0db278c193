// gc_emu.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// The KERNELS of --fasta -- rnaseqc_amd/csrc/rsqc_gc.h (gc_pack_kernel, exon_gc_kernel, gc_candidates_kernel), the G/C bit helpers
// of rsqc_device.h (gc_count, gc_value) and the mate pairing of rsqc_k5.h (pair_bucket_*, gc_replay_kernel, gc_replay_big_kernel),
// unmodified -- compiled for the host on top of the 64-lane fiber emulation of wavemu.h.  The host side that strings them together
// is restated here with plain memory:
//   rsqc_set_reference (rsqc_api.cpp): the loop that lays out word_off / length / words, the bit array of words + 2, ONE staging
//       buffer of longest + 64 bytes that every contig passes through (never cleared in between), launch_gc_pack per contig with
//       a non-zero length, then launch_exon_gc (grids as the launchers of rsqc_kernels.hip compute them);
//   rsqc_submit (rsqc_submit.cpp): launch_gc_candidates per batch into a list of the batch's own, capacity = its records;
//   rsqc_finalize (rsqc_finalize.cpp): the batches' lists appended in submission order;
//   run_gc_content / partition_by_name (rsqc_fragsize.hip): max(1, n / PB_MEAN) buckets, count / scan / scatter, gc_replay_kernel on
//       one workgroup per bucket, gc_replay_big_kernel on 64 workgroups of 1024, scratch of 2 n + 16 indices.
// Device memory the product does not clear (hipMalloc) is filled with poison here.  Nothing is EXPECTED here: tests/gc_ref.py and
// the oracle say what must come out, the tests compare.
#include "wavemu.h"

#include <algorithm>
#include <string>
#include <vector>

#include "../../rnaseqc_amd/csrc/rsqc_read.h"
#include "../../rnaseqc_amd/csrc/rsqc_device.h"
#include "../../rnaseqc_amd/csrc/rsqc_index.h"
#include "../../rnaseqc_amd/csrc/rsqc_wave.h"
#include "../../rnaseqc_amd/csrc/rsqc_k1s.h"
#include "../../rnaseqc_amd/csrc/rsqc_gc.h"
#include "../../rnaseqc_amd/csrc/rsqc_k5.h"

using namespace rsqc;

namespace {
template <class F> void launch(uint32_t grid, int threads, F &&body) {
    wavemu::grid_dim().x = grid;
    for (uint32_t b = 0; b < grid; ++b) { wavemu::block_idx().x = b; wavemu::run_block(threads, body); }
}

constexpr unsigned long long kPoison64 = 0xA5A5A5A5A5A5A5A5ull;

// the device annotation as rsqc_set_annotation builds it (the pieces the --fasta kernels read)
struct Ann {
    HostIndex hx; std::vector<EiRank> rank; std::vector<uint32_t> ex_id, zero_range; DevAnnotation d{};
    int build(const rsqc_annotation *a) {
        std::string err;
        const int rc = hx.build(a, nullptr, err);
        if (rc) return rc;
        d.n_ref = a->n_ref; d.n_contigs = a->n_contigs; d.n_genes = a->n_genes; d.n_listed = a->n_genes_listed; d.n_exons = a->n_exons;
        d.bin_shift = HostIndex::kBinShift;
        d.contig = hx.contig.data();
        if (hx.ex_rows.empty()) hx.ex_rows.push_back(ExonRow{0, 0, 0, 0});
        if (hx.gb.empty()) hx.gb.push_back(GeneBreak{0, 0});
        if (hx.ex_pmax.empty()) hx.ex_pmax.push_back(0);
        d.ex = hx.ex_rows.data(); d.gb = hx.gb.data(); d.ex_pmax = hx.ex_pmax.data();
        d.ex_binhi = hx.ex_binhi.data(); d.gb_bin = hx.gb_bin.data(); d.ex_cov = hx.ex_cov.data();
        hx.build_rank(rank);
        d.ei = hx.ei.data(); d.ei_rank = rank.data(); d.ei_coarse = hx.ei_coarse.data();
        ex_id.assign(a->exon_row_id, a->exon_row_id + a->n_exons); if (ex_id.empty()) ex_id.push_back(0);
        d.ex_id = ex_id.data();
        zero_range.assign((size_t)a->n_contigs + 1, 0);
        d.bed_range = zero_range.data(); d.have_bed = 0;
        return 0;
    }
};

struct State {
    std::vector<unsigned long long> bits, off, len;                                   // the packed reference (DevReference)
    std::vector<uint64_t> file, q; std::vector<uint32_t> h2, row, fl; std::vector<int32_t> end, tid;   // the candidate list of the last run
    DevReference ref() const { return DevReference{bits.data(), off.data(), len.data()}; }
} S;
}  // namespace

#define EMU_API extern "C" __attribute__((visibility("default")))

EMU_API void gcemu_set_schedule_seed(unsigned long long seed) { wavemu::set_seed(seed); }

// words of the bit array for `ref` (what rsqc_set_reference sums up): the caller sizes `words_out` with it
EMU_API uint64_t gcemu_reference_words(const rsqc_reference *ref) {
    uint64_t words = 0;
    for (int i = 0; i < ref->n; ++i) words += (ref->length[i] + 63) / 64;
    return words;
}

// rsqc_set_reference.  Out: the packed words, word_off / length per contig of the annotation, exon_gc by exon id.  Returns 0, an
// RSQC_ERR_* code, or 2000 + k for check k of the harness itself (a write outside the arrays).  The packed reference stays for gcemu_run.
EMU_API int gcemu_reference(const rsqc_annotation *a, const rsqc_reference *ref, unsigned long long *words_out, unsigned long long *word_off,
                            unsigned long long *length, double *exon_gc) {
    Ann A;
    int rc = A.build(a);
    if (rc) return rc;
    const int nc = a->n_contigs;
    S = State{};
    S.off.assign((size_t)std::max(nc, 1), ~0ull); S.len.assign((size_t)std::max(nc, 1), 0ull);
    unsigned long long words = 0, longest = 0;
    for (int i = 0; i < ref->n; ++i) {
        const int k = ref->contig[i];
        if (k < 0 || k >= nc || S.off[(size_t)k] != ~0ull) return RSQC_ERR_ARG;
        if (ref->length[i] && !ref->sequence[i]) return RSQC_ERR_ARG;
        S.off[(size_t)k] = words; S.len[(size_t)k] = ref->length[i];
        words += (ref->length[i] + 63) / 64;
        longest = std::max<unsigned long long>(longest, ref->length[i]);
    }
    S.bits.assign((size_t)words + 2, kPoison64);
    std::vector<uint8_t> stage((size_t)longest + 64, (uint8_t)'G');                   // (poison that would count: a read behind a contig's bases shows)
    for (int i = 0; i < ref->n; ++i) {
        if (!ref->length[i]) continue;
        memcpy(stage.data(), ref->sequence[i], (size_t)ref->length[i]);
        const uint64_t n_words = (ref->length[i] + 63) / 64;
        unsigned long long *dst = S.bits.data() + S.off[(size_t)ref->contig[i]];
        const uint64_t len = ref->length[i];
        launch((uint32_t)std::min<uint64_t>((n_words + 255) / 256, 65536), 256, [&]() { gc_pack_kernel(stage.data(), len, dst); });
    }
    if (S.bits[(size_t)words] != kPoison64 || S.bits[(size_t)words + 1] != kPoison64) return 2001;
    std::vector<double> gc((size_t)std::max(a->n_exons, 1) + 1, -7.0);
    if (a->n_exons > 0) launch((uint32_t)((a->n_exons + 255) / 256), 256, [&]() { exon_gc_kernel(A.d, S.ref(), gc.data()); });
    if (gc[(size_t)std::max(a->n_exons, 1)] != -7.0) return 2002;
    for (unsigned long long w = 0; w < words; ++w) words_out[w] = S.bits[(size_t)w];
    for (int k = 0; k < nc; ++k) { word_off[k] = S.off[(size_t)k]; length[k] = S.len[(size_t)k]; }
    for (int e = 0; e < a->n_exons; ++e) exon_gc[e] = gc[(size_t)e];
    return 0;
}

// The chain behind the reference of the last gcemu_reference call.  n_batches > 0: gc_candidates_kernel per batch; else the n_direct
// candidates of the columns d_* as they are (crafted names, hashes and file orders).  Then the pairing and both replay kernels.
// bins: [RSQC_GC_BINS + 1].  stats: [0] candidates, [1] buckets paired through the set, [2] buckets sorted in LDS, [3] buckets listed as
// oversize, [4] the device error word, [5] buckets.  Returns 0, an RSQC_ERR_* code of the harness's own set-up, or 2000 + k.
EMU_API int gcemu_run(const rsqc_params *p, const rsqc_annotation *a, const rsqc_batch *const *batches, int n_batches,
                      uint32_t n_direct, const uint64_t *d_file, const uint64_t *d_q, const uint32_t *d_h2, const uint32_t *d_row, const int32_t *d_end,
                      const uint32_t *d_fl, const int32_t *d_tid, unsigned long long *bins, uint64_t *stats) {
    S.file.clear(); S.q.clear(); S.h2.clear(); S.row.clear(); S.fl.clear(); S.end.clear(); S.tid.clear();
    int error = 0;
    const DevReference R = S.ref();
    if (n_batches > 0) {
        Ann A;
        int rc = A.build(a);
        if (rc) return rc;
        if ((int)S.off.size() < a->n_contigs) return RSQC_ERR_ARG;
        DevParams dp{p->mapq_threshold, p->base_mismatch, p->chimeric_distance, p->stranded, p->unpaired, p->exclude_chimeric, p->n_filter_tags, p->legacy};
        for (int k = 0; k < n_batches; ++k) {
            const rsqc_batch *b = batches[k];
            const uint64_t n = b->n;
            if (!n) continue;                                                          // (launch_gc_candidates)
            // the batch with the slack the device buffers carry
            std::vector<rsqc_rec_core> core((size_t)n + 2); std::vector<rsqc_rec_aux> aux((size_t)n + 2);
            std::vector<uint32_t> cigar((size_t)b->n_cigar_total + 8, 0u), qh2((size_t)n + 2, 0u);
            memcpy(core.data(), b->core, (size_t)n * sizeof(rsqc_rec_core)); memcpy(aux.data(), b->aux, (size_t)n * sizeof(rsqc_rec_aux));
            if (b->n_cigar_total) memcpy(cigar.data(), b->cigar, (size_t)b->n_cigar_total * 4);
            if (b->qhash2) memcpy(qh2.data(), b->qhash2, (size_t)n * 4);
            DevBatch db{};
            db.qhash2 = b->qhash2 ? qh2.data() : nullptr;
            db.n = n; db.record_base = b->file_index_base; db.core = core.data(); db.aux = aux.data(); db.cigar = cigar.data();
            db.n_seg = b->n_seg; db.seg_tid = b->seg_tid; db.seg_start = b->seg_start; db.seg_file_index = b->seg_file_index;
            db.n_wide = b->n_wide; db.wide_index = b->wide_index; db.wide_nm = b->wide_nm; db.wide_l_qseq = b->wide_l_qseq; db.wide_n_cigar = b->wide_n_cigar;
            const uint32_t cap = (uint32_t)n;
            std::vector<uint64_t> file((size_t)cap + 1, kPoison64), q((size_t)cap + 1, kPoison64);
            std::vector<uint32_t> row((size_t)cap + 1, 0xA5A5A5A5u), fl((size_t)cap + 1, 0xA5A5A5A5u), h2((size_t)cap + 1, 0xA5A5A5A5u);
            std::vector<int32_t> end((size_t)cap + 1, (int32_t)0xA5A5A5A5u), tid((size_t)cap + 1, (int32_t)0xA5A5A5A5u);
            uint32_t count = 0;
            GcCandidates gc{file.data(), q.data(), row.data(), end.data(), fl.data(), tid.data(), &count, cap, h2.data()};
            const uint64_t blocks = (n + GC_CAND_THREADS - 1) / GC_CAND_THREADS;
            launch((uint32_t)std::min<uint64_t>(blocks, 4096), GC_CAND_THREADS, [&]() { gc_candidates_kernel(A.d, dp, db, R, gc, &error); });
            if (error) { stats[4] = (uint64_t)(int64_t)error; return 0; }
            if (count > cap) return 2003;
            if (file[cap] != kPoison64 || q[cap] != kPoison64 || row[cap] != 0xA5A5A5A5u || fl[cap] != 0xA5A5A5A5u || h2[cap] != 0xA5A5A5A5u) return 2004;
            for (uint32_t j = 0; j < count; ++j) {
                S.file.push_back(file[j]); S.q.push_back(q[j]); S.h2.push_back(h2[j]); S.row.push_back(row[j]); S.fl.push_back(fl[j]);
                S.end.push_back(end[j]); S.tid.push_back(tid[j]);
            }
        }
    } else {
        S.file.assign(d_file, d_file + n_direct); S.q.assign(d_q, d_q + n_direct); S.h2.assign(d_h2, d_h2 + n_direct); S.row.assign(d_row, d_row + n_direct);
        S.fl.assign(d_fl, d_fl + n_direct); S.end.assign(d_end, d_end + n_direct); S.tid.assign(d_tid, d_tid + n_direct);
    }
    const uint32_t n = (uint32_t)S.file.size();
    for (int i = 0; i <= RSQC_GC_BINS; ++i) bins[i] = 0ull;
    for (int i = 0; i < 6; ++i) stats[i] = 0;
    stats[0] = n;
    g_k5_hashed_buckets = 0; g_k5_sorted_buckets = 0;
    if (n == 0) return 0;                                                              // (run_gc_content)
    const GcCandidates c{S.file.data(), S.q.data(), S.row.data(), S.end.data(), S.fl.data(), S.tid.data(), nullptr, n, S.h2.data()};
    const uint32_t nb = k5_bucket_count(n);                                             // (rsqc_k5_plan.h: the library's own rule)
    std::vector<uint32_t> count(nb + 1, 0u), off(nb + 1, 0xDEADu), cursor(nb + 1, 0xDEADu), perm((size_t)n + 1, 0xFFFFFFFFu), big_list(PB_BIG_MAX + 1, 0xDEADu),
        big_idx(2 * (size_t)n + 16, 0xDEADu);
    big_list[0] = 0u;
    const uint32_t G = k5_part_grid(n);
    launch(G, 256, [&]() { pair_bucket_count_kernel(c.qhash, n, nb, count.data()); });
    launch(1, 1024, [&]() { pair_bucket_scan_kernel(count.data(), nb, off.data(), cursor.data(), big_list.data(), &error); });
    launch(G, 256, [&]() { pair_bucket_scatter_kernel(c.qhash, n, nb, cursor.data(), perm.data()); });
    if (off[nb] != n || perm[n] != 0xFFFFFFFFu) return 2005;
    std::vector<unsigned long long> dbins((size_t)RSQC_GC_BINS + 2, 0ull);
    dbins[(size_t)RSQC_GC_BINS + 1] = kPoison64;
    launch(nb, PB_THREADS, [&]() { gc_replay_kernel(c, off.data(), perm.data(), R, dbins.data()); });
    launch(K5_BIG_GRID, 1024, [&]() { gc_replay_big_kernel(c, off.data(), perm.data(), big_list.data(), big_idx.data(), R, dbins.data()); });
    if (dbins[(size_t)RSQC_GC_BINS + 1] != kPoison64) return 2006;
    for (int i = 0; i <= RSQC_GC_BINS; ++i) bins[i] = dbins[(size_t)i];
    stats[1] = g_k5_hashed_buckets; stats[2] = g_k5_sorted_buckets; stats[3] = big_list[0]; stats[4] = (uint64_t)(int64_t)error; stats[5] = nb;
    return 0;
}

// the candidate list of the last gcemu_run (stats[0] entries per column), in list order
EMU_API void gcemu_candidates(uint64_t *file, uint64_t *q, uint32_t *h2, uint32_t *row, int32_t *end, uint32_t *fl, int32_t *tid) {
    for (size_t k = 0; k < S.file.size(); ++k) { file[k] = S.file[k]; q[k] = S.q[k]; h2[k] = S.h2[k]; row[k] = S.row[k]; end[k] = S.end[k]; fl[k] = S.fl[k]; tid[k] = S.tid[k]; }
}
