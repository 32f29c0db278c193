// k1_emu.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// The per-record KERNELS themselves -- rnaseqc_amd/csrc/rsqc_k1.h (classify_ei_kernel), rsqc_k1s.h (classify_slow_kernel) and
// rsqc_kr.h (read_length_kernel) with the wave helpers of rsqc_wave.h, unmodified -- compiled for the host on top of the
// 64-lane fiber emulation of wavemu.h: per-wave LDS queues, ballot / mbcnt compaction, workgroup LDS tables, pair chunks, the
// overflow list and the general kernel that takes it, the Read-Length transfer function.  hostemu.cpp covers the per-record
// functions one record at a time; this covers what the wavefronts do with them.  `slow_kernel` = 0 sends the overflow list
// through the general per-record code on the host instead of classify_slow_kernel (the two must agree).
#include "wavemu.h"

#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../rnaseqc_amd/csrc/rsqc_read.h"
#include "../../rnaseqc_amd/csrc/rsqc_device.h"
#include "../../rnaseqc_amd/csrc/rsqc_index.h"
#include "../../rnaseqc_amd/csrc/rsqc_wave.h"
#include "../../rnaseqc_amd/csrc/rsqc_k1.h"
#include "../../rnaseqc_amd/csrc/rsqc_k1s.h"
#include "../../rnaseqc_amd/csrc/rsqc_kr.h"
#include "../../rnaseqc_amd/csrc/rsqc_rl_compose.h"
#define RSQC_FIN_STAMP(sec)
#define RSQC_FIN_SECT(base, sec)
#define RSQC_FIN_BEGIN
#include "../../rnaseqc_amd/csrc/rsqc_k4.h"

using namespace rsqc;

namespace {
struct SlowAccH {
    std::vector<uint64_t> *reads, *unique;
    std::vector<double> *exon_rows;
    std::vector<uint32_t> *cov;
    std::vector<std::set<std::pair<uint64_t, uint32_t>>> *names;          // a name = (64-bit hash, second hash)
    void gene_hit(uint32_t g, bool nd, uint64_t qh, uint32_t qh2) { (*reads)[g]++; if (nd) (*unique)[g]++; (*names)[g].insert({qh, qh2}); }
    void exon_add(uint32_t row, double f) { (*exon_rows)[row] += f; }
    void cov_range(uint32_t cidx, uint32_t len) { if (!len) return; (*cov)[cidx] += 1u; (*cov)[cidx + len] -= 1u; }
};
}  // namespace

// ---- KR under test (k1emu_run_kr below): what the Read-Length part of k1emu_run_bed takes from and hands to the caller.  Without a
// request (every other entry point) that part runs as it always did: state 0 in, no rl_seg, one block, the final state checked.
namespace {
struct KrRequest {
    uint32_t r_in;            // the context's state when the batch arrives (plain batches; a batch of ranges is composed from 0)
    int ranges;               // the batch is several file ranges (rsqc_batch.seg_file_index): rl_seg armed as rsqc_submit.cpp arms it, a block per segment
    uint32_t *tile_span;      // [(n + 63) / 64] out
    uint32_t *extremes;       // [3 * entries] out: rl_stats (plain) or rl_seg (ranges) as the per-record kernels left them
    uint32_t *summary;        // [(entries + 1) * RSQC_RL_SUMMARY_WORDS] in / out: the caller's poison in, the slots out (one guard slot behind)
    int32_t state;            // out: the state the kernel left (plain) / the slots composed in file order by rsqc_rl_compose.h (ranges)
    int error;                // out: the device error word behind read_length_kernel
};
KrRequest *g_kr = nullptr;
}  // namespace

extern "C" __attribute__((visibility("default"))) unsigned long long k1emu_uniform_calls() { return g_k1e_uniform_calls; }
extern "C" __attribute__((visibility("default"))) unsigned long long k1emu_ucache_hits() { return g_k1e_ucache_hits; }
extern "C" __attribute__((visibility("default"))) unsigned long long k1emu_uniform2_calls() { return g_k1e_uniform2_calls; }

// the seeded schedule of wavemu.h for every kernel this library runs from now on (0: back to the default round-robin)
extern "C" __attribute__((visibility("default"))) void k1emu_set_schedule_seed(unsigned long long seed) { wavemu::set_seed(seed); }

// k1e_overflow and the flush of classify_long_kernel's tail on their own: ONE workgroup of four waves whose LDS stage already holds `start`
// entries ((1 << 48) | slot; the rest of the buffer is `poison`).  Wave w makes n_calls[w] calls of k1e_overflow, call c with the lanes of
// masks[first[w] + c] set and the index (w << 40) | (c << 8) | lane, then the workgroup flushes as the kernel does.  Out: the general
// kernel's list (ovf_index[0 : *ovf_count], capacity `cap`) and the final stage counter / end.  Returns the kernel error word.
extern "C" __attribute__((visibility("default")))
int k1emu_overflow_script(uint32_t start, const uint64_t *masks, const uint32_t *first /*[4]*/, const uint32_t *n_calls /*[4]*/, uint64_t poison,
                          uint64_t *ovf_index, uint32_t cap, uint32_t *ovf_count, uint32_t *ctl_out /*[2]*/) {
    static unsigned long long s_stage[K1E_OVF_STAGE];          // (what __shared__ is under the emulation: one workgroup at a time)
    static K1eStageCtl s_ctl;
    static uint32_t s_piece;
    if (start > K1E_OVF_STAGE) return RSQC_ERR_ARG;
    for (uint32_t j = 0; j < K1E_OVF_STAGE; ++j) s_stage[j] = j < start ? ((1ull << 48) | j) : poison;
    for (uint32_t j = 0; j < cap; ++j) ovf_index[j] = poison;
    int error = 0;
    *ovf_count = 0u;
    K1Args A{};
    A.acc.ovf_count = ovf_count; A.acc.ovf_index = ovf_index; A.acc.ovf_cap = cap; A.acc.error = &error;
    g_k1e_args = &A;
    wavemu::grid_dim().x = 1; wavemu::block_idx().x = 0;
    wavemu::run_block(RSQC_K1_THREADS, [&]() {
        if (threadIdx.x == 0) { s_ctl.init(); s_ctl.n = start; }
        __syncthreads();
        const uint32_t w = threadIdx.x >> 6, l = threadIdx.x & 63u;
        for (uint32_t c = 0; c < n_calls[w]; ++c)
            k1e_overflow(((masks[first[w] + c] >> l) & 1ull) != 0ull, ((uint64_t)w << 40) | ((uint64_t)c << 8) | l, s_stage, &s_ctl);
        __syncthreads();
        k1e_stage_flush(A.acc, s_stage, &s_ctl, &s_piece);
    });
    g_k1e_args = nullptr;
    ctl_out[0] = s_ctl.n; ctl_out[1] = s_ctl.end;
    return error;
}

// the candidates of the last --bed run, in file order: file index, name hash, second hash, BED row, end position, flag_size
namespace { struct LastCand { uint64_t file, q; uint32_t h2; int32_t name, end; uint32_t fs; }; std::vector<LastCand> g_last_cands; }
extern "C" __attribute__((visibility("default")))
void k1emu_last_candidates(uint64_t *file, uint64_t *q, uint32_t *h2, int32_t *name, int32_t *end, uint32_t *fs) {
    for (size_t k = 0; k < g_last_cands.size(); ++k) { const LastCand &c = g_last_cands[k]; file[k] = c.file; q[k] = c.q; h2[k] = c.h2; name[k] = c.name; end[k] = c.end; fs[k] = c.fs; }
}
// returns 0, an RSQC_ERR_* code, or 1000 + k for a failed internal check k
extern "C" __attribute__((visibility("default")))
int k1emu_run_bed(const rsqc_params *p, const rsqc_annotation *a, const rsqc_batch *b, const rsqc_bed *bed, int grid, int slow_kernel,
                  uint64_t *counters, uint64_t *gene_reads, uint64_t *gene_unique, uint64_t *gene_frag, double *exon_reads,
                  int32_t *read_length, uint32_t *cov_out, uint64_t *stats);
extern "C" __attribute__((visibility("default")))
int k1emu_run(const rsqc_params *p, const rsqc_annotation *a, const rsqc_batch *b, int grid, int slow_kernel,
              uint64_t *counters, uint64_t *gene_reads, uint64_t *gene_unique, uint64_t *gene_frag, double *exon_reads /*by exon id*/,
              int32_t *read_length, uint32_t *cov_out /*cov_entries or NULL*/, uint64_t *stats /*[4]: overflow, listed | deferred << 32, pairs, coarse-table hits*/) {
    return k1emu_run_bed(p, a, b, nullptr, grid, slow_kernel, counters, gene_reads, gene_unique, gene_frag, exon_reads, read_length, cov_out, stats);
}
// `bed` (may be NULL): with it the --bed instance classify_ei_kernel<true> runs, and the fragment-size candidates it leaves in the workgroups'
// regions must be EXACTLY the records that pass src/RNASeQC.cpp:372 and the block tests of bed_interval_of, computed here record by record
// without the kernel's wave-level cursor shortcut (that path had no emulation coverage); stats[3] then = candidates
extern "C" __attribute__((visibility("default")))
int k1emu_run_bed(const rsqc_params *p, const rsqc_annotation *a, const rsqc_batch *b, const rsqc_bed *bed, int grid, int slow_kernel,
              uint64_t *counters, uint64_t *gene_reads, uint64_t *gene_unique, uint64_t *gene_frag, double *exon_reads /*by exon id*/,
              int32_t *read_length, uint32_t *cov_out /*cov_entries or NULL*/, uint64_t *stats /*[4]: overflow, listed | deferred << 32, pairs, coarse-table hits*/) {
    HostIndex hx; std::string err;
    int rc = hx.build(a, nullptr, err);
    if (rc) return rc;
    DevAnnotation d{};
    d.n_ref = a->n_ref; d.n_contigs = a->n_contigs; d.n_genes = a->n_genes; d.n_listed = a->n_genes_listed; d.n_exons = a->n_exons;
    d.bin_shift = HostIndex::kBinShift;
    d.contig = hx.contig.data();
    if (hx.ex_rows.empty()) hx.ex_rows.push_back(ExonRow{0, 0, 0, 0});
    if (hx.gb.empty()) hx.gb.push_back(GeneBreak{0, 0});
    if (hx.ex_pmax.empty()) hx.ex_pmax.push_back(0);
    d.ex = hx.ex_rows.data(); d.gb = hx.gb.data(); d.ex_pmax = hx.ex_pmax.data();
    d.ex_binhi = hx.ex_binhi.data(); d.gb_bin = hx.gb_bin.data(); d.ex_cov = hx.ex_cov.data();
    std::vector<EiRank> rank; hx.build_rank(rank);
    d.ei = hx.ei.data(); d.ei_rank = rank.data(); d.ei_coarse = hx.ei_coarse.data();
    std::vector<uint32_t> ex_id(a->exon_row_id, a->exon_row_id + a->n_exons); if (ex_id.empty()) ex_id.push_back(0);
    d.ex_id = ex_id.data();
    std::vector<uint32_t> zero_range((size_t)a->n_contigs + 1, 0);
    d.bed_range = zero_range.data(); d.have_bed = 0;
    std::vector<int32_t> bed_pmax;
    if (bed) {                                                             // as rsqc_set_bed builds them (no bin table: bed_interval_of searches)
        for (int i = 0; i < bed->n_intervals; ++i) {
            if (bed->contig[i] < 0 || bed->contig[i] >= a->n_contigs) return RSQC_ERR_ARG;
            zero_range[(size_t)bed->contig[i] + 1]++;
        }
        for (int k = 0; k < a->n_contigs; ++k) zero_range[(size_t)k + 1] += zero_range[(size_t)k];
        bed_pmax.resize((size_t)std::max(bed->n_intervals, 1));
        for (int k = 0; k < a->n_contigs; ++k) {
            int32_t m = INT32_MIN;
            for (uint32_t i = zero_range[(size_t)k]; i < zero_range[(size_t)k + 1]; ++i) { m = std::max(m, bed->end[i]); bed_pmax[i] = m; }
        }
        d.bed_start = bed->start; d.bed_end = bed->end; d.bed_pmax = bed_pmax.data(); d.bed_binhi = nullptr; d.bed_bin_base = nullptr; d.have_bed = 1;
    }
    DevParams dp{p->mapq_threshold, p->base_mismatch, p->chimeric_distance, p->stranded, p->unpaired, p->exclude_chimeric, p->n_filter_tags, 0};

    // the batch with the slack the device buffers carry (kernels read a few entries past the end with ignored loads)
    const uint64_t n = b->n;
    std::vector<rsqc_rec_core> core((size_t)n + 2); std::vector<rsqc_rec_aux> aux((size_t)n + 2);
    std::vector<uint32_t> cigar((size_t)b->n_cigar_total + 8, 0u);
    if (n) { memcpy(core.data(), b->core, (size_t)n * sizeof(rsqc_rec_core)); memcpy(aux.data(), b->aux, (size_t)n * sizeof(rsqc_rec_aux)); }
    if (b->n_cigar_total) memcpy(cigar.data(), b->cigar, (size_t)b->n_cigar_total * 4);
    std::vector<uint32_t> qh2((size_t)n + 2, 0u);
    if (n && b->qhash2) memcpy(qh2.data(), b->qhash2, (size_t)n * 4);
    DevBatch db{};
    db.qhash2 = b->qhash2 ? qh2.data() : nullptr;
    db.n = n; db.record_base = b->file_index_base; db.core = core.data(); db.aux = aux.data(); db.cigar = cigar.data();
    db.n_seg = b->n_seg; db.seg_tid = b->seg_tid; db.seg_start = b->seg_start;
    db.n_wide = b->n_wide; db.wide_index = b->wide_index; db.wide_nm = b->wide_nm; db.wide_l_qseq = b->wide_l_qseq; db.wide_n_cigar = b->wide_n_cigar;
    const bool kr_ranges = g_kr && g_kr->ranges;
    if (kr_ranges) { if (!b->seg_file_index || !b->n_seg) return RSQC_ERR_ARG; db.seg_file_index = b->seg_file_index; }

    const size_t G = (size_t)a->n_genes, E = (size_t)a->n_exons;
    std::vector<unsigned long long> u64(3 * G + RSQC_N_COUNTERS + 1, 0ull);
    std::vector<double> exon_acc(E + 1, 0.0);
    std::vector<uint32_t> cov((size_t)hx.cov_entries + 64, 0u);
    const uint64_t total_waves = (uint64_t)grid * K1E_WAVES;
    const uint64_t per_wave = (((n + total_waves - 1) / total_waves) + 63ull) & ~63ull;
    const uint32_t chunk_cap = (uint32_t)(per_wave * K1E_WAVES * FAST_SET);
    const uint32_t slow_cap = 1u << 16;
    const int lgrid = grid > 2 ? grid - 1 : grid;                          // workgroups of classify_long_kernel: each owns a chunk behind the K1 grid's
    const int n_chunks = grid + lgrid;
    std::vector<PairRec> pairs((size_t)chunk_cap * n_chunks + slow_cap + 8, PairRec{0xFFFFFFF0u, 0xFEEDu, 0ull});
    std::vector<uint32_t> chunk_count((size_t)n_chunks + 2, 0xDEADu);
    std::vector<uint32_t> ovf_count(4, 0u); std::vector<uint64_t> ovf_index(1u << 20);
    std::vector<uint32_t> defer_index((size_t)n + 64, 0xDEFE0000u), defer_list((size_t)n + 64 * (size_t)grid + 64, 0xDEFE0001u); uint32_t defer_total = 0;
    std::vector<uint32_t> tile_span((size_t)((n + 63) / 64) + 64 * (size_t)total_waves + 64, 0xABCDu);
    std::vector<uint32_t> rl_stats = {0u, 0xFFFFFFFFu, 0u};
    int32_t rl_state = g_kr && !kr_ranges ? (int32_t)g_kr->r_in : 0; int error = 0;
    // a batch of ranges: the per-segment inputs, armed {max span 0, min l_qseq UINT_MAX, max l_qseq 0} (rsqc_submit.cpp)
    std::vector<uint32_t> rl_seg;
    if (kr_ranges) for (uint32_t s = 0; s < b->n_seg; ++s) { rl_seg.push_back(0u); rl_seg.push_back(0xFFFFFFFFu); rl_seg.push_back(0u); }
    DevAccum acc{};
    acc.gene_reads = u64.data(); acc.gene_unique = acc.gene_reads + G; acc.gene_frag = acc.gene_unique + G; acc.counters = acc.gene_frag + G;
    acc.exon_acc = exon_acc.data(); acc.cov_diff = cov.data();
    acc.pairs = pairs.data();
    acc.pair_chunk_cap = chunk_cap; acc.pair_chunk_count = chunk_count.data();
    acc.pair_slow_base = chunk_cap * (uint32_t)n_chunks; acc.pair_slow_cap = slow_cap; acc.pair_slow_count = chunk_count.data() + n_chunks;
    acc.ovf_count = ovf_count.data(); acc.ovf_index = (uint64_t *)ovf_index.data(); acc.ovf_cap = (uint32_t)ovf_index.size();
    acc.defer_index = defer_index.data(); acc.defer_list = defer_list.data(); acc.defer_total = &defer_total;
    // --bed: the workgroups' candidate regions (a slot per record) and their counts
    std::vector<uint64_t> fr_file((size_t)n + 64), fr_qhash((size_t)n + 64);
    std::vector<int32_t> fr_name((size_t)n + 64), fr_end((size_t)n + 64);
    std::vector<uint32_t> fr_fs((size_t)n + 64), fr_h2((size_t)n + 64), fr_counts((size_t)grid + 1, 0xDEADu);
    acc.frag.file_index = fr_file.data(); acc.frag.qhash = fr_qhash.data(); acc.frag.name = fr_name.data(); acc.frag.endpos = fr_end.data();
    acc.frag.flag_size = fr_fs.data(); acc.frag.h2 = fr_h2.data(); acc.frag.chunk_count = fr_counts.data(); acc.frag.count = nullptr; acc.frag.cap = (uint32_t)n;
    acc.tile_span = tile_span.data();
    acc.rl_stats = rl_stats.data(); acc.read_length = &rl_state; acc.error = &error;
    acc.rl_seg = kr_ranges ? rl_seg.data() : nullptr;

    const K1Args A{d, dp, db, acc};
    g_k1e_args = &A; g_k1e_coarse_hits = 0; g_k1e_uniform_calls = 0; g_k1e_ucache_hits = 0; g_k1e_uniform2_calls = 0;
    wavemu::grid_dim().x = (uint32_t)grid;
    for (int k = 0; k < grid; ++k) {
        wavemu::block_idx().x = (uint32_t)k;
        if (bed) wavemu::run_block(RSQC_K1_THREADS, [&]() { classify_ei_kernel<true>(A); });
        else wavemu::run_block(RSQC_K1_THREADS, [&]() { classify_ei_kernel<false>(A); });      // (the instance of runs without a BED)
    }
    uint64_t n_deferred = 0;
    for (uint32_t k = 0; k < defer_total; ++k) { ++n_deferred; if ((defer_list[k] & 0x7FFFFFFFu) >= n) return 1013; }
    {   // the records it deferred (more than eight operations / three blocks, the three-block ring's surplus) -> classify_long_kernel
        wavemu::grid_dim().x = (uint32_t)lgrid;
        for (int k = 0; k < lgrid; ++k) {
            wavemu::block_idx().x = (uint32_t)k;
            wavemu::run_block(RSQC_K1_THREADS, [&]() { classify_long_kernel(A, (uint32_t)grid); });
        }
        wavemu::grid_dim().x = (uint32_t)grid;
    }
    if (getenv("K1EMU_TRACE")) fprintf(stderr, "k1emu: per-record kernels done, error %d\n", error);
    uint64_t listed = 0;
    if (error) return error;

    // ---- the overflow list through the general per-record code ------------------------------------------------------
    std::vector<uint64_t> reads(G, 0), unique(G, 0);
    std::vector<double> exon_rows(E, 0.0);
    std::vector<std::set<std::pair<uint64_t, uint32_t>>> names(G);
    SlowAccH sacc{&reads, &unique, &exon_rows, &cov, &names};
    std::vector<int32_t> tid_of((size_t)n, -1);
    for (uint32_t s = 0; s < b->n_seg; ++s) for (uint64_t i = b->seg_start[s]; i < b->seg_start[s + 1]; ++i) tid_of[(size_t)i] = b->seg_tid[s];
    auto load = [&](uint64_t i, Record &r) -> bool {
        const rsqc_rec_core &co = b->core[i]; const rsqc_rec_aux &au = b->aux[i];
        r.tid = tid_of[(size_t)i]; r.pos = co.pos; r.mpos = co.mpos; r.isize = co.isize; r.flag = au.flag;
        r.mapq = au.mapq; r.tagbits = au.tagbits; r.l_qseq = au.l_qseq; r.nm = au.nm; r.n_cigar = au.n_cigar;
        if (au.l_qseq == RSQC_LQSEQ_ESCAPE || au.nm == RSQC_NM_ESCAPE || au.n_cigar == RSQC_NCIGAR_ESCAPE) {
            uint32_t w = 0;
            while (w < b->n_wide && b->wide_index[w] < i) ++w;
            if (w >= b->n_wide || b->wide_index[w] != i) return false;
            r.l_qseq = b->wide_l_qseq[w]; r.nm = b->wide_nm[w]; r.n_cigar = b->wide_n_cigar[w];
        }
        r.cigar = cigar.data() + co.cigar_off; r.qhash = au.qhash;
        return true;
    };
    std::set<uint64_t> seen_ovf;
    const uint32_t n_overflow = ovf_count[0];                  // (read_length_kernel, the batch's last kernel, zeroes the counter)
    if (slow_kernel) {
        // the general KERNEL on the list, sized as launch_classify_slow sizes it; it adds to the same accumulators and appends
        // its (gene, name) pairs to the slow-path region of the pair buffer
        for (uint32_t k = 0; k < ovf_count[0]; ++k) {
            const uint64_t i = ovf_index[k] & ~(1ull << 63);
            if (i >= n || !seen_ovf.insert(i).second) return 1002;
            if (ovf_index[k] >> 63) ++listed;
        }
        const uint32_t blocks = (uint32_t)std::max<uint64_t>(2, std::min<uint64_t>(8, n / 200 / RSQC_SLOW_THREADS + 1));
        wavemu::grid_dim().x = blocks;
        for (uint32_t k = 0; k < blocks; ++k) {
            wavemu::block_idx().x = k;
            wavemu::run_block(RSQC_SLOW_THREADS, [&]() { classify_slow_kernel<false>(d, dp, db, acc); });
        }
        if (error) return error;
        const uint32_t ns = chunk_count[(size_t)n_chunks];
        if (ns > slow_cap) return 1008;
        for (uint32_t j = 0; j < ns; ++j) {
            const PairRec &pr = pairs[(size_t)acc.pair_slow_base + j];
            if (pr.gene >= G) return 1005;
            names[pr.gene].insert({(uint64_t)pr.hash, pr.h2});
        }
    } else
    for (uint32_t k = 0; k < ovf_count[0]; ++k) {
        const uint64_t i = ovf_index[k] & ~(1ull << 63);
        const bool long_straggler = (ovf_index[k] >> 63) != 0;            // K1E_OVF_LONG: blocks and operations are this code's to count / check
        if (i >= n || !seen_ovf.insert(i).second) return 1002;            // every record at most once
        Record r;
        if (!load(i, r)) return RSQC_ERR_ARG;
        RecordCounters rc2; bool hq; uint32_t aligned; Blocks B;
        const bool go2 = gate_cascade(d, dp, r, rc2, hq, aligned, B);
        if (long_straggler) { if (rc2.error) return rc2.error; acc.counters[RSQC_C_ALIGNMENT_BLOCKS] += rc2.blocks; ++listed; }
        if (!go2) return 1003;                                            // only records that reach the feature stage are listed
        bool over = false;
        FeatureOut<SLOW_SET, SLOW_STAGE> so;
        exon_metrics<SLOW_SET>(d, dp, r, hq, aligned, sacc, so, over);
        if (over) return RSQC_ERR_CAPACITY;
        for (int k2 = 0; k2 < SLOW_STAGE; ++k2) {
            if (!((so.cmask >> k2) & 1u)) continue;
            const Commit &c = so.commit[k2];
            if (c.len > 0) sacc.exon_add(c.row, (double)c.len / (double)aligned);
            sacc.cov_range(c.cidx, c.len);
        }
        for (int k2 = 0; k2 < so.n_hit; ++k2) sacc.gene_hit(so.hit[k2], !(r.flag & RSQC_FDUP), r.qhash, b->qhash2 ? b->qhash2[i] : 0u);
        for (int c = 0; c < RSQC_N_COUNTERS; ++c) if ((so.bits >> c) & 1ull) acc.counters[c]++;
    }
    // ---- pairs -> distinct names per gene ------------------------------------------------------------------------------
    uint64_t n_pairs = 0;
    for (int k = 0; k < n_chunks; ++k) {
        const uint32_t cnt = chunk_count[(size_t)k];
        if (cnt > chunk_cap) return 1004;
        for (uint32_t j = 0; j < cnt; ++j) {
            const PairRec &pr = pairs[(size_t)k * chunk_cap + j];
            if (pr.gene >= G) return 1005;
            names[pr.gene].insert({(uint64_t)pr.hash, pr.h2}); ++n_pairs;
        }
    }
    // ---- Read-Length inputs: tile maxima and batch extremes against the per-record values; the state machine itself ---
    uint32_t rl = (uint32_t)rl_state, smax = 0, lmin = 0xFFFFFFFFu, lmax = 0;
    {
        std::vector<uint32_t> want((size_t)((n + 63) / 64), 0u);
        std::vector<uint32_t> want_seg(rl_seg.size());
        for (size_t k = 0; k < want_seg.size(); ++k) want_seg[k] = k % 3 == 1 ? 0xFFFFFFFFu : 0u;
        uint32_t sg = 0;
        for (uint64_t i = 0; i < n; ++i) {
            Record r;
            if (!load(i, r)) return RSQC_ERR_ARG;
            RecordCounters rc2; bool hq; uint32_t aligned; Blocks B;
            gate_cascade(d, dp, r, rc2, hq, aligned, B);
            if (rc2.error) return rc2.error;
            while (kr_ranges && sg + 1 < b->n_seg && b->seg_start[sg + 1] <= i) ++sg;
            if (rc2.rl_eligible) {
                want[(size_t)(i >> 6)] = std::max(want[(size_t)(i >> 6)], rc2.rl_span);
                smax = std::max(smax, rc2.rl_span); lmin = std::min(lmin, (uint32_t)rc2.rl_lqseq); lmax = std::max(lmax, (uint32_t)rc2.rl_lqseq);
                if (rc2.rl_span > rl) rl = (uint32_t)rc2.rl_lqseq;
                if (kr_ranges) {
                    uint32_t *ws = want_seg.data() + 3 * (size_t)sg;
                    ws[0] = std::max(ws[0], rc2.rl_span); ws[1] = std::min(ws[1], (uint32_t)rc2.rl_lqseq); ws[2] = std::max(ws[2], (uint32_t)rc2.rl_lqseq);
                }
            }
        }
        // per-wave ranges are multiples of 64 records, so a wave's tile t is batch tile (wbeg / 64 + t)
        for (size_t t = 0; t < want.size(); ++t) if (tile_span[t] != want[t]) return 1006;
        if (kr_ranges) { if (rl_seg != want_seg) return 1014; }              // (the batch-level extremes are not kept for a batch of ranges)
        else if (rl_stats[0] != smax || rl_stats[1] != lmin || rl_stats[2] != lmax) return 1007;
        const uint32_t entries = kr_ranges ? b->n_seg : 1u;
        if (g_kr) {
            for (size_t t = 0; t < want.size(); ++t) g_kr->tile_span[t] = tile_span[t];
            for (uint32_t k = 0; k < 3u * entries; ++k) g_kr->extremes[k] = kr_ranges ? rl_seg[k] : rl_stats[k];
        }
        // the Read-Length KERNEL: the batch's transfer function applied to the entry state must leave the value of the walk above
        // (a batch of ranges: a block per segment, a slot each, composed by the product's own loop in file order from state 0)
        std::vector<uint32_t> own_summary(g_kr ? 0 : RSQC_RL_SUMMARY_WORDS + 8, 0u);
        uint32_t *const summary = g_kr ? g_kr->summary : own_summary.data();
        wavemu::grid_dim().x = entries;
        for (uint32_t k = 0; k < entries; ++k) {
            wavemu::block_idx().x = k;
            wavemu::run_block(64, [&]() { read_length_kernel(d, dp, db, acc, summary); });
        }
        wavemu::grid_dim().x = 1; wavemu::block_idx().x = 0;
        if (kr_ranges) {
            std::vector<std::vector<uint32_t>> keys(entries); std::vector<std::vector<int32_t>> vals(entries);
            std::vector<RlTable> tables;
            for (uint32_t k = 0; k < entries; ++k) {
                const uint32_t *w = summary + (size_t)k * RSQC_RL_SUMMARY_WORDS;
                for (uint32_t j = 0; j < std::min<uint32_t>(w[0], RSQC_RL_MAXP); ++j) { keys[k].push_back(w[2 + 2 * j]); vals[k].push_back((int32_t)w[3 + 2 * j]); }
                tables.push_back(RlTable{b->seg_file_index[k], keys[k].data(), vals[k].data(), (uint32_t)keys[k].size()});
            }
            rl_state = rl_compose(tables);
        }
        if (g_kr) { g_kr->state = rl_state; g_kr->error = error; }
        if (error) return error;
        if ((uint32_t)rl_state != rl) return 1009;
    }
    // ---- the fragment-counting KERNELS (rsqc_k4.h) on the pair buffers as the kernels above left them: must equal the name sets
    if (slow_kernel && G > 0) {
        const uint64_t parts_bound = n_pairs / RSQC_K4_PART_READS + chunk_count[(size_t)n_chunks] / RSQC_K4_PART_READS + G + 2;
        const uint64_t all_pairs = n_pairs + chunk_count[(size_t)n_chunks];
        const uint64_t keys_bound = 2 * all_pairs + (uint64_t)RSQC_K4_SUB_CAP * std::min<uint64_t>(parts_bound, all_pairs / RSQC_K4_PART_READS + 1) + 16 * G + 16;
        const uint32_t lay_blocks = (uint32_t)((G + 1023) / 1024);
        std::vector<uint4> ginfo(G + 1), part_info(parts_bound);
            std::vector<uint32_t> part_first(G + 2), cursor(parts_bound, 0u), full_list(parts_bound), blk_parts(lay_blocks);
        std::vector<unsigned long long> blk_space(lay_blocks), frag(G, 0ull); std::vector<FragKey> list(keys_bound);
        uint32_t full_n = 0;
        wavemu::grid_dim().x = lay_blocks;
        for (uint32_t k = 0; k < lay_blocks; ++k) { wavemu::block_idx().x = k; wavemu::run_block(1024, [&]() { frag_layout_totals_kernel(acc.gene_reads, (uint32_t)G, blk_space.data(), blk_parts.data(), &error); }); }
        for (uint32_t k = 0; k < lay_blocks; ++k) { wavemu::block_idx().x = k; wavemu::run_block(1024, [&]() { frag_layout_kernel(acc.gene_reads, (uint32_t)G, blk_space.data(), blk_parts.data(), part_first.data(), ginfo.data(), cursor.data(), part_info.data(), &full_n); }); }
        if (error) return error;
        if (part_first[G] > parts_bound) return 1010;
        const uint32_t fgrid = frag_local_chunk_wgs((uint32_t)n_chunks) + 4u;
        wavemu::grid_dim().x = fgrid;
        for (uint32_t k = 0; k < fgrid; ++k) {
            wavemu::block_idx().x = k;
            wavemu::run_block(RSQC_K4L_THREADS, [&]() { frag_local_kernel(pairs.data(), chunk_cap, chunk_count.data(), (uint32_t)n_chunks, acc.pair_slow_base, slow_cap,
                                                                          ginfo.data(), cursor.data(), list.data(), &error); });
        }
        wavemu::grid_dim().x = 8;
        for (uint32_t k = 0; k < 8; ++k) { wavemu::block_idx().x = k; wavemu::run_block(RSQC_K4_COUNT_THREADS, [&]() { frag_count_kernel<RSQC_K4_PART_SLOTS / 2>(part_first.data() + G, cursor.data(), part_info.data(), list.data(), frag.data(), full_list.data(), &full_n, &error); }); }
        wavemu::grid_dim().x = 2;
        for (uint32_t k = 0; k < 2; ++k) { wavemu::block_idx().x = k; wavemu::run_block(RSQC_K4_COUNT_THREADS, [&]() { frag_count_kernel<RSQC_K4_PART_SLOTS>(part_first.data() + G, cursor.data(), part_info.data(), list.data(), frag.data(), full_list.data(), &full_n, &error); }); }
        if (error) return error;
        for (size_t g = 0; g < G; ++g) {
            // (a key of 0 is stored as a fixed non-zero constant by frag_local_kernel: a name hashing to 0 and one hashing to that
            //  constant would merge -- neither occurs in the tests' names)
            if (frag[g] != (unsigned long long)names[g].size()) return 1011;
        }
    }
    for (size_t g = 0; g < (size_t)a->n_genes_listed; ++g) {
        gene_reads[g] = acc.gene_reads[g] + reads[g]; gene_unique[g] = acc.gene_unique[g] + unique[g]; gene_frag[g] = names[g].size();
    }
    for (int c = 0; c < RSQC_N_COUNTERS; ++c) counters[c] = acc.counters[c];
    for (int e = 0; e < a->n_exons; ++e) exon_reads[a->exon_row_id[e]] = exon_rows[(size_t)e] + exon_acc[a->exon_row_id[e]];
    *read_length = (int32_t)rl;
    if (cov_out) memcpy(cov_out, cov.data(), hx.cov_entries * 4);
    uint64_t n_cand = 0;
    g_last_cands.clear();
    if (getenv("K1EMU_TRACE")) fprintf(stderr, "k1emu: reached the candidate check\n");
    if (bed) {                                                             // the kernel's candidates against the per-record rule, no shortcut
        std::map<uint64_t, size_t> got;                                    // record index -> slot
        for (int k = 0; k < grid; ++k) {
            uint32_t beg, end;
            k1e_wg_range((uint32_t)n, (uint32_t)grid, (uint32_t)k, beg, end);
            if (fr_counts[(size_t)k] > end - beg) return 1020;
            for (uint32_t j = 0; j < fr_counts[(size_t)k]; ++j) {
                const uint64_t idx = fr_file[(size_t)beg + j] - b->file_index_base;
                if (idx >= n || idx < beg || idx >= end || !got.emplace(idx, (size_t)beg + j).second) return 1021;
            }
        }
        for (uint64_t i = 0; i < n; ++i) {
            Record r;
            if (!load(i, r)) return RSQC_ERR_ARG;
            RecordCounters rc2; bool hq; uint32_t aligned; Blocks B;
            gate_cascade(d, dp, r, rc2, hq, aligned, B);
            const int32_t name = (rc2.frag_candidate && r.tid >= 0 && r.tid < a->n_contigs) ? bed_interval_of(d, r) : -1;
            const auto it = got.find(i);
            if ((name >= 0) != (it != got.end())) return name >= 0 ? 1022 : 1023;      // 1022: the kernel skipped a candidate (the cursor shortcut)
            if (name < 0) continue;
            ++n_cand;
            const size_t sl = it->second;
            const bool fok = !(r.flag & RSQC_FMREVERSE) && (r.flag & RSQC_FREVERSE) && r.pos != r.mpos;
            const uint32_t sz = (uint32_t)(r.isize < 0 ? -(int64_t)r.isize : (int64_t)r.isize);
            if (fr_name[sl] != name || fr_end[sl] != rc2.endpos || fr_qhash[sl] != r.qhash || fr_fs[sl] != ((sz & 0x7FFFFFFFu) | (fok ? 0x80000000u : 0u)) ||
                fr_h2[sl] != (b->qhash2 ? b->qhash2[i] : 0u)) return 1024;
            g_last_cands.push_back(LastCand{fr_file[sl], fr_qhash[sl], fr_h2[sl], fr_name[sl], fr_end[sl], fr_fs[sl]});
        }
    }
    stats[0] = n_overflow; stats[1] = listed | (n_deferred << 32); stats[2] = n_pairs; stats[3] = bed ? n_cand : g_k1e_coarse_hits;
    return 0;
}

// ---- the Read-Length stage on its own terms (tests/test_kr_edges_host.py): the same run as k1emu_run -- every check above holds --
// with an entry state or as a batch of file ranges, and with the kernel's inputs and raw summary slots handed back.
// summary: (entries + 1) * RSQC_RL_SUMMARY_WORDS words, filled by the caller (a poison pattern: words the kernel does not own must come
// back as they went in); entries = 1, or n_seg for ranges.  info[0] = the final state, info[1] = the device error word.
extern "C" __attribute__((visibility("default")))
int k1emu_run_kr(const rsqc_params *p, const rsqc_annotation *a, const rsqc_batch *b, int grid, uint32_t r_in, int ranges,
                 uint32_t *tile_span, uint32_t *extremes, uint32_t *summary, int32_t *info /*[2]*/) {
    const size_t G = (size_t)std::max(a->n_genes, 1), E = (size_t)std::max(a->n_exons, 1);
    std::vector<uint64_t> counters(RSQC_N_COUNTERS), gr(G), gu(G), gf(G); std::vector<double> ex(E);
    int32_t rl = 0; uint64_t stats[4] = {0, 0, 0, 0};
    KrRequest rq{r_in, ranges, tile_span, extremes, summary, 0, 0};
    g_kr = &rq;
    const int rc = k1emu_run_bed(p, a, b, nullptr, grid, 1, counters.data(), gr.data(), gu.data(), gf.data(), ex.data(), &rl, nullptr, stats);
    g_kr = nullptr;
    info[0] = rq.state; info[1] = rq.error;
    return rc;
}
// rsqc_rl_compose.h as the product calls it: tables k = (span, state)[offset[k] : offset[k + 1]] at file_index[k], any order
extern "C" __attribute__((visibility("default")))
int32_t k1emu_rl_compose(const uint64_t *file_index, const uint32_t *offset, const uint32_t *span, const int32_t *state, uint32_t n) {
    std::vector<RlTable> tables;
    for (uint32_t k = 0; k < n; ++k) tables.push_back(RlTable{file_index[k], span + offset[k], state + offset[k], offset[k + 1] - offset[k]});
    return rl_compose(tables);
}

// the message rsqc_last_error gives for a pass that ended on the limit of 128 prefix maxima (rsqc_rl_compose.h: rl_limit_message), from raw
// summary slots as k1emu_run_kr hands them back; returns its length (0: no slot is flagged)
extern "C" __attribute__((visibility("default")))
uint32_t k1emu_rl_limit_message(const uint32_t *summary, uint32_t entries, const uint64_t *file_index, const uint64_t *records, char *out, uint32_t cap) {
    const std::string msg = rl_limit_message(summary + 1, RSQC_RL_SUMMARY_WORDS, entries, file_index, records);
    if (cap) { const size_t m = std::min<size_t>(msg.size(), cap - 1); memcpy(out, msg.data(), m); out[m] = 0; }
    return (uint32_t)msg.size();
}

#ifdef K1EMU_MAIN
// A stand-alone program over case files (tests/hostemu/__init__.py: write_kr_case_file), so that the harness and the kernels run under the
// host sanitizers without anything sanitized inside Python.  Prints one line per file: rc, error, state, and per slot P and the flag word;
// `guard` counts the words behind entry P of any slot (and of the guard slot) that no longer hold the poison.
#include <cstdio>
#include <memory>
namespace {
// (every array in an allocation of exactly its size: a read one entry past it is the sanitizer's to report)
struct Blob { std::unique_ptr<unsigned char[]> store; size_t bytes = 0; template <class T> const T *as() const { return bytes ? reinterpret_cast<const T *>(store.get()) : nullptr; } };
bool read_blob(FILE *f, Blob &bl) {
    uint64_t nb = 0;
    if (fread(&nb, 8, 1, f) != 1) return false;
    bl.bytes = (size_t)nb; bl.store.reset(new unsigned char[(size_t)nb ? (size_t)nb : 1]);
    return nb == 0 || fread(bl.store.get(), 1, (size_t)nb, f) == (size_t)nb;
}
}  // namespace
int main(int argc, char **argv) {
    const uint32_t POISON = 0xA5A5A5A5u;
    for (int f_i = 1; f_i < argc; ++f_i) {
        FILE *f = fopen(argv[f_i], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[f_i]); return 2; }
        uint64_t head[3];                                              // grid, entry state, ranges
        if (fread(head, 8, 3, f) != 3) return 2;
        Blob bl[30];
        for (int k = 0; k < 30; ++k) if (!read_blob(f, bl[k])) { fprintf(stderr, "short case file %s\n", argv[f_i]); return 2; }
        fclose(f);
        if (bl[0].bytes != sizeof(rsqc_params) || bl[1].bytes != 20 || bl[18].bytes != 40) return 2;
        const rsqc_params *p = bl[0].as<rsqc_params>();
        const int32_t *an = bl[1].as<int32_t>();
        rsqc_annotation a{};
        a.n_ref = an[0]; a.n_contigs = an[1]; a.n_genes = an[2]; a.n_genes_listed = an[3]; a.n_exons = an[4];
        a.gene_row_contig = bl[2].as<int32_t>(); a.gene_row_start = bl[3].as<int32_t>(); a.gene_row_end = bl[4].as<int32_t>();
        a.gene_row_flags = bl[5].as<uint8_t>(); a.gene_row_id = bl[6].as<uint32_t>();
        a.exon_row_contig = bl[7].as<int32_t>(); a.exon_row_start = bl[8].as<int32_t>(); a.exon_row_end = bl[9].as<int32_t>();
        a.exon_row_flags = bl[10].as<uint8_t>(); a.exon_row_id = bl[11].as<uint32_t>(); a.exon_row_gene = bl[12].as<uint32_t>();
        a.gene_is_globin = bl[13].as<uint8_t>(); a.gene_exon_off = bl[14].as<uint32_t>(); a.gene_exon_row = bl[15].as<uint32_t>();
        a.gene_row_order = bl[16].as<uint32_t>(); a.exon_row_order = bl[17].as<uint32_t>();
        const uint64_t *bn = bl[18].as<uint64_t>();
        rsqc_batch b{};
        b.n = bn[0]; b.file_index_base = bn[1]; b.n_cigar_total = bn[2]; b.n_seg = (uint32_t)bn[3]; b.n_wide = (uint32_t)bn[4];
        b.core = bl[19].as<rsqc_rec_core>(); b.aux = bl[20].as<rsqc_rec_aux>(); b.cigar = bl[21].as<uint32_t>();
        b.seg_tid = bl[22].as<int32_t>(); b.seg_start = bl[23].as<uint64_t>();
        b.wide_index = bl[24].as<uint64_t>(); b.wide_nm = bl[25].as<int32_t>(); b.wide_l_qseq = bl[26].as<int32_t>(); b.wide_n_cigar = bl[27].as<uint32_t>();
        b.qhash2 = bl[28].as<uint32_t>(); b.seg_file_index = bl[29].as<uint64_t>();
        const uint32_t entries = head[2] ? b.n_seg : 1u;
        std::vector<uint32_t> tile_span((size_t)((b.n + 63) / 64)), extremes(3 * (size_t)entries), summary((size_t)(entries + 1) * RSQC_RL_SUMMARY_WORDS, POISON);
        int32_t info[2] = {0, 0};
        const int rc = k1emu_run_kr(p, &a, &b, (int)head[0], (uint32_t)head[1], (int)head[2], tile_span.data(), extremes.data(), summary.data(), info);
        printf("k1emu_kr rc=%d error=%d state=%d entries=%u", rc, info[1], info[0], entries);
        uint64_t touched = 0;
        for (uint32_t k = 0; k <= entries; ++k) {
            const uint32_t *w = summary.data() + (size_t)k * RSQC_RL_SUMMARY_WORDS;
            const uint32_t from = k < entries ? 2u + 2u * std::min<uint32_t>(w[0], RSQC_RL_MAXP) : 0u;
            if (k < entries) printf(" P%u=%u:%u", k, w[0], w[1]);
            for (uint32_t j = from; j < RSQC_RL_SUMMARY_WORDS; ++j) touched += w[j] != POISON;
        }
        printf(" guard=%llu\n", (unsigned long long)touched);
    }
    return 0;
}
#endif
