// rsqc_ctx.h -- private to csrc/: the context, its buffer types and the helpers that more than one unit of the C ABI calls (rsqc_api.cpp:
// lifetime, inputs; rsqc_submit.cpp: pools, run_batch; rsqc_finalize.cpp: end of file; rsqc_group.cpp: RCCL; rsqc_decode_api.cpp: BAM / SAM decode)
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rsqc_device.h"
#include "rsqc_decode.h"
#include "rsqc_sam.h"

// Knobs that make the library SKIP work (wrong or incomplete results) exist only in the diagnostic build (`make prof`,
// -DRSQC_K1_PROF): the product library does not read them.
#if defined(RSQC_K1_PROF) || defined(RSQC_DIAG_KNOBS)       /* (`make variant NAME=diag DEFS=-DRSQC_DIAG_KNOBS`: the knobs without the section timers) */
#define RSQC_DIAG(name) getenv(name)
// (RSQC_HOST_TRACE=1: host clock at the steps of a pass to stderr -- where a pass spends what the kernels' events do not show)
namespace rsqc {
inline void host_trace(const char *what) {
    static const bool on = getenv("RSQC_HOST_TRACE") != nullptr;
    if (!on) return;
    static std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[host] %-28s +%8.1f us\n", what, std::chrono::duration<double, std::micro>(now - last).count());
    last = now;
}
}  // namespace rsqc
#define RSQC_TRACE(what) rsqc::host_trace(what)
#else
#define RSQC_DIAG(name) ((const char *)nullptr)
#define RSQC_TRACE(what) ((void)0)
#endif

namespace rsqc {

struct DevBuf {
    void *p = nullptr; size_t bytes = 0;
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};
struct HostBuf {                   // page-locked host memory: a window of results that grows only (host_reserve)
    void *p = nullptr; size_t bytes = 0;
    void release() { if (p) (void)hipHostFree(p); p = nullptr; bytes = 0; }
};
struct UploadedBatch {
    DevBatch d{};
    std::vector<DevBuf> bufs;
    uint64_t n = 0, n_cigar_total = 0, file_index_base = 0;
    std::vector<uint64_t> seg_file_index, seg_records;   // a batch of several file ranges (rsqc_batch.seg_file_index): per segment
    DevBuf rl_seg;                                   // ... and its per-segment Read-Length inputs [3 * n_seg] (armed at every submit)
    bool pooled = false;           // transient upload: its buffers go back to the context's pool
    const uint64_t *umi = nullptr; // rsqc_batch.umi on the device (a pass under rsqc_markdup_use_umi only): read by the collection, by no kernel of the batch
};

// What a submitted batch leaves behind for the end-of-file stage is written into WORST-CASE sized buffers (the counts
// are only known on the device).  A batch that has completed is RETIRED at the next rsqc_submit / rsqc_wait: its
// counts are read from a page-locked mirror, what it actually emitted is appended to a growing arena, and the
// worst-case buffers go back to the pool -- so the memory held until rsqc_finalize is what was emitted (16 B per
// (gene, name) pair, 28 B per fragment-size candidate, 32 B per GC candidate) plus the buffers of the batches in flight.
struct PairBuf {                // (gene, qname-hash) pairs of one submitted batch
    DevBuf rec, counts;         // rec: PairRec[cap] {gene, second name hash (zero for a batch without rsqc_batch.qhash2), name hash}; counts: [n_chunks] per K1 block, then [1] slow-path counter
    uint64_t cap = 0;           // pair slots allocated
    uint32_t n_chunks = 0, chunk_cap = 0, slow_base = 0, slow_cap = 0;
    uint32_t counts_cap = 0;
    uint64_t pairs_bound = 0;   // most pairs the batch can have emitted
    uint32_t *h_counts = nullptr;   // page-locked mirror of `counts` (copied when the batch's kernels are done)
    hipEvent_t done = nullptr;      // the counts have arrived in h_counts
    hipEvent_t kernels = nullptr;   // the batch's per-record kernels are through (what the copy of the counts waits for, on a side stream)
    bool used = false;
};
struct FragBuf {                // fragment-size candidates of one submitted batch (BED runs only)
    DevBuf file, qhash, name, endpos, fs, h2, count;
    DevBuf r_file, r_qhash, r_name, r_endpos, r_fs, r_h2, r_counts;   // the per-record kernel's workgroup regions (packed into the columns above by frag_compact_kernel)
    uint32_t cap = 0, grid_cap = 0;
    uint32_t *h_count = nullptr;
    bool used = false;
};
struct GcBuf {                  // fragment GC candidates of one submitted batch (--fasta runs only)
    DevBuf file, qhash, row, endpos, flag_lq, tid, h2, count;
    uint32_t cap = 0;
    uint32_t *h_count = nullptr;
    bool used = false;
};
// growing device arrays of the retired batches: a few parallel columns with one fill level
struct Arena {
    DevBuf col[8]; size_t width[8] = {0, 0, 0, 0, 0, 0, 0, 0}; int n_col = 0;
    uint64_t used = 0, cap = 0;
};

// device-side BAM decode (rsqc_decode_*): the window buffers are sized once for the largest call and reused; the batch
// columns a window is parsed into are read by the per-read kernels of that window before the next window's kernels
// (same stream) overwrite them
struct DecodeState {
    bool active = false;
    BamTagSpec tags{};
    uint64_t next_file_index = 0, records = 0;
    uint32_t head = 1u << 22;          // room in front of the window for the carried-over part of a record
    uint32_t tail = 0;                 // bytes carried over, parked at [head - tail, head)
    size_t out_cap = 0, comp_cap = 0, blk_cap = 0;
    DevBuf comp, blocks, ubuf, seg, seg_rec0, seg_ops0, rec_off, ops_at, mark, core, aux, qh2, cigar, seg_tid, seg_start,
           wide_index, wide_nm, wide_lq, wide_nc, sum, carry, tailtmp, scratch;
    DevBuf umi;                        // the window's UMI keys: allocated only when tags.umi_src selects a source
    DecodeSummary *h_sum = nullptr;    // page-locked
    DevBgzfBlock *h_blocks = nullptr;  // page-locked, blk_cap entries
    bool unsorted = false;
    uint64_t n_bad = 0;
    std::vector<std::string> bad_names;
    std::vector<const char *> bad_ptrs;
    // RSQC_DECODE_PROFILE: stage times of the stream, printed at rsqc_decode_end
    bool profile = false; hipEvent_t pe[4] = {nullptr, nullptr, nullptr, nullptr};
    double ms_copy = 0, ms_inflate = 0, ms_parse = 0, ms_call = 0; uint64_t prof_in = 0, prof_out = 0, prof_calls = 0;
    std::chrono::steady_clock::time_point prof_t0;
    // a call is enqueued, then finished (its summary read, its records submitted) -- at once, or by the next call when the
    // stream is pipelined: the next call's file bytes then cross PCIe beside this call's kernels
    bool pipelined = false, pending = false, pend_limited = false;
    int slot = 0;                      // which half of comp / blocks / h_blocks the call in flight reads
    DecodeWindow pend_w{};
    std::chrono::steady_clock::time_point pend_wall0;
    hipStream_t copy_stream = nullptr; hipEvent_t ev_copy = nullptr;
    std::vector<int32_t> run_tid;      // contig segments of the last window
    rsqc_batch last{};                 // the last window's batch (device pointers): rsqc_decode_window::device_batch
    // a SAM text stream (rsqc_decode_begin_sam): the stages of rsqc_sam.hip instead of the BAM framing and parsing
    bool sam = false;
    size_t sam_cap = 0;                // the out_cap the SAM buffers below were sized for
    uint32_t sam_rec_cap = 0;
    DevBuf sam_ebits, sam_tbits, sam_segcnt, sam_segk0, sam_rtid, sam_nops, sam_st, sam_sc, sam_scratch, sam_slots, sam_names;
    SamRefTable sam_refs{};
    SamStatus *h_sam_st = nullptr;     // page-locked
    SamWindow pend_s{};
    uint64_t sam_line0 = 1;            // line number of the first byte of the next window (header lines counted)
    std::vector<std::string> sam_ref_names;
    std::vector<int32_t> sam_last_runs;  // rsqc_decode_end: runs of the last window and of the one that ended the last line
};

// --sort (rsqc_sort_begin / rsqc_sort_end, rsqc_sort_api.cpp): what has been collected, columns that grow by doubling
struct SortState {
    bool active = false;
    uint64_t n = 0, n_ops = 0, n_wide = 0, cap_n = 0, cap_ops = 0, cap_wide = 0, batches_in = 0;
    DevBuf core, aux, qh2, key, cigar, wide_index, wide_nm, wide_lq, wide_nc;
    DevBuf umi; uint64_t cap_umi = 0;                // rsqc_markdup_use_umi only: the records' UMI keys, 8 bytes each, released by the marking stage
    std::vector<uint64_t> batch_rec0, batch_pool0;   // first record / first operation of every collected batch
};

// --junctions (rsqc_junctions_begin / rsqc_junctions_end, rsqc_junction_api.cpp): the instances of the pass, three columns that grow by
// doubling to the host's bound; the finished table on the host
struct JunctionState {
    bool active = false, done = false;
    uint64_t cap = 0, cap0 = 0, bound = 0;             // instances the columns hold; the first size; half the operations submitted so far
    DevBuf key_hi, end, info, cursor;                  // cursor: u64 instances, u64 contributing records
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;   // around every batch's extraction
    std::vector<int32_t> tid, start, end_h;
    std::vector<uint32_t> reads, hq_reads, max_overhang;
    rsqc_junction_table table{};
};

// --mark-duplicates (rsqc_markdup_begin / rsqc_markdup_end / rsqc_markdup_verdicts, rsqc_markdup_api.cpp): the figures of the stage that
// rsqc_sort_end ran, the verdict column (one byte per record of the collection, in arrival order), one window of it on the host
struct MarkdupState {
    bool active = false, done = false;
    uint64_t n = 0;                                    // records of the collection the verdicts are for
    int passes_lo = 0, passes_hi = 0;                  // live radix passes of the two sort stages
    rsqc_markdup_info info{};
    bool use_umi = false;                              // rsqc_markdup_use_umi: the UMI key is part of the signature
    int passes_mapq = 0, passes_umi = 0;               // ... and the live passes of its two extra sort stages
    rsqc_markdup_umi_info umi_info{};
    uint32_t umi_edits = 0;                            // rsqc_markdup_umi_edits: 1 = UMIs one substitution apart are grouped before marking
    rsqc_markdup_umi_group_info group_info{};
    DevBuf verdict;
    std::vector<uint8_t> h_verdict;                    // the window of the last rsqc_markdup_verdicts
};

// --bedgraph (rsqc_track_begin / rsqc_track_end / rsqc_track_rows / rsqc_track_text, rsqc_track_api.cpp): the difference array of
// the pass (4 bytes per reference position, kept across rsqc_reset), the rows on the device (16 bytes each), one window on the host
struct TrackState {
    bool active = false, done = false, have_names = false, merge_later = false;
    int32_t n = 0;
    uint64_t total = 0;                                // slots of the difference array without the scan's extra one: sum of (length + 1)
    DevBuf diff, off, length, sums, names, name_off, counts, chunk_sum, totals, rows, linelen, text;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;   // around every batch's events kernel
    rsqc_track_info info{};
    std::vector<int32_t> h_tid;                        // the window of the last rsqc_track_rows
    std::vector<uint32_t> h_start, h_end, h_depth;
    HostBuf h_text;                                    // the window of the last rsqc_track_text
};

// What the stages over the track that follow a gene model hold alike (rsqc_genemodel_api.cpp): the model of the pass (12 bytes per
// segment) and the items of its launch plan, each stage its own
struct GeneStage {
    bool active = false, done = false;
    int32_t n_genes = 0;
    uint64_t n_items = 0;
    DevBuf seg_tid, seg_start, seg_end, items;
};

// --gene-body (rsqc_genebody_begin / rsqc_genebody_end / rsqc_genebody_sums, rsqc_genebody_api.cpp): 24 bytes per item, the sums on
// the device (800 bytes per gene), one window on the host
struct GenebodyState : GeneStage {
    DevBuf sums, total;
    rsqc_genebody_info info{};
    HostBuf h_sums;                                    // the window of the last rsqc_genebody_sums
};

// --tin (rsqc_tin_begin / rsqc_tin_end / rsqc_tin_rows, rsqc_tin_api.cpp): 20 bytes per item, 8 per gene, one partial per item and
// one row per gene on the device (24 bytes each), the rows on the host
struct TinState : GeneStage {
    DevBuf item_off, part, rows;
    rsqc_tin_info info{};
    HostBuf h_rows;                                    // every gene's row behind rsqc_tin_end
};

// What the stages behind every decode window hold alike (rsqc_window_stage_api.cpp): the tables and their scalar words on the device, the
// same in page-locked memory behind the stage's end, what the host added, the events around every window's kernel
struct WindowStage {
    bool active = false, done = false;
    DevBuf tab;
    HostBuf h_tab;
    uint64_t seen = 0;                                 // records of the pass's decode windows
    std::vector<uint64_t> added;                       // the stage's add: the words of the host's table once there is something, summed on the host
    uint64_t added_seen = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;   // around every window's kernel
};

// --cycles (rsqc_cycles_begin / rsqc_cycles_add / rsqc_cycles_end, rsqc_cycle_api.cpp): CYC_TABLE_WORDS of 64 bits
struct CycleState : WindowStage {
    rsqc_cycle_info info{};
};

// --mismatches (rsqc_mismatch_begin / rsqc_mismatch_add / rsqc_mismatch_end, rsqc_mismatch_api.cpp): the reference at four bits per base
// with a word offset and a length per contig -- kept across rsqc_reset, with the lengths it was packed for on the host --, and
// MM_TABLE_WORDS of 64 bits
struct MismatchState : WindowStage {
    bool have_ref = false;
    DevBuf ref_words, ref_off, ref_len;
    std::vector<uint64_t> ref_length;                  // the n lengths of the packed reference
    uint32_t min_mapq = 0;
    rsqc_mismatch_info info{};
};

// --alleles (rsqc_alleles_begin / rsqc_alleles_add / rsqc_alleles_end, rsqc_allele_api.cpp): the sites' positions and every contig's first
// site on the device (uploaded at every begin), AL_S_WORDS scalar words and the cells [site][8] behind them in one buffer, the same in
// page-locked memory (compacted to [site][7] behind rsqc_alleles_end); the host adds AL_S_WORDS + n_sites * 7 words
struct AlleleState : WindowStage {
    DevBuf pos, first;
    int32_t n_contigs = 0;
    uint32_t n_sites = 0, min_mapq = 0, min_baseq = 0;
    bool merge = false;                                // RSQC_ALLELE_MERGE at rsqc_alleles_begin
    rsqc_allele_info info{};
};

}  // namespace rsqc
using namespace rsqc;            // (every unit that sees this header is host code of the library)

struct rsqc_ctx {
    rsqc_params params{};
    int device = 0;
    hipStream_t stream = nullptr;
    std::string last_error;
    int sticky = 0;
    int k1_variant = 41, k1_grid = 256 * 20;  // workgroups of the per-read kernel (RSQC_K1_GRID overrides), set once at create: four rounds of five workgroups per CU

    // annotation (host copies needed at finalize)
    bool have_ann = false;
    int32_t n_ref = 0, n_contigs = 0, n_genes = 0, n_listed = 0, n_exons = 0;
    std::vector<uint32_t> exon_row_id;          // row -> exon id
    std::vector<DevBuf> ann_bufs;
    DevAnnotation dann{};
    DevParams dparams{};
    // K3 inputs
    const uint32_t *d_ge_off = nullptr, *d_ge_row = nullptr, *d_gene_cov_off = nullptr, *d_gene_coding = nullptr;
    const uint8_t *d_gene_flags = nullptr, *d_gene_owned = nullptr;   // owned by ann_bufs
    const uint32_t *d_gene_order = nullptr;
    uint32_t k3_large = 0, k3_medium = 0, k3_xlarge = 0, k3_le6144 = 0, k3_le3072 = 0, k3_le2048 = 0, k3_le1024 = 0;
    int stream_prio = 0, prio_side = 0;         // RSQC_STREAM_PRIO (rsqc_create)
    uint32_t n_exons_outside_gene = 0;          // of the annotation in use (rsqc_results.exons_outside_gene_row)
    hipEvent_t fin_e0 = nullptr, fin_e1 = nullptr;
    uint64_t cov_entries = 0;
    bool have_bed = false;

    // accumulators
    // one device arena holds every small result vector (single memset at reset, single D2H at finalize):
    // u64[3G+K] | u64 bias3,bias5[L] | f64 exon_acc[E] | f64 gmean,gstd,gcv[L] | f64 ecv[E] | u8 gvalid[L] | u8 ecv_valid[E] | u8 exon_hit[E] | misc[64]
    DevBuf d_arena, d_cov, d_ovf_index, d_tiles;
    DevBuf d_defer;                             // classify_ei_kernel's deferred list (per-workgroup regions, then the dense list): reused batch after batch (stream order)
    DevBuf d_ei_rank;                                   // rank table of the interval index
    char *h_arena = nullptr;                      // pinned host mirror
    size_t arena_bytes = 0, off_u64 = 0, off_exon = 0, off_gmean = 0, off_gstd = 0, off_gcv = 0, off_bias3 = 0,
           off_bias5 = 0, off_ecv = 0, off_gvalid = 0, off_ecvv = 0, off_ehit = 0, off_misc = 0;
    hipStream_t stream2 = nullptr, stream3 = nullptr, stream4 = nullptr;   // K3 (three size classes) runs beside K4
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join3 = nullptr, ev_join4 = nullptr, ev_retired = nullptr;
    DevAccum acc{};
    uint64_t tile_cap = 0;
    std::vector<PairBuf> pair_pool;
    std::vector<size_t> pairs_in_flight;        // indices into pair_pool, submission order (batches not retired yet)
    Arena pair_arena, frag_arena, gc_arena;     // what the retired batches emitted
    DevBuf d_arena_count;                       // u32: pair_arena.used for the K4 launch over the arena
    std::vector<DevBuf> parked;                 // outgrown arena columns, freed at the next synchronisation point
    DevBuf d_table, d_tab_off, d_tab_cap;
    std::vector<FragBuf> frag_pool;
    std::vector<size_t> frags_in_flight;
    uint32_t frag_remaining = 0;
    // --fasta
    bool have_ref = false;
    DevBuf d_ref_bits, d_ref_off, d_ref_len, d_gc_bins, d_exon_gc;
    DevReference dref{};
    std::vector<GcBuf> gc_pool;
    std::vector<size_t> gcs_in_flight;
    std::vector<uint64_t> h_gc;                 // [RSQC_GC_BINS + 1]
    std::vector<double> h_exon_gc;              // by exon id
    SortScratch gc_scratch, frag_scratch;
    uint32_t frag_kept = 0;                     // samples run_fragment_sizes left in frag_scratch (k1 / v1)
    // K3 outputs
    bool finalized = false;

    // batches
    std::vector<UploadedBatch *> resident;
    std::vector<UploadedBatch *> transient;     // owned by submit(), freed at wait()
    uint64_t next_record_base = 0;
    bool have_ranges = false;                   // a batch of several file ranges was submitted in this pass: Read Length is composed on the host
    bool have_composed_rl = false; int32_t composed_rl = 0;
    bool early_copied = false;                  // run_finalize_kernels copied everything but geneFragmentCounts and the status words beside the fragment kernels
    std::vector<uint32_t> h_rl_arm;
    int name_mode = -1;                         // -1 no batch yet in this pass; 0 batches without qhash2 (64-bit names); 1 with (96-bit names)
    // per submitted batch: file index of its first record and the Read-Length transfer function the KR kernel leaves
    // on the device (rsqc_shard_info)
    std::vector<uint64_t> batch_file_index, batch_records;
    DevBuf d_rl_summary;
    uint32_t *h_rl_raw = nullptr;               // page-locked (a copy into pageable memory would hold the host until the coverage kernel ahead of it ended)
    size_t h_rl_raw_cap = 0;                    // ... words
    std::vector<uint32_t> h_rl_offset, h_rl_span;
    std::vector<int32_t> h_rl_state;
    std::vector<uint64_t> h_sample_file;        // fragment-size samples kept by this shard (first N by file index), ascending
    std::vector<uint32_t> h_sample_size;

    // timing
    std::vector<std::pair<hipEvent_t, hipEvent_t>> k1_events, h2d_events, long_events;
    std::vector<DevBuf> upload_pool;            // device buffers of retired transient uploads
    std::vector<hipEvent_t> event_pool;
    rsqc_timing timing{};

    DecodeState dec;
    SortState sort;
    JunctionState junc;
    TrackState track;
    GenebodyState genebody;
    TinState tin;
    CycleState cyc;
    MismatchState mm;
    AlleleState al;
    MarkdupState markdup;

    // host results
    std::vector<uint64_t> h_fcount;
    std::vector<int64_t> h_fsize;
    rsqc_results results{};
};

#define HIP_TRY(c, expr)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail((c), RSQC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

namespace rsqc {

int fail(rsqc_ctx *c, int code, const std::string &msg);
int dev_alloc(rsqc_ctx *c, DevBuf &b, size_t bytes, bool zero);
// a buffer of at least `bytes` that grows only (its content is lost when it grows).  false: there is no such memory -- the HIP error
// is cleared and the buffer is empty; the caller composes the text
bool dev_reserve(DevBuf &b, size_t bytes);
bool host_reserve(HostBuf &b, size_t bytes);
hipEvent_t get_event(rsqc_ctx *c);
int resolve_events(rsqc_ctx *c);
// device buffer of at least `bytes` from the context's pool of retired upload buffers (smallest that fits), or empty
DevBuf take_pooled(rsqc_ctx *c, size_t bytes);
void free_batch(UploadedBatch *u);
// a transient batch whose kernels have completed: keep its device buffers for the next rsqc_submit
void retire_batch(rsqc_ctx *c, UploadedBatch *u);
// n entries of the columns src[] appended to the arena (grown when it has to be), on stream s
int arena_append(rsqc_ctx *c, Arena &a, const void *const *src, uint32_t n, hipStream_t s);
void free_parked(rsqc_ctx *c);                 // caller: the stream has been synchronised
int retire_completed(rsqc_ctx *c, bool all);
int run_batch(rsqc_ctx *c, UploadedBatch *u);
const char *device_error_text(int err);
std::string device_error_message(rsqc_ctx *c, int err);      // ... naming the cause where the device left one (stream idle)
// collecting mode: the batch's records are appended to the collection instead of being run (rsqc_sort_api.cpp)
int sort_append(rsqc_ctx *c, UploadedBatch *u);
void sort_drop(rsqc_ctx *c);                   // leaves the collecting mode and frees the collection (hipFree waits for the device)
// --mark-duplicates: the stage at the head of rsqc_sort_end, on the complete collection (rsqc_markdup_api.cpp)
int markdup_run(rsqc_ctx *c);
void markdup_drop(rsqc_ctx *c);                // ends the mode and frees the verdict column
// --junctions: the batch's instances appended to the collection, on the main stream (rsqc_junction_api.cpp)
int junction_extract(rsqc_ctx *c, const UploadedBatch *u, const DevBatch &d);
void junction_drop(rsqc_ctx *c, bool free_buffers);   // ends the mode and forgets the instances
// --bedgraph: the batch's coverage events added to the difference array, on the main stream (rsqc_track_api.cpp)
int track_events(rsqc_ctx *c, const UploadedBatch *u, const DevBatch &d);
void track_drop(rsqc_ctx *c, bool free_buffers);      // ends the mode and forgets the track
// --gene-body: the stage behind rsqc_track_end (rsqc_genebody_api.cpp)
void genebody_drop(rsqc_ctx *c, bool free_buffers);   // ends the mode and forgets the model and the sums
// --tin: the stage behind rsqc_track_end (rsqc_tin_api.cpp)
void tin_drop(rsqc_ctx *c, bool free_buffers);        // ends the mode and forgets the model and the rows
// --cycles, --mismatches, --alleles (rsqc_cycle_api.cpp, rsqc_mismatch_api.cpp, rsqc_allele_api.cpp).  launch: the window's kernel on the main
// stream (sam: W is pend_s.W); drop: ends the mode and forgets the counts; free_buffers: the tables too, and the packed reference / the sites
void cycle_launch(rsqc_ctx *c, const DecodeWindow &W, const SamWindow *S);
void cycle_drop(rsqc_ctx *c, bool free_buffers);
void mismatch_launch(rsqc_ctx *c, const DecodeWindow &W, const SamWindow *S);
void mismatch_drop(rsqc_ctx *c, bool free_buffers);
void alleles_launch(rsqc_ctx *c, const DecodeWindow &W, const SamWindow *S);
void alleles_drop(rsqc_ctx *c, bool free_buffers);
// what the three have in common (rsqc_window_stage_api.cpp), and the one list of them, walked in the order of the kernels behind a
// window: n_rec records submitted from a window; the stages' kernels behind its parse stage, each between a pair of events; every stage
// dropped (free_inputs: the stages that were given a reference or sites at their begin free all they hold, whatever free_tables says)
void window_stages_seen(rsqc_ctx *c, uint64_t n_rec);
int window_stages_launch(rsqc_ctx *c, const DecodeWindow &W, const SamWindow *S);
void window_stages_drop(rsqc_ctx *c, bool free_tables, bool free_inputs);
// N: the stage's public calls and its noun, for the texts.  The order of the calls at a begin; the device and the page-locked table
// reserved and the device one cleared, the caller's capacity texts; the common part of a drop; an add's guards, and the words the host
// has added so far (sized at the first add); an end (the order of the calls, then once a pass: `bytes` read back, the events'
// milliseconds handed to `finish`, which sums in what the host added -- window_sum_added -- fills the info and checks the table)
struct WindowNames { const char *begin, *add, *end, *noun; };
int window_begin_check(rsqc_ctx *c, const WindowStage &S, const WindowNames &N);
int window_tables(rsqc_ctx *c, WindowStage &S, size_t bytes, const std::string &no_device, const std::string &no_host);
void window_drop(rsqc_ctx *c, WindowStage &S, bool free_tables);
int window_add_check(rsqc_ctx *c, const WindowStage &S, const WindowNames &N);
uint64_t *window_added(WindowStage &S, size_t words);
int window_end(rsqc_ctx *c, WindowStage &S, const WindowNames &N, size_t bytes, int (*finish)(rsqc_ctx *, double ms));
void window_sum_added(const WindowStage &S, uint64_t *h, size_t words);
// what the two have in common (rsqc_genemodel_api.cpp).  who: the public call, for the texts; what: the stage, as the texts name it.
// A begin behind its own argument checks (the order of the calls, the model against the track's contigs; n_seg: its segments), the
// figures its capacity texts end with, the model and the items reserved and copied (stream order: the caller synchronises); an end
// (the order of the calls, then `run` once a pass: a run that fails leaves the pass void until rsqc_reset)
int gene_begin_check(rsqc_ctx *c, const char *who, const char *what, const GeneStage &G, int32_t n_genes, const uint32_t *seg_off, const int32_t *seg_tid,
                     const uint32_t *seg_start, const uint32_t *seg_end, size_t *n_seg);
std::string gene_sizes(int32_t n_genes, size_t n_seg, size_t n_items);
int gene_reserve(rsqc_ctx *c, const char *who, DevBuf &b, size_t bytes, const char *what, const std::string &sizes);
int gene_upload(rsqc_ctx *c, const char *who, GeneStage &G, const std::string &sizes, int32_t n_genes, size_t n_seg, const int32_t *seg_tid,
                const uint32_t *seg_start, const uint32_t *seg_end, const void *items, size_t n_items, size_t item_bytes);
void gene_drop(GeneStage &G, bool free_buffers);
int gene_end(rsqc_ctx *c, GeneStage &G, const char *begin, const char *end, int (*run)(rsqc_ctx *));
// `work` enqueued between a pair of events and `after` behind it (the copies of what it left), the stream synchronised: its milliseconds
template <class Work, class After>
int run_timed(rsqc_ctx *c, double *ms, Work work, After after) {
    hipEvent_t e0 = get_event(c), e1 = get_event(c);
    HIP_TRY(c, hipEventRecord(e0, c->stream));
    work();
    HIP_TRY(c, hipEventRecord(e1, c->stream));
    if (int rc = after()) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    float f = 0.f;
    *ms = hipEventElapsedTime(&f, e0, e1) == hipSuccess ? f : 0;
    c->event_pool.push_back(e0); c->event_pool.push_back(e1);
    return 0;
}

template <class T>
int upload(rsqc_ctx *c, std::vector<DevBuf> &owner, const T *host, size_t n, const T **out, bool from_pool = false) {
    const size_t bytes = n * sizeof(T);
    // 32 bytes of slack: kernels load a few entries past the end with unconditional, ignored loads
    DevBuf b = from_pool ? take_pooled(c, bytes + 32) : DevBuf{};
    if (!b.p) { HIP_TRY(c, hipMalloc(&b.p, bytes + 32)); b.bytes = bytes + 32; }
    if (bytes) HIP_TRY(c, hipMemcpyAsync(b.p, host, bytes, hipMemcpyHostToDevice, c->stream));
    owner.push_back(b);
    *out = (const T *)b.p;
    return 0;
}

}  // namespace rsqc
