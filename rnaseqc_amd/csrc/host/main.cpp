// main.cpp -- `rnaseqc [OPTIONS] gtf bam output` (or `--bam-list=FILE gtf output`, a cohort): the reference's command line (flag table
// src/RNASeQC.cpp:39-65, defaults :87-100, exit codes :678-766) in front of the HIP hot path.
// Host side only: GTF/BED ingest, BAM decode into SoA batches, report writers.  Every per-record
// computation happens on the GPU through the C ABI (include/rnaseqc_amd.h); without a GPU the
// program exits with code 10.
#include <signal.h>
#include <sys/stat.h>
#include <unistd.h>

#include <memory>
#include <sys/types.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <future>
#include <map>
#include <iostream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "bam.hpp"
#include "bgzf_feed.hpp"
#include "fasta.hpp"
#include "gtf.hpp"
#include "report.hpp"
#include "sam_feed.hpp"
#include "../rsqc_rl_compose.h"

using namespace rsqc_host;

namespace {

const char *VERSION = "RNASeQC 2.4.3";

struct ParseError : std::runtime_error { using std::runtime_error::runtime_error; };          // exit 5
struct ValidationError : std::runtime_error { using std::runtime_error::runtime_error; };    // exit 6
struct Help {};

struct Options {
    std::vector<std::string> positional;
    std::string sample, bed, fasta, stranded, chimeric_tag = "ch";
    bool has_sample = false, has_bed = false, has_fasta = false, has_stranded = false;
    bool legacy = false, exclude_chimeric = false, unpaired = false, rpkm = false, coverage = false, version = false;
    int verbosity = 0;
    long chimeric_distance = 2000000; unsigned long fragment_samples = 1000000, mapq = 255, base_mismatch = 6;
    bool has_mapq = false;
    long bias_offset = 0, bias_window = 100; unsigned long bias_gene_length = 200, coverage_mask = 500, detection = 5;
    std::vector<std::string> tags;
    int gpus = 0;                      // --gpus (extension): GPUs to shard the BAM over by contig; 0 = RSQC_GPUS or 1
    std::string bam_list; bool has_bam_list = false;   // --bam-list (extension): a cohort, the positionals are `gtf output`
    bool bedgraph = false;             // --bedgraph (extension): the per-base coverage track, <sample>.coverage.bedgraph (rsqc_track_begin / _end / _text)
    bool gene_body = false;            // --gene-body (extension): coverage along the gene body in 100 bins, <sample>.gene_body.tsv (rsqc_genebody_begin / _end / _sums; turns the track on)
    bool tin = false;                  // --tin (extension): per-gene transcript integrity from the coverage track, <sample>.tin.tsv and <sample>.tin_summary.tsv (rsqc_tin_begin / _end / _rows; turns the track on)
    bool cycles = false;               // --cycles (extension): base quality and composition by read cycle, <sample>.cycle_bases.tsv and <sample>.cycle_quality.tsv (rsqc_cycles_begin / _add / _end)
    // --mismatches (extension; needs --fasta): errors by read cycle against the reference, <sample>.mismatch_cycles.tsv, .mismatch_types.tsv and
    // .mismatch_quality.tsv (rsqc_mismatch_begin / _add / _end); --mismatches-mapq=N: the least mapping quality of a counted record, as given
    bool mismatches = false, has_mismatches_mapq = false; long mismatches_mapq = 0;
    // --alleles=FILE (extension): base counts at the single-base sites of a VCF, <sample>.allele_counts.tsv (rsqc_alleles_begin / _add / _end);
    // --allele-mapq=N / --allele-baseq=N: the least mapping quality of a counted record and the least quality of a counted base, as given
    bool has_alleles = false, has_allele_mapq = false, has_allele_baseq = false; std::string alleles; long allele_mapq = 0, allele_baseq = 0;
    bool junctions = false;            // --junctions (extension): reads per splice junction, <sample>.junctions.tsv (rsqc_junctions_begin / rsqc_junctions_end)
    bool mark_duplicates = false;      // --mark-duplicates (extension, implies --sort): flag 0x400 rewritten on the GPU before the records are counted (rsqc_markdup_begin / rsqc_markdup_end)
    // --umi-tag=XX / --umi-qname[=C] (extensions, each implies --mark-duplicates): the UMI joins the duplicate signature (rsqc_markdup_use_umi);
    // the tag's two letters / the separator in front of the UMI at the end of the read name, as given (checked at validation)
    bool has_umi_tag = false, has_umi_qname = false; std::string umi_tag, umi_sep = "_";
    // --umi-edits=N (extension; with one of the two above): 1 groups UMIs one substitution apart before marking (rsqc_markdup_umi_edits); as given
    bool has_umi_edits = false; std::string umi_edits = "0";
    bool sort = false;                 // --sort (extension): input in any order, put in coordinate order on the GPU (rsqc_sort_begin / rsqc_sort_end)
};

void usage(std::ostream &o) {
    o << "  rnaseqc {OPTIONS} [gtf] [bam] [output]\n\n    " << VERSION << "\n\n  OPTIONS:\n\n"
         "      -h, --help                        Display this message and quit\n"
         "      --version                         Display the version and quit\n"
         "      gtf                               The input GTF file containing features to check the bam against\n"
         "      bam                               The input SAM/BAM file containing reads to process\n"
         "      output                            Output directory\n"
         "      -s[sample], --sample=[sample]     The name of the current sample.  Default: The bam's filename\n"
         "      --bed=[BEDFILE]                   Optional input BED file containing non-overlapping exons used for fragment size calculations\n"
         "      --fasta=[fasta]                   Optional input FASTA (with .fai index): enables the GC-content statistics (CRAM input is not supported)\n"
         "      --chimeric-distance=[DISTANCE]    Maximum accepted distance between read mates. Default: 2000000 [bp]\n"
         "      --fragment-samples=[SAMPLES]      Number of fragment size samples. Default: 1000000\n"
         "      -q[QUALITY], --mapping-quality=[QUALITY]  Lower bound on read quality for exon coverage counting. Default: 255\n"
         "      --base-mismatch=[MISMATCHES]      Maximum number of allowed mismatches. Default: 6\n"
         "      --offset=[OFFSET]                 Offset into the gene for the 3' and 5' windows. Default: 0 [bp]\n"
         "      --window-size=[SIZE]              Size of the 3' and 5' windows. Default: 100 [bp]\n"
         "      --gene-length=[LENGTH]            Minimum size of a gene for bias calculation. Default: 200 [bp]\n"
         "      --legacy                          Use legacy counting rules.  Gene and exon counts match output of RNA-SeQC 1.1.9\n"
         "      --stranded=[stranded]             'RF', 'rf', 'FR', or 'fr'\n"
         "      -v, --verbose                     Give some feedback; twice for progress updates\n"
         "      -t[TAG...], --tag=[TAG...]        Filter out reads with the specified tag\n"
         "      --chimeric-tag=[TAG]              Reads marked with this tag are chimeric. Default: ch\n"
         "      --exclude-chimeric                Exclude chimeric reads from the read counts\n"
         "      -u, --unpaired                    Allow unpaired reads to be quantified\n"
         "      --rpkm                            Output gene RPKM values instead of TPMs\n"
         "      --coverage                        Write per-transcript coverage statistics to a table\n"
         "      --coverage-mask=[SIZE]            Bases masked at both transcript ends. Default: 500bp\n"
         "      -d[threshold], --detection-threshold=[threshold]  Counts to call a gene detected. Default: 5 reads\n"
         "      --gpus=[N]                        (extension) Shard the BAM by contig over N GPUs of this node; needs [bam].bai. Default: 1\n"
         "      --bam-list=[FILE]                 (extension) A cohort on one GPU: FILE lists one input per line, path[<TAB>sample]; the positionals are [gtf] [output]\n"
         "      --sort                            (extension) Accept input in any order: the records are put in coordinate order on the GPU before they are counted\n"
         "      --mark-duplicates                 (extension) Flag duplicate fragments on the GPU before they are counted: implies --sort, replaces the input's 0x400 flags (one GPU, one input)\n"
         "      --umi-tag=[XX]                    (extension) UMI-aware --mark-duplicates (implied): the UMI is the Z value of aux tag XX (e.g. RX); exact match, the anchor's UMI, 31 bases at most, N voids it\n"
         "      --umi-qname=[C]                   (extension) The same with the UMI taken from the read name, behind its last C. Default: _ (use : for bcl-convert names)\n"
         "      --umi-edits=[N]                   (extension) With --umi-tag / --umi-qname: 1 merges UMIs of one position that are one substitution apart (towards the higher count, count >= 2 x - 1) before marking. Default: 0, exact match\n"
         "      --junctions                       (extension) Count reads per splice junction on the GPU and write [sample].junctions.tsv (one GPU)\n"
         "      --bedgraph                        (extension) Build the per-base coverage track on the GPU and write [sample].coverage.bedgraph (one GPU; needs LN in the header)\n"
         "      --gene-body                       (extension) Sum the coverage along every gene's body, 5' to 3' in 100 bins, on the GPU and write [sample].gene_body.tsv (one GPU; needs LN in the header)\n"
         "      --tin                             (extension) Measure every gene's transcript integrity (TIN: the evenness of its coverage) on the GPU and write [sample].tin.tsv and [sample].tin_summary.tsv (one GPU; needs LN in the header)\n"
         "      --cycles                          (extension) Count base composition and base quality by read cycle on the GPU, from the SEQ and QUAL the decode already holds, and write [sample].cycle_bases.tsv and [sample].cycle_quality.tsv (one GPU)\n"
         "      --mismatches                      (extension) Walk every record's CIGAR over its SEQ, QUAL and the --fasta reference on the GPU and write [sample].mismatch_cycles.tsv, [sample].mismatch_types.tsv and [sample].mismatch_quality.tsv (one GPU; needs --fasta)\n"
         "      --mismatches-mapq=[N]             (extension) With --mismatches: the least mapping quality of a counted record, 0..255. Default: 0 (not -q)\n"
         "      --alleles=[VCF]                   (extension) Count on the GPU which base every record shows at the single-base sites of VCF (plain, gzip or bgzip) and write [sample].allele_counts.tsv (one GPU)\n"
         "      --allele-mapq=[N]                 (extension) With --alleles: the least mapping quality of a counted record, 0..255. Default: 0 (not -q)\n"
         "      --allele-baseq=[N]                (extension) With --alleles: the least base quality of a counted base, 0..93; lower ones count as low_baseq. Default: 0\n";
}

long to_long(const std::string &flag, const std::string &v) {
    char *e = nullptr;
    const long x = strtol(v.c_str(), &e, 10);
    if (v.empty() || (e && *e)) throw ParseError("Argument '" + flag + "' received invalid value type '" + v + "'");
    return x;
}
unsigned long to_ulong(const std::string &flag, const std::string &v) {
    char *e = nullptr;
    if (v.empty() || v[0] == '-') throw ParseError("Argument '" + flag + "' received invalid value type '" + v + "'");
    const unsigned long x = strtoul(v.c_str(), &e, 10);
    if (e && *e) throw ParseError("Argument '" + flag + "' received invalid value type '" + v + "'");
    return x;
}

Options parse(int argc, char **argv) {
    Options o;
    bool only_positional = false;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        if (only_positional || a.size() < 2 || a[0] != '-') { o.positional.push_back(a); continue; }
        if (a == "--") { only_positional = true; continue; }
        std::string name, value; bool has_value = false;
        if (a[1] == '-') {
            const size_t eq = a.find('=');
            name = a.substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
            if (eq != std::string::npos) { value = a.substr(eq + 1); has_value = true; }
        } else {
            // short flags: -v, -vv, -u, -h may be bundled; -s/-q/-t/-d take the rest of the token or the next one
            size_t k = 1;
            bool consumed = false;
            while (k < a.size() && !consumed) {
                const char c = a[k];
                if (c == 'v') { ++o.verbosity; ++k; }
                else if (c == 'u') { o.unpaired = true; ++k; }
                else if (c == 'h') throw Help();
                else if (c == 's' || c == 'q' || c == 't' || c == 'd') {
                    std::string v = a.substr(k + 1);
                    if (v.empty()) { if (i + 1 >= argc) throw ParseError(std::string("Flag '") + c + "' requires an argument but received none"); v = argv[++i]; }
                    const std::string f(1, c);
                    if (c == 's') { o.sample = v; o.has_sample = true; }
                    else if (c == 'q') { o.mapq = to_ulong(f, v); o.has_mapq = true; }
                    else if (c == 't') o.tags.push_back(v);
                    else o.detection = to_ulong(f, v);
                    consumed = true;
                } else throw ParseError(std::string("Flag could not be matched: '") + c + "'");
            }
            continue;
        }
        auto need = [&]() -> std::string {
            if (has_value) return value;
            if (i + 1 >= argc) throw ParseError("Flag '" + name + "' requires an argument but received none");
            return std::string(argv[++i]);
        };
        if (name == "help") throw Help();
        else if (name == "version") o.version = true;
        else if (name == "sample") { o.sample = need(); o.has_sample = true; }
        else if (name == "bed") { o.bed = need(); o.has_bed = true; }
        else if (name == "fasta") { o.fasta = need(); o.has_fasta = true; }
        else if (name == "chimeric-distance") o.chimeric_distance = to_long(name, need());
        else if (name == "fragment-samples") o.fragment_samples = to_ulong(name, need());
        else if (name == "mapping-quality") { o.mapq = to_ulong(name, need()); o.has_mapq = true; }
        else if (name == "base-mismatch") o.base_mismatch = to_ulong(name, need());
        else if (name == "offset") o.bias_offset = to_long(name, need());
        else if (name == "window-size") o.bias_window = to_long(name, need());
        else if (name == "gene-length") o.bias_gene_length = to_ulong(name, need());
        else if (name == "legacy") o.legacy = true;
        else if (name == "stranded") { o.stranded = need(); o.has_stranded = true; }
        else if (name == "verbose") ++o.verbosity;
        else if (name == "tag") o.tags.push_back(need());
        else if (name == "chimeric-tag") o.chimeric_tag = need();
        else if (name == "exclude-chimeric") o.exclude_chimeric = true;
        else if (name == "unpaired") o.unpaired = true;
        else if (name == "rpkm") o.rpkm = true;
        else if (name == "coverage") o.coverage = true;
        else if (name == "gpus") o.gpus = (int)to_ulong(name, need());
        else if (name == "bam-list") { o.bam_list = need(); o.has_bam_list = true; }
        else if (name == "sort") o.sort = true;
        else if (name == "mark-duplicates") o.mark_duplicates = o.sort = true;
        else if (name == "umi-tag") { o.umi_tag = need(); o.has_umi_tag = o.mark_duplicates = o.sort = true; }
        else if (name == "umi-qname") { if (has_value) o.umi_sep = value; o.has_umi_qname = o.mark_duplicates = o.sort = true; }
        else if (name == "umi-edits") { o.umi_edits = need(); o.has_umi_edits = true; }
        else if (name == "junctions") o.junctions = true;
        else if (name == "bedgraph") o.bedgraph = true;
        else if (name == "gene-body") o.gene_body = true;
        else if (name == "tin") o.tin = true;
        else if (name == "cycles") o.cycles = true;
        else if (name == "alleles") { o.alleles = need(); o.has_alleles = true; }
        else if (name == "allele-mapq") { o.allele_mapq = to_long(name, need()); o.has_allele_mapq = true; }
        else if (name == "allele-baseq") { o.allele_baseq = to_long(name, need()); o.has_allele_baseq = true; }
        else if (name == "mismatches") o.mismatches = true;
        else if (name == "mismatches-mapq") { o.mismatches_mapq = to_long(name, need()); o.has_mismatches_mapq = true; }
        else if (name == "coverage-mask") o.coverage_mask = to_ulong(name, need());
        else if (name == "detection-threshold") o.detection = to_ulong(name, need());
        else throw ParseError("Flag could not be matched: " + name);
    }
    return o;
}

bool make_dirs(const std::string &path) {          // boost::filesystem::create_directories
    std::string cur;
    for (size_t i = 0; i <= path.size(); ++i) {
        if (i == path.size() || path[i] == '/') {
            if (!cur.empty() && cur != "/") {
                struct stat st;
                if (stat(cur.c_str(), &st) != 0) { if (mkdir(cur.c_str(), 0777) != 0) return false; }
                else if (!S_ISDIR(st.st_mode)) return false;
            }
        }
        if (i < path.size()) cur += path[i];
    }
    return true;
}

std::string basename_of(const std::string &p) {
    const size_t s = p.find_last_of('/');
    return s == std::string::npos ? p : p.substr(s + 1);
}

}  // namespace

// ---- one process, several GPUs: the BAM sharded by contig ------------------------------------------
// Every GPU holds the whole annotation and owns a set of contigs (longest-processing-time packing on the index's record
// counts); a host thread per GPU reads ITS contigs through the BAM index (BamReader::seek) and feeds its context; at
// end of file the contexts' result ranges are summed onto the first GPU (rsqc_reduce_peer: peer copies over xGMI), and the
// two order-dependent outputs are composed on the host from the shards' summaries (rsqc_shard_summary).
struct Shard {
    rsqc_ctx *gpu = nullptr; int device = 0;
    std::vector<int> contigs; bool tail = false;
    uint64_t load = 0, n_records = 0;
    int rc = RSQC_OK; std::string error; bool unsorted = false; std::vector<std::string> bad_refid;
};

constexpr int kFileIndexShift = 36;      // virtual file index of a batch: (contig << 36) + records of the contig before it

// ---- device decode (rsqc_decode_*): the default.  RSQC_DECODE=host keeps inflate + record parsing on the CPU threads.
// The device path reads the file with pread through the block feeder, which needs a regular file: a FIFO, /dev/stdin or a
// process substitution is streamed by the host reader instead (as every input was before the device decode existed).
bool device_decode_wanted(bool input_is_stream) {
    if (input_is_stream) return false;
    const char *e = getenv("RSQC_DECODE");
    return !(e && (!strcmp(e, "host") || !strcmp(e, "cpu")));
}
rsqc_decode_params decode_params(const Options &o, int n_ref, uint64_t file_index_base) {
    rsqc_decode_params dp{};
    dp.n_ref = n_ref;
    if (o.chimeric_tag.size() == 2) { dp.has_chimeric_tag = 1; dp.chimeric_tag[0] = o.chimeric_tag[0]; dp.chimeric_tag[1] = o.chimeric_tag[1]; }
    for (size_t k = 0; k < o.tags.size() && k < RSQC_MAX_FILTER_TAGS; ++k)
        if (o.tags[k].size() == 2) { dp.filter_tag[k][0] = o.tags[k][0]; dp.filter_tag[k][1] = o.tags[k][1]; }   // (other lengths never match)
    dp.file_index_base = file_index_base;
    if (o.has_umi_tag) { dp.umi_source = RSQC_UMI_SOURCE_TAG; dp.umi_tag[0] = o.umi_tag[0]; dp.umi_tag[1] = o.umi_tag[1]; }      // (lengths checked at validation)
    if (o.has_umi_qname) { dp.umi_source = RSQC_UMI_SOURCE_QNAME; dp.umi_sep = o.umi_sep[0]; }
    return dp;
}
// inflated bytes a call of decode_range can hold: what the device's window buffers are sized for, once (rsqc_decode_begin)
uint64_t decode_reserve_bytes(uint64_t file_size) {
    const uint64_t max_out = getenv("RSQC_DECODE_MAX_OUT") ? (uint64_t)atoll(getenv("RSQC_DECODE_MAX_OUT")) : (uint64_t)1024 << 20;
    return std::min<uint64_t>(max_out + (1u << 20), file_size * 16 + (1u << 20));
}
// One stream of BGZF blocks [voff_beg, voff_end) through the GPU: the feeder reads and frames the blocks, every chunk is one
// rsqc_decode_submit.  on_window sees what each call decoded.  Returns an RSQC_* code; info describes the whole stream.
// sam_names: the @SQ names of a BGZF-compressed SAM (the stream goes through the device SAM stages, rsqc_decode_begin_sam)
template <class F>
int decode_range(rsqc_ctx *gpu, BgzfFeeder &feed, const rsqc_decode_params &dp, uint64_t voff_beg, uint64_t voff_end, rsqc_decode_info &info, F &&on_window,
                 const char *const *sam_names = nullptr) {
    // Calls are large on purpose: the inflate kernel runs one wave per BGZF block, twenty waves per CU = 5 120 on the chip, and a
    // call's time is that of its LAST block: a call of 5 300 blocks (128 MB of a file compressed 3 x, round 4's chunk) runs 180 of
    // them on an empty chip.  Up to 1 GB of inflated data = 16 000 blocks per call whatever the file's compression (the feeder reads
    // what that takes, up to 512 MB of file), the device buffers sized for that once (profiles/r5_decode_chunk_sweep.txt).
    // (RSQC_DECODE_CHUNK / RSQC_DECODE_MAX_OUT: compressed bytes read per call at most / inflated bytes per call -- the tests use
    //  small values so that records straddle many calls)
    const size_t chunk = getenv("RSQC_DECODE_CHUNK") ? (size_t)atoll(getenv("RSQC_DECODE_CHUNK")) : (size_t)512 << 20;
    const uint64_t max_out = getenv("RSQC_DECODE_MAX_OUT") ? (uint64_t)atoll(getenv("RSQC_DECODE_MAX_OUT")) : (uint64_t)1024 << 20;
    rsqc_decode_params dpr = dp;
    dpr.pipelined = 1;                          // a call's records are reported by the call after it (the last by rsqc_decode_end)
    dpr.reserve_inflated_bytes = decode_reserve_bytes(feed.file_size());
    int rc = sam_names ? rsqc_decode_begin_sam(gpu, &dpr, sam_names) : rsqc_decode_begin(gpu, &dpr);
    if (rc != RSQC_OK) return rc;
    const bool prof = getenv("RSQC_DECODE_PROFILE") != nullptr;
    double t_feed = 0;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto t0 = now();
    feed.start(voff_beg, voff_end, chunk, max_out);
    for (;;) {
        auto tf = now();
        BgzfFeeder::Chunk *ch = feed.next();
        t_feed += std::chrono::duration<double, std::milli>(now() - tf).count();
        if (!ch) break;
        if (ch->blocks.empty()) continue;
        rsqc_decode_window w{};
        rc = rsqc_decode_submit(gpu, ch->data, ch->total_bytes, ch->blocks.data(), (uint32_t)ch->blocks.size(), ch->skip, ch->limit, &w);
        if (rc != RSQC_OK) { rsqc_decode_info dropped{}; (void)rsqc_decode_end(gpu, &dropped); return rc; }
        if (w.n_records) on_window(w);
    }
    if (prof) fprintf(stderr, "[decode] host: CPU share of the inflate work at the end %.2f; %.1f ms waiting for file chunks of %.1f ms in the range\n", feed.cpu_share(), t_feed, std::chrono::duration<double, std::milli>(now() - t0).count());
    rc = rsqc_decode_end(gpu, &info);
    if (rc == RSQC_OK && info.last.n_records) on_window(info.last);
    return rc;
}

void shard_worker(Shard &sh, const std::string &bam_path, const Options &o, int threads, const std::vector<BamReader::ContigRange> &index,
                  int n_ref, uint64_t tail_voff, size_t BATCH, BgzfFeeder *device_feed) {
    try {
        if (device_feed) {                                             // device decode: the shard's feeder, opened and page-locked by the caller
            BgzfFeeder &feed = *device_feed;
            feed.read_threads = std::max(1, threads / 4);
            std::vector<int> ranges = sh.contigs;
            if (sh.tail) ranges.push_back(n_ref);
            for (int c : ranges) {
                const bool is_tail = c == n_ref;
                rsqc_decode_info di{};
                bool stale = false;
                sh.rc = decode_range(sh.gpu, feed, decode_params(o, n_ref, (uint64_t)c << kFileIndexShift), is_tail ? tail_voff : index[(size_t)c].beg,
                                     is_tail ? 0 : index[(size_t)c].end, di, [&](const rsqc_decode_window &w) {
                                         sh.n_records += w.n_records;
                                         for (uint32_t k = 0; k < w.n_runs; ++k) if (is_tail ? w.run_tid[k] >= 0 : w.run_tid[k] != c) stale = true;
                                     });
                if (sh.rc != RSQC_OK) { sh.error = rsqc_last_error(sh.gpu); return; }
                if (stale) { sh.rc = RSQC_ERR_ARG; sh.error = is_tail ? "placed records behind the last indexed contig: stale index?" : "records of another contig inside an indexed range: stale index?"; return; }
                if (di.unsorted) sh.unsorted = true;
                for (int k = 0; k < di.n_bad_refid && k < 64; ++k) if (sh.bad_refid.size() < 64) sh.bad_refid.push_back(di.bad_refid[k]);
            }
            sh.rc = rsqc_finalize_device(sh.gpu);
            if (sh.rc != RSQC_OK) sh.error = rsqc_last_error(sh.gpu);
            return;
        }
        HostBatch bufs[2];
        for (auto &hb : bufs) { hb.core.use_pinned(true); hb.aux.use_pinned(true); hb.qh2.use_pinned(true); hb.cigar.use_pinned(true); hb.core.reserve(BATCH); hb.aux.reserve(BATCH); hb.qh2.reserve(BATCH); hb.cigar.reserve(BATCH * 2); }
        int cur = 0; bool in_flight = false;
        std::vector<int> ranges = sh.contigs;
        if (sh.tail) ranges.push_back(n_ref);                          // the unplaced records behind the last contig
        for (int c : ranges) {
            BamReader bam;
            bam.set_threads(threads);
            if (!bam.open(bam_path)) { sh.rc = RSQC_ERR_ARG; sh.error = "Unable to open BAM file: " + bam_path; return; }
            bam.set_tags(o.chimeric_tag, o.tags);
            const bool is_tail = c == n_ref;
            if (!bam.seek(is_tail ? tail_voff : index[(size_t)c].beg, is_tail ? 0 : index[(size_t)c].end)) { sh.rc = RSQC_ERR_ARG; sh.error = "cannot seek in " + bam_path; return; }
            uint64_t left = is_tail ? ~0ull : (index[(size_t)c].n_records ? index[(size_t)c].n_records : ~0ull), done = 0;
            while (left) {
                HostBatch &hb = bufs[cur];
                hb.clear();
                hb.file_index_base = ((uint64_t)c << kFileIndexShift) + done;
                size_t n = bam.read_batch(hb, (size_t)std::min<uint64_t>(left, BATCH));
                bool last = false;
                if (n && !is_tail && hb.keep_leading_contig(c)) { n = hb.size(); last = true; }   // ran into the next contig
                if (is_tail && n) {                                    // (the tail holds unplaced records only: tid -1)
                    for (int32_t t : hb.seg_tid) if (t >= 0) { sh.rc = RSQC_ERR_ARG; sh.error = "placed records behind the last indexed contig: stale index?"; return; }
                }
                if (in_flight) { if ((sh.rc = rsqc_wait(sh.gpu)) != RSQC_OK) { sh.error = rsqc_last_error(sh.gpu); return; } in_flight = false; }
                if (n == 0) break;
                if (hb.unsorted) sh.unsorted = true;
                for (auto &nm : hb.bad_refid) if (sh.bad_refid.size() < 64) sh.bad_refid.push_back(nm);
                rsqc_batch view = hb.view();
                if ((sh.rc = rsqc_submit(sh.gpu, &view)) != RSQC_OK) { sh.error = rsqc_last_error(sh.gpu); return; }
                in_flight = true; cur ^= 1;
                done += n; sh.n_records += n;
                if (left != ~0ull) left -= std::min<uint64_t>(left, n);
                if (last) break;
            }
            if (in_flight) { if ((sh.rc = rsqc_wait(sh.gpu)) != RSQC_OK) { sh.error = rsqc_last_error(sh.gpu); return; } in_flight = false; }
        }
        sh.rc = rsqc_finalize_device(sh.gpu);
        if (sh.rc != RSQC_OK) sh.error = rsqc_last_error(sh.gpu);
    } catch (std::exception &e) { sh.rc = RSQC_ERR_ARG; sh.error = e.what(); }
}

// merged outputs that do not come out of the reduction
struct ShardMerge { int32_t read_length = 0; std::vector<int64_t> fsize; std::vector<uint64_t> fcount; uint32_t remaining = 0; };

int merge_shards(std::vector<Shard> &shards, uint32_t fragment_samples, ShardMerge &m, std::string &err) {
    std::vector<rsqc::RlTable> items;
    std::vector<std::pair<uint64_t, uint32_t>> samples;
    for (auto &sh : shards) {
        rsqc_shard_info si{};
        const int rc = rsqc_shard_summary(sh.gpu, &si);
        if (rc != RSQC_OK) { err = rsqc_last_error(sh.gpu); return rc; }
        for (uint32_t b = 0; b < si.n_batches; ++b)
            items.push_back(rsqc::RlTable{si.batch_file_index[b], si.rl_span + si.rl_offset[b], si.rl_state + si.rl_offset[b], si.rl_offset[b + 1] - si.rl_offset[b]});
        for (uint32_t k = 0; k < si.n_samples; ++k) samples.emplace_back(si.sample_file_index[k], si.sample_size[k]);
    }
    // Read Length (src/RNASeQC.cpp:275-278): the batches of all shards in file order, each applied as its transfer function
    m.read_length = rsqc::rl_compose(items);
    // fragment sizes (src/Expression.cpp:482-540): the --fragment-samples first samples of the union, in file order
    const size_t keep = std::min<size_t>(samples.size(), fragment_samples);
    if (keep < samples.size()) std::nth_element(samples.begin(), samples.begin() + (long)keep, samples.end());
    std::vector<uint32_t> sz(keep);
    for (size_t k = 0; k < keep; ++k) sz[k] = samples[k].second;
    std::sort(sz.begin(), sz.end());
    for (size_t i = 0; i < keep;) { size_t j = i + 1; while (j < keep && sz[j] == sz[i]) ++j; m.fsize.push_back((int64_t)sz[i]); m.fcount.push_back((uint64_t)(j - i)); i = j; }
    m.remaining = fragment_samples - (uint32_t)keep;
    return RSQC_OK;
}

namespace {

using Clock = std::chrono::steady_clock;
double seconds_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }
const char *const kUnsortedWarning = "Warning: The input bam does not appear to be sorted. An unsorted bam will yield incorrect results";

// The exception in flight as the reference's exit code, its message on stderr behind `prefix` (src/RNASeQC.cpp:678-766; the
// argument errors that print the usage text are main()'s own).  Called from a catch (...) block.
int explain_exception(const std::string &prefix) {
    using std::cerr; using std::endl;
    try { throw; }
    catch (std::invalid_argument &e) { cerr << prefix << "Invalid argument type provided: " << e.what() << endl; return 7; }
    catch (FileError &e) { cerr << prefix << e.what() << endl; return 10; }
    catch (GtfError &e) { cerr << prefix << "Failed to parse the GTF: " << e.what() << endl; return 11; }
    catch (BedError &e) { cerr << prefix << "Failed to parse the BED: " << e.what() << endl; return 11; }
    catch (std::length_error &e) { cerr << prefix << "Unable to parse the GFT lines" << endl << e.what() << endl; return 1; }
    catch (std::range_error &e) { cerr << prefix << "Invalid range" << endl << e.what() << endl; return 2; }
    catch (std::domain_error &e) { cerr << prefix << "Unable to perform string conversion" << endl << e.what() << endl; return 3; }
    catch (std::bad_alloc &e) { cerr << prefix << "Memory allocation failure. Out of memory" << endl << e.what() << endl; return 10; }
    catch (std::exception &e) { cerr << prefix << "Encountered an IO failure" << endl << e.what() << endl; return 10; }
    catch (...) { cerr << prefix << "Unknown error" << endl; return -1; }
}

// ---- one input, opened: its format by content and its header.  Nothing here touches the GPU, so a cohort does this for
// sample k+1 on a thread beside sample k's decode.
struct Input {
    std::string path;
    bool is_stream = false;                           // a FIFO / stdin: streamed by the host (the block feeder needs pread)
    InputFormat fmt = InputFormat::Unknown;
    std::vector<std::string> contigs;                 // the header's reference names, in order
    std::vector<uint64_t> lengths;                    // ... and their lengths (@SQ LN / l_ref; 0: absent)
    uint64_t first_voff = 0, file_size = 0;           // BAM for the device decode: virtual offset of the first record
    std::unique_ptr<SamTextFeeder> stream_feed;       // SAM text from a stream: holds the bytes that were read to sniff it
    std::unique_ptr<BamReader> reader;                // BAM decoded on the host (RSQC_DECODE=host, or a stream)
    std::string error;                                // not empty: the input cannot be opened (exit code 10)
    Clock::time_point t_open;
    bool sam() const { return fmt == InputFormat::SamText || fmt == InputFormat::SamBgzf; }
};

std::unique_ptr<Input> open_input(const std::string &path, const Options &o) {
    std::unique_ptr<Input> in(new Input());
    in->path = path; in->t_open = Clock::now();
    const std::string unable = "Unable to open BAM file: " + path;
    { struct stat st; if (stat(path.c_str(), &st) == 0) { in->is_stream = !S_ISREG(st.st_mode); in->file_size = (uint64_t)st.st_size; } }
    // the input's format by its content
    in->fmt = in->is_stream ? InputFormat::Unknown : sniff_file(path);
    std::string reader_path = path;                   // what the host BAM reader opens
    if (in->is_stream) {
        // a FIFO / stdin: its first bytes are read to tell the format and stay the first chunk's; a BAM is handed on to the
        // host reader through a pipe of this process that replays them
        in->stream_feed.reset(new SamTextFeeder());
        if (!in->stream_feed->open(path)) { in->error = unable; return in; }
        const std::vector<uint8_t> &first = in->stream_feed->peek(1 << 16);
        in->fmt = sniff_format(first.data(), first.size());
        if (in->fmt == InputFormat::Bam || in->fmt == InputFormat::Unknown) {
            int pfd[2];
            if (pipe(pfd) != 0) { in->error = unable; return in; }
            signal(SIGPIPE, SIG_IGN);
            const int src = in->stream_feed->release_fd();
            std::thread([src, pfd, head = in->stream_feed->peek(0)]() {
                auto put = [&](const uint8_t *b, size_t n) { while (n) { const ssize_t w = write(pfd[1], b, n); if (w <= 0) return false; b += w; n -= (size_t)w; } return true; };
                bool ok = put(head.data(), head.size());
                std::vector<uint8_t> buf(1 << 20);
                while (ok) { const ssize_t g = read(src, buf.data(), buf.size()); if (g <= 0) break; ok = put(buf.data(), (size_t)g); }
                close(pfd[1]); close(src);
            }).detach();
            reader_path = "/dev/fd/" + std::to_string(pfd[0]);
            in->stream_feed.reset();
            in->fmt = InputFormat::Bam;
        }
    }
    if (in->fmt == InputFormat::PlainGzip) { in->error = unable + " (gzip-compressed but not BGZF: recompress it with bgzip)"; return in; }
    if (in->fmt == InputFormat::SamBgzf && in->is_stream) {
        in->error = unable + " (BGZF-compressed SAM is read from a regular file only: decompress it into the pipe)"; return in;
    }
    // The header.  SAM (plain or BGZF-compressed): the @SQ lines are read here, the text goes to the device SAM stages.  BAM with
    // the device decode (the default): the host only inflates the header's own blocks; the multi-threaded CPU reader (whose
    // pools start inflating the file as soon as it is opened) comes up only for RSQC_DECODE=host and for streams.
    if (in->sam()) {
        SamHeader hdr;
        if (in->stream_feed) {
            bool complete = false;
            for (size_t want = 1 << 16;; want *= 2) {
                const auto &hd = in->stream_feed->peek(want);
                hdr = SamHeader{};
                parse_sam_header((const char *)hd.data(), hd.size(), hdr, complete);
                if (complete || hd.size() < want) break;
            }
        } else if (!read_sam_header(path, hdr)) { in->error = unable; return in; }
        in->contigs = hdr.names; in->lengths = hdr.lengths;
    } else if (device_decode_wanted(in->is_stream)) {
        BgzfFeeder probe;
        if (!probe.open(path)) { in->error = unable; return in; }
        try { in->first_voff = probe.first_record_voffset(&in->contigs, &in->lengths); }
        catch (std::exception &) { in->error = unable; return in; }
    } else {
        in->reader.reset(new BamReader());
        if (!in->reader->open(reader_path)) { in->error = unable; in->reader.reset(); return in; }
        in->reader->set_tags(o.chimeric_tag, o.tags);
        if (o.has_umi_tag) in->reader->set_umi(RSQC_UMI_SOURCE_TAG, o.umi_tag[0], o.umi_tag[1], 0);
        if (o.has_umi_qname) in->reader->set_umi(RSQC_UMI_SOURCE_QNAME, 0, 0, o.umi_sep[0]);
        in->contigs = in->reader->contigs(); in->lengths = in->reader->contig_lengths();
    }
    return in;
}

// ---- what a process sets up once and every sample of it uses: the context, its inputs, the page-locked buffers
struct Session {
    rsqc_params P{};
    rsqc_ctx *gpu = nullptr;
    std::future<int> gpu_ready;                        // rsqc_create, beside the GTF parse
    int gpu_rc = RSQC_OK; bool gpu_asked = false;
    Clock::time_point t_start, t_gtf0, t_gtf1, t_gpu0, t_gpu1, t_loop0, t_loop1, t_rep0, t_rep1;
    // the annotation as parsed: chromosomeMap before any input's header joined it, and the chromosomes with GTF features
    std::map<std::string, int> base_chrom_id; std::vector<std::string> base_chrom_name;
    std::vector<char> gtf_chrom;
    // the header the annotation is flattened for, and what of it the context holds
    bool flattened = false, inputs_set = false, needs_reset = false;
    bool dirty = false;                                // a pass that did not reach its results is in the context
    std::vector<std::string> contigs;
    FastaFile fasta;
    std::vector<std::vector<uint8_t>> fasta_seq;
    bool keep_fasta = false;                           // a cohort: the bases stay on the host for the next set of inputs
    std::vector<char> in_fasta;
    std::future<void> fasta_loaded;                    // (declared behind what its thread fills: its destructor joins the reader first)
    // feeders and staging, page-locked once
    std::unique_ptr<BgzfFeeder> feed; std::string feed_path; bool feed_ready_checked = true, feed_prepared = false;
    std::future<bool> feed_ready;                      // the feeder's buffers, page-locked beside the GTF parse
    std::unique_ptr<SamTextFeeder> sam_feed;
    std::unique_ptr<HostBatch[]> bufs;
    bool decode_reserved = false; uint64_t reserve_file_size = 0;
    // a cohort: messages carry the sample's name, the reports are written on a thread beside the next sample (one job at most)
    std::string prefix;
    bool async_reports = false;
    JunctionIndex junction_index;                      // --junctions: the annotation's exon boundaries, built once
    GeneBodyModel gene_body; bool gene_body_built = false;      // --gene-body: the model for the header in use (its contigs and their lengths)
    std::vector<uint64_t> gene_body_lengths;
    // --mismatches: the header (contigs and lengths) the context's packed reference was made for; empty: none is kept
    bool mismatch_packed = false;
    std::vector<std::string> mismatch_contigs; std::vector<uint64_t> mismatch_lengths;
    SiteFile sites;                                    // --alleles: the file's lines, parsed once; resolved against every input's header
    std::future<void> report_job;
    void finish_reports() { if (report_job.valid()) report_job.get(); }
};

int feeder_cpu_threads() {
    const int spare = effective_cpus() - 4;
    return getenv("RSQC_DECODE_CPU_THREADS") ? atoi(getenv("RSQC_DECODE_CPU_THREADS")) : (spare >= 4 ? spare : 0);
}
size_t feeder_chunk_bytes() { return getenv("RSQC_DECODE_CHUNK") ? (size_t)atoll(getenv("RSQC_DECODE_CHUNK")) : (size_t)512 << 20; }
uint64_t feeder_max_out_bytes() { return getenv("RSQC_DECODE_MAX_OUT") ? (uint64_t)atoll(getenv("RSQC_DECODE_MAX_OUT")) : (uint64_t)1024 << 20; }
bool feeder_prepin() { return !(getenv("RSQC_FEED_PREPIN") && !atoi(getenv("RSQC_FEED_PREPIN"))); }

// The page-locked chunk buffers of the device decode's feeder (one GPU: ~1.3 GB, a few hundred ms of page-locking) come up
// beside the GTF parse.  `path`: the file whose size and compression the buffers are sized for -- a cohort's largest BAM.  A
// file that cannot be opened is reported later, where the reference reports it.
void start_early_feeder(Session &S, const std::string &path) {
    S.feed.reset(new BgzfFeeder());
    S.feed_path = path;
    BgzfFeeder *ef = S.feed.get();
    const int ct = feeder_cpu_threads();
    const size_t chunk = feeder_chunk_bytes();
    const uint64_t max_out = feeder_max_out_bytes();
    S.feed_ready_checked = false;
    S.feed_ready = std::async(std::launch::async, [ef, path, ct, chunk, max_out] {
        try {
            if (!ef->open(path)) return false;
            // (the room behind a chunk's file bytes is page-locked for the largest share the CPUs can reach: 12 threads have
            //  settled at 0.10-0.25 of a call on every file measured; 0.5 only where there are the threads for it)
            if (ct > 0) ef->set_cpu_share(ct, 0.15, std::min(0.5, std::max(0.1, 0.025 * ct)), max_out);
            ef->reserve(chunk, max_out);
            return true;
        } catch (std::exception &) { return false; }
    });
}

// annotation and BED of one context; 0, or the exit code with the message printed
int set_annotation_and_bed(const Options &o, Annotation &ann, rsqc_ctx *gpu, const uint8_t *owned, bool warn, const std::string &prefix, int &rc) {
    using std::cerr; using std::endl;
    if ((rc = rsqc_set_annotation(gpu, &ann.ann, owned)) != RSQC_OK) {
        // (the GTF parsed: this is the device index refusing the annotation -- e.g. no memory for the interval tables -- and
        //  its own message says which)
        cerr << prefix << "Unable to build the annotation index on the GPU: " << rsqc_last_error(gpu) << endl; return 11;
    }
    // accepted with a warning (an exon outside its gene's row): the reference's counterpart is its per-read
    // "Gene encountered after computing coverage" (src/Metrics.cpp:108-112); said once, before the BAM loop
    if (warn && rsqc_last_error(gpu)[0]) cerr << prefix << "Warning: " << rsqc_last_error(gpu) << endl;
    if (o.has_bed && (rc = rsqc_set_bed(gpu, &ann.bed)) != RSQC_OK) { cerr << prefix << "Failed to parse the BED: " << rsqc_last_error(gpu) << endl; return 11; }
    return 0;
}
// --fasta: the contigs of the FASTA index that the flattened annotation names, on every context
int set_reference(Session &S, Annotation &ann, const std::vector<rsqc_ctx *> &ctxs, int &rc) {
    using std::cerr; using std::endl;
    if (S.fasta_loaded.valid()) S.fasta_loaded.get();                     // FileError -> 10
    S.in_fasta.assign(ann.contig_names.size(), 0);
    std::vector<int32_t> r_contig; std::vector<uint64_t> r_len; std::vector<const uint8_t *> r_seq;
    for (size_t i = 0; i < S.fasta.index.size(); ++i) {
        int cid = -1;
        for (size_t k = 0; k < ann.contig_names.size(); ++k) if (ann.contig_names[k] == S.fasta.index[i].name) { cid = (int)k; break; }
        if (cid < 0) continue;                                            // a contig neither the BAM nor the GTF/BED names
        r_contig.push_back(cid); r_len.push_back(S.fasta_seq[i].size()); r_seq.push_back(S.fasta_seq[i].data());
        S.in_fasta[(size_t)cid] = 1;
    }
    rsqc_reference ref{(int32_t)r_contig.size(), r_contig.data(), r_len.data(), r_seq.data()};
    for (rsqc_ctx *gpu : ctxs)
        if ((rc = rsqc_set_reference(gpu, &ref)) != RSQC_OK) { cerr << S.prefix << "Failed to load the reference: " << rsqc_last_error(gpu) << endl; return 10; }
    if (!S.keep_fasta) std::vector<std::vector<uint8_t>>().swap(S.fasta_seq);   // the bases live on the device now
    return 0;
}

// header check: at least one BAM contig must carry GTF features (src/RNASeQC.cpp:216-238)
bool shares_contigs(const Session &S, const Annotation &ann, const std::vector<std::string> &contigs) {
    for (auto &n : contigs) {
        auto it = ann.chrom_id.find(n);
        if (it != ann.chrom_id.end() && (size_t)it->second < S.gtf_chrom.size() && S.gtf_chrom[(size_t)it->second]) return true;
    }
    return false;
}
// the annotation flattened against a header's contig order (the BED and the reference follow: their contig ids come from the same map)
void flatten_for(Session &S, Annotation &ann, const std::vector<std::string> &contigs) {
    S.finish_reports();                                    // (the writer of the sample before reads the flattened tables)
    if (S.flattened) { ann.chrom_id = S.base_chrom_id; ann.chrom_name = S.base_chrom_name; }   // as a run of this input alone sees chromosomeMap
    ann.flatten(contigs);
    S.contigs = contigs; S.flattened = true;
    S.gene_body_built = false;
}

// what the report writer reads of rsqc_results, in memory of its own: the vectors behind rsqc_results are the context's and
// valid only until its next rsqc_finalize
struct ResultsCopy {
    rsqc_results res{};
    std::vector<std::vector<char>> store;
    template <class T> void keep(const T *&p, size_t n) {
        if (!p) return;
        store.emplace_back(std::max<size_t>(n, 1) * sizeof(T));
        memcpy(store.back().data(), p, n * sizeof(T));
        p = (const T *)store.back().data();
    }
    explicit ResultsCopy(const rsqc_results &r) : res(r) {
        const size_t L = (size_t)std::max(r.n_genes_listed, 0), E = (size_t)std::max(r.n_exons, 0);
        keep(res.gene_reads, L); keep(res.gene_unique, L); keep(res.gene_fragments, L);
        keep(res.exon_reads, E); keep(res.exon_hit, E);
        keep(res.gene_cov_mean, L); keep(res.gene_cov_std, L); keep(res.gene_cov_cv, L); keep(res.gene_cov_valid, L);
        keep(res.exon_cv, E); keep(res.exon_cv_valid, E);
        keep(res.bias_three, L); keep(res.bias_five, L);
        keep(res.fragment_size, r.n_fragment_sizes); keep(res.fragment_count, r.n_fragment_sizes);
        keep(res.gc_bins, RSQC_GC_BINS); keep(res.exon_gc, E);
    }
};

struct Sample { std::string path, name; bool name_given = false; std::future<std::unique_ptr<Input>> opened; };   // name_given: as --sample (the GCT value column)
// a row of cohort.tsv
struct SampleRow { std::string sample, input, format = "not run"; uint64_t records = 0; double seconds = 0; int exit_code = 0; bool fatal = false; };

// ---- one sample on one GPU: the input opened and its header read (or taken over from the thread that did), the contig check,
// the context's inputs (set, kept, or replaced when the header's contigs differ from the sample before), the decode loop,
// finalize and the reports.  Returns the exit code of a run of this input alone; throws what main() maps to exit codes.
// the junction table of a sample, copied for the report thread
struct JunctionCopy {
    std::vector<int32_t> tid, start, end; std::vector<uint32_t> reads, hq_reads, max_overhang;
    rsqc_junction_table table{};
    explicit JunctionCopy(const rsqc_junction_table &t) : tid(t.tid, t.tid + t.n), start(t.start, t.start + t.n), end(t.end, t.end + t.n), reads(t.reads, t.reads + t.n),
                                                          hq_reads(t.hq_reads, t.hq_reads + t.n), max_overhang(t.max_overhang, t.max_overhang + t.n), table(t) {
        table.tid = tid.data(); table.start = start.data(); table.end = end.data(); table.reads = reads.data(); table.hq_reads = hq_reads.data(); table.max_overhang = max_overhang.data();
    }
};

// --bedgraph: <output>/<sample>.coverage.bedgraph from the rows on the device, a window of text at a time: the next window is
// formatted (rsqc_track_text) while a second thread writes the one before.  Returns an RSQC code; io_failed: the file could not be written
int write_bedgraph(rsqc_ctx *gpu, const std::string &path, uint64_t n_rows, uint64_t &bytes_out, double &text_seconds, bool &io_failed) {
    const uint64_t window = 4194304;                   // (the most rsqc_track_text takes)
    const Clock::time_point t0 = Clock::now();
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    io_failed = !f.is_open(); bytes_out = 0;
    std::vector<char> buf[2];
    std::future<void> writing;
    int cur = 0, rc = RSQC_OK;
    for (uint64_t first = 0; first < n_rows && rc == RSQC_OK && !io_failed; first += window) {
        const char *text = nullptr; uint64_t bytes = 0;
        if ((rc = rsqc_track_text(gpu, first, std::min(window, n_rows - first), &text, &bytes)) != RSQC_OK) break;
        buf[cur].assign(text, text + bytes);           // (the context's window ends with the next call)
        if (writing.valid()) writing.get();
        if (!f.good()) { io_failed = true; break; }
        const std::vector<char> *b = &buf[cur];
        writing = std::async(std::launch::async, [&f, b] { f.write(b->data(), (std::streamsize)b->size()); });
        bytes_out += bytes; cur ^= 1;
    }
    if (writing.valid()) writing.get();
    f.close();
    if (!f.good()) io_failed = true;
    text_seconds = seconds_between(t0, Clock::now());
    return rc;
}

int run_sample(const Options &o, Annotation &ann, Session &S, Sample &sample, const std::string &out_dir, SampleRow &row) {
    using std::cerr; using std::cout; using std::endl;
    std::unique_ptr<Input> opened = sample.opened.valid() ? sample.opened.get() : open_input(sample.path, o);
    Input &in = *opened;
    const std::string &path = in.path;
    const Clock::time_point t_open = in.t_open;
    struct Timer { SampleRow &row; Clock::time_point t0; bool armed = true; ~Timer() { if (armed) row.seconds = seconds_between(t0, Clock::now()); } } timer{row, t_open};
    row.format = input_format_name(in.fmt);
    if (!in.error.empty()) { cerr << S.prefix << in.error << endl; return 10; }
    const bool sam_input = in.sam();
    const std::vector<std::string> &bam_contigs = in.contigs;
    if (sam_input && o.verbosity > 1) cout << "Input: " << input_format_name(in.fmt) << " (" << bam_contigs.size() << " @SQ lines), parsed on the GPU" << endl;
    if (o.verbosity > 1) cout << "Checking bam header..." << endl;
    if (!shares_contigs(S, ann, bam_contigs)) { cerr << S.prefix << "BAM file shares no contigs with GTF" << endl; return 11; }
    if (o.bedgraph || o.gene_body || o.tin)            // the track needs every contig's length
        for (size_t k = 0; k < bam_contigs.size(); ++k)
            if (k >= in.lengths.size() || in.lengths[k] == 0) {
                std::vector<const char *> flags;       // "--a needs", "--a and --b need", "--a, --b and --c need"
                if (o.bedgraph) flags.push_back("--bedgraph");
                if (o.gene_body) flags.push_back("--gene-body");
                if (o.tin) flags.push_back("--tin");
                std::string who;
                for (size_t f = 0; f < flags.size(); ++f) who += std::string(f == 0 ? "" : f + 1 == flags.size() ? " and " : ", ") + flags[f];
                cerr << S.prefix << who << (flags.size() > 1 ? " need" : " needs") << " the length (LN) of every contig in the header: none for " << bam_contigs[k] << endl; return 10;
            }
    // --mismatches: per header contig its entry of the FASTA index (-1: the FASTA lacks it); a length that contradicts the header's is refused
    std::vector<int> mismatch_entry;
    if (o.mismatches) {
        mismatch_entry.assign(bam_contigs.size(), -1);
        for (size_t k = 0; k < bam_contigs.size(); ++k)
            for (size_t i = 0; i < S.fasta.index.size(); ++i) if (S.fasta.index[i].name == bam_contigs[k]) { mismatch_entry[k] = (int)i; break; }
        for (size_t k = 0; k < bam_contigs.size(); ++k) {
            const uint64_t ln = k < in.lengths.size() ? in.lengths[k] : 0;
            if (mismatch_entry[k] >= 0 && ln && ln != S.fasta.index[(size_t)mismatch_entry[k]].length) {
                cerr << S.prefix << "--mismatches: contig " << bam_contigs[k] << " has " << ln << " bases in the header (LN) and " << S.fasta.index[(size_t)mismatch_entry[k]].length
                     << " in the FASTA: this is not the reference the input was aligned to" << endl;
                return 10;
            }
        }
    }
    const bool same_header = S.flattened && bam_contigs == S.contigs;
    if (!same_header) flatten_for(S, ann, bam_contigs);
    // --gene-body, --tin: the model of this header's contigs and lengths (one for both), built when either changes
    if ((o.gene_body || o.tin) && (!S.gene_body_built || S.gene_body_lengths != in.lengths)) { S.gene_body.build(ann, in.lengths); S.gene_body_lengths = in.lengths; S.gene_body_built = true; }
    const int n_ref_bam = (int)bam_contigs.size();
    // --alleles: the file's sites in this header's contig order
    ResolvedSites sites;
    if (o.has_alleles) resolve_sites(S.sites, bam_contigs, sites);

    // ---- the context and its inputs
    if (!S.gpu_asked) {
        S.t_gpu0 = Clock::now();
        S.gpu_rc = S.gpu_ready.get();
        S.t_gpu1 = Clock::now();
        S.gpu_asked = true;
    }
    if (S.gpu_rc != RSQC_OK) { cerr << S.prefix << "Unable to initialise the GPU hot path: " << rsqc_strerror(S.gpu_rc) << endl; row.fatal = true; return 10; }
    rsqc_ctx *gpu = S.gpu;
    int rc;
    auto hip_failed = [&](int code) { if (code == RSQC_ERR_HIP) row.fatal = true; return code; };
    auto gpu_failed = [&](int code) { cerr << S.prefix << rsqc_strerror(code) << ": " << rsqc_last_error(gpu) << endl; hip_failed(code); return 10; };      // a call of the library that failed: its text, exit 10
    if (S.dirty || (S.inputs_set && !same_header)) {
        // another contig order, or a sample that failed in the middle of its pass: everything in flight is waited for and the
        // context is as rsqc_create left it (its streams, pools and decode buffers kept)
        if ((rc = rsqc_clear_inputs(gpu)) != RSQC_OK) return gpu_failed(rc);
        S.inputs_set = false; S.dirty = false; S.needs_reset = false;
        S.mismatch_packed = false;                                         // (the packed reference went with the inputs)
    }
    if (!S.inputs_set) {
        S.dirty = true;                                                    // (a set that fails half-way is cleared before the next one)
        if (int code = set_annotation_and_bed(o, ann, gpu, nullptr, true, S.prefix, rc)) { hip_failed(rc); return code; }
        if (o.has_fasta) if (int code = set_reference(S, ann, {gpu}, rc)) { hip_failed(rc); return code; }
        S.inputs_set = true; S.dirty = false;
    } else if (S.needs_reset) {
        if ((rc = rsqc_reset(gpu)) != RSQC_OK) return gpu_failed(rc);
    }
    S.needs_reset = false;

    const bool device_decode = device_decode_wanted(in.is_stream) && !sam_input;
    if (device_decode && !S.decode_reserved && !(getenv("RSQC_DECODE_PRERESERVE") && !atoi(getenv("RSQC_DECODE_PRERESERVE")))) {
        // the device's window buffers are set up before the loop, like the host path's page-locked batches below: once, for the
        // largest file the process will read
        rsqc_decode_params dp = decode_params(o, n_ref_bam, 0);
        dp.reserve_inflated_bytes = decode_reserve_bytes(std::max(S.reserve_file_size, in.file_size));
        rsqc_decode_info none{};
        if ((rc = rsqc_decode_begin(gpu, &dp)) != RSQC_OK || (rc = rsqc_decode_end(gpu, &none)) != RSQC_OK) {
            cerr << S.prefix << "Unable to set up the device decode: " << rsqc_last_error(gpu) << endl; hip_failed(rc); return 10;
        }
        S.decode_reserved = true;
    }
    // the feeder's chunk buffers are page-locked here, before the loop: page-locking takes the HIP runtime's lock, and done
    // by the read-ahead thread during the loop it stalled the thread that feeds the GPU (193 -> 237 M reads/s)
    if (device_decode) {
        // RSQC_DECODE_CPU_THREADS=n: n spare CPU threads inflate the tail of every chunk beside the GPU (BgzfFeeder::set_cpu_share)
        // (default: the CPUs the process may use minus four for the file reads and the thread that feeds the GPU; measured on the
        //  16-CPU box, 12 threads: 258 -> 279 M reads/s, 85 -> 97 M on the realistic-entropy file, profiles/r2_decode_cpu_share_ab.txt)
        if (!S.feed_ready_checked) {
            S.feed_ready_checked = true;
            if (S.feed_ready.get()) S.feed_prepared = true; else S.feed.reset();
        }
        if (!S.feed) { S.feed.reset(new BgzfFeeder()); S.feed_path.clear(); S.feed_prepared = false; }
        if (S.feed_path != path) {                     // (the next file of a cohort: the buffers stay)
            S.feed_path.clear();
            if (!S.feed->open(path)) { cerr << S.prefix << "Unable to open BAM file: " << path << endl; return 10; }
            S.feed_path = path;
        }
        if (!S.feed_prepared) {
            const int cpu_share_threads = feeder_cpu_threads();
            if (cpu_share_threads > 0) S.feed->set_cpu_share(std::max(1, cpu_share_threads), 0.15, 0.5, (uint64_t)1 << 30);
            if (feeder_prepin()) S.feed->reserve(feeder_chunk_bytes());
            S.feed_prepared = true;
        }
        // (threads that read one chunk's slices side by side; RSQC_FEED_READ_THREADS overrides)
        S.feed->read_threads = getenv("RSQC_FEED_READ_THREADS") ? std::max(1, atoi(getenv("RSQC_FEED_READ_THREADS"))) : std::max(1, std::min(8, effective_cpus() / 2));
    }
    if (o.verbosity) cout << "Parsing bam..." << endl;
    std::vector<int> visit;
    unsigned long long alignmentCount = 0;
    bool warned_unsorted = false;
    auto warn_unsorted = [&] { if (!warned_unsorted && !o.sort) { cerr << S.prefix << kUnsortedWarning << endl; warned_unsorted = true; } };
    // a contig the input visits: the order of coverage.tsv, the sort check, the FASTA's gaps (src/RNASeQC.cpp:350-355)
    auto visit_contig = [&](int32_t t, bool &revisit) {
        if (t < 0 || (!visit.empty() && visit.back() == t)) return;
        if (std::find(visit.begin(), visit.end(), t) != visit.end()) { revisit = true; if (o.sort) return; }     // a contig that comes back (--sort: expected, listed once)
        visit.push_back(t);
        if (o.has_fasta && (size_t)t < S.in_fasta.size() && !S.in_fasta[(size_t)t])
            cerr << S.prefix << "Warning: Provided Fasta does not contain chromosome " << ann.contig_names[(size_t)t]
                 << ". No GC statistics will be collected for this chromosome" << endl;
    };
    auto on_window = [&](const rsqc_decode_window &w) {
        bool revisit = false;
        for (uint32_t k = 0; k < w.n_runs; ++k) visit_contig(w.run_tid[k], revisit);
        if (revisit) warn_unsorted();
        alignmentCount += w.n_records;
        row.records = alignmentCount;
        if (o.verbosity > 1) cout << "Alignments processed: " << alignmentCount << endl;
    };
    // stderr of the reference's loop: the names of records with a RefID the header lacks (src/RNASeQC.cpp:333-337, under -v)
    // and the sort warning (:354-355).  The reference repeats the warning for every offending record; it is given
    // once here -- an unsorted file voids the results either way (the static index does not reproduce what the
    // reference's destructively trimmed window would count).
    auto after_stream = [&](int code, const rsqc_decode_info &di) {
        if (code == RSQC_ERR_INPUT) throw std::runtime_error(rsqc_last_error(gpu));
        if (code != RSQC_OK) return;
        if (o.verbosity) for (int k = 0; k < di.n_bad_refid && k < 64; ++k) cerr << S.prefix << "Unrecognized RefID on alignment: " << di.bad_refid[k] << endl;
        if (di.unsorted) warn_unsorted();
    };
    S.dirty = true;
    // --mismatches: every decode window leaves the counts of its records' walk over the reference on the device.  The reference is packed for
    // this header here, in front of the loop's window like the other inputs (a cohort: once, while its contigs and lengths stay)
    std::vector<const char *> mismatch_seq; std::vector<uint64_t> mismatch_len;
    if (o.mismatches) {
        for (size_t k = 0; k < bam_contigs.size(); ++k) {
            const int i = mismatch_entry[k];
            mismatch_seq.push_back(i >= 0 ? (const char *)S.fasta_seq[(size_t)i].data() : nullptr);
            mismatch_len.push_back(i >= 0 ? (uint64_t)S.fasta_seq[(size_t)i].size() : (k < in.lengths.size() ? in.lengths[k] : 0));
        }
        const bool kept = S.mismatch_packed && S.mismatch_contigs == bam_contigs && S.mismatch_lengths == mismatch_len;
        S.mismatch_packed = false;
        if ((rc = rsqc_mismatch_begin(gpu, n_ref_bam, mismatch_len.data(), kept ? nullptr : mismatch_seq.data(), (uint32_t)o.mismatches_mapq)) != RSQC_OK) return gpu_failed(rc);
        S.mismatch_packed = true; S.mismatch_contigs = bam_contigs; S.mismatch_lengths = mismatch_len;
        // one input that the device decodes: the bases live on the device now (a cohort may meet another header, the host reader compares with them)
        if (!S.async_reports && (sam_input || device_decode)) { std::vector<std::vector<uint8_t>>().swap(S.fasta_seq); mismatch_seq.clear(); }
    }
    // --alleles: the sites go to the device for this header; every decode window leaves the bases of its records at them there
    if (o.has_alleles && (rc = rsqc_alleles_begin(gpu, n_ref_bam, (uint32_t)sites.tid.size(), sites.tid.data(), sites.pos.data(), (uint32_t)o.allele_mapq, (uint32_t)o.allele_baseq)) != RSQC_OK)
        return gpu_failed(rc);
    S.t_loop0 = Clock::now();
    rc = RSQC_OK;
    // --sort: the loops below collect (no per-read kernel runs); rsqc_sort_end orders the records and runs them
    if (o.sort && (rc = rsqc_sort_begin(gpu)) != RSQC_OK) return gpu_failed(rc);
    // --mark-duplicates: rsqc_sort_end first rewrites flag 0x400 of the collection
    if (o.mark_duplicates && (rc = rsqc_markdup_begin(gpu)) != RSQC_OK) return gpu_failed(rc);
    // --umi-tag / --umi-qname: the UMI key of the decode streams / the host reader's batches joins the signature
    if ((o.has_umi_tag || o.has_umi_qname) && (rc = rsqc_markdup_use_umi(gpu)) != RSQC_OK) return gpu_failed(rc);
    if (o.umi_edits == "1" && (rc = rsqc_markdup_umi_edits(gpu, 1)) != RSQC_OK) return gpu_failed(rc);
    // --junctions: every batch the per-read kernels run leaves its junction instances on the device (under --sort: the sorted batches)
    if (o.junctions && (rc = rsqc_junctions_begin(gpu)) != RSQC_OK) return gpu_failed(rc);
    // --bedgraph: and its coverage events, in a difference array over the header's contigs (kept by the context while it is large enough)
    if (o.bedgraph || o.gene_body || o.tin) {
        std::vector<const char *> track_names;
        for (auto &nm : bam_contigs) track_names.push_back(nm.c_str());
        if ((rc = rsqc_track_begin(gpu, n_ref_bam, in.lengths.data(), track_names.data())) != RSQC_OK) return gpu_failed(rc);
    }
    // --gene-body: the model of this header's contigs (built when the header changes), checked, planned and uploaded
    if (o.gene_body) {
        const GeneBodyModel &m = S.gene_body;
        if ((rc = rsqc_genebody_begin(gpu, (int32_t)m.reverse.size(), m.seg_off.data(), m.seg_tid.data(), m.seg_start.data(), m.seg_end.data(), m.reverse.data())) != RSQC_OK) return gpu_failed(rc);
    }
    // --tin: the same model without its strands, in buffers of the mode's own
    if (o.tin) {
        const GeneBodyModel &m = S.gene_body;
        if ((rc = rsqc_tin_begin(gpu, (int32_t)m.gene_len.size(), m.seg_off.data(), m.seg_tid.data(), m.seg_start.data(), m.seg_end.data())) != RSQC_OK) return gpu_failed(rc);
    }
    // --cycles: every decode window leaves the counts of its records' SEQ / QUAL by read cycle on the device; the host reader counts its own
    if (o.cycles && (rc = rsqc_cycles_begin(gpu)) != RSQC_OK) return gpu_failed(rc);
    if (sam_input) {
        // ---- SAM text: the host reads the file (plain) or frames its BGZF blocks, the device does the rest
        rsqc_decode_info di{};
        std::vector<const char *> names;
        for (auto &nm : bam_contigs) names.push_back(nm.c_str());
        if (in.fmt == InputFormat::SamBgzf) {
            BgzfFeeder feed;
            if (!feed.open(path)) { cerr << S.prefix << "Unable to open BAM file: " << path << endl; return 10; }
            feed.read_threads = std::max(1, std::min(8, effective_cpus() / 2));
            rc = decode_range(gpu, feed, decode_params(o, n_ref_bam, 0), 0, 0, di, on_window, names.data());
        } else {
            SamTextFeeder *sam_feed = in.stream_feed.get();
            if (!sam_feed) {                           // a regular file: the process's feeder, its chunk buffers page-locked once
                if (!S.sam_feed) S.sam_feed.reset(new SamTextFeeder());
                if (!S.sam_feed->open(path)) { cerr << S.prefix << "Unable to open BAM file: " << path << endl; return 10; }
                sam_feed = S.sam_feed.get();
            }
            // (RSQC_SAM_CHUNK: bytes of text per call; the tests use small values so that lines straddle many calls)
            const size_t chunk = getenv("RSQC_SAM_CHUNK") ? (size_t)atoll(getenv("RSQC_SAM_CHUNK")) : (size_t)256 << 20;
            rsqc_decode_params dp = decode_params(o, n_ref_bam, 0);
            dp.pipelined = 1;
            dp.reserve_inflated_bytes = chunk + (1u << 20);
            rc = rsqc_decode_begin_sam(gpu, &dp, names.data());
            if (rc == RSQC_OK) {
                sam_feed->start(chunk);
                while (SamTextFeeder::Chunk *ch = sam_feed->next()) {
                    rsqc_decode_window w{};
                    rc = rsqc_decode_submit_text(gpu, ch->data, ch->bytes, &w);
                    if (rc != RSQC_OK) break;
                    if (w.n_records) on_window(w);
                }
                if (rc != RSQC_OK) { rsqc_decode_info dropped{}; (void)rsqc_decode_end(gpu, &dropped); }
                else {
                    if (!sam_feed->error().empty()) { rsqc_decode_info dropped{}; (void)rsqc_decode_end(gpu, &dropped); throw std::runtime_error(sam_feed->error()); }
                    rc = rsqc_decode_end(gpu, &di);
                    if (rc == RSQC_OK && di.last.n_records) on_window(di.last);
                }
            }
        }
        after_stream(rc, di);
    } else if (device_decode) {
        // ---- device decode: the host reads the file and frames the BGZF blocks, nothing else
        rsqc_decode_info di{};
        rc = decode_range(gpu, *S.feed, decode_params(o, n_ref_bam, 0), in.first_voff, 0, di, on_window);
        after_stream(rc, di);
    } else {
        // ---- host decode: inflate and record parsing on the CPU threads, batches through page-locked staging sized once
        const size_t BATCH = getenv("RSQC_BATCH") ? (size_t)atol(getenv("RSQC_BATCH")) : (size_t)1 << 21;
        if (!S.bufs) {
            S.bufs.reset(new HostBatch[2]);
            for (int k = 0; k < 2; ++k) {
                HostBatch &hb = S.bufs[k];
                hb.core.use_pinned(true); hb.aux.use_pinned(true); hb.qh2.use_pinned(true); hb.cigar.use_pinned(true);
                hb.core.reserve(BATCH); hb.aux.reserve(BATCH); hb.qh2.reserve(BATCH); hb.cigar.reserve(BATCH * 2);
            }
        }
        BamReader &bam = *in.reader;
        bam.set_cycles(o.cycles);
        if (o.mismatches) bam.set_mismatches(mismatch_seq, mismatch_len, (uint32_t)o.mismatches_mapq);
        if (o.has_alleles) bam.set_alleles(sites.pos, sites.first, (uint32_t)o.allele_mapq, (uint32_t)o.allele_baseq);
        int cur = 0; bool in_flight = false;
        for (;;) {
            HostBatch &hb = S.bufs[cur];
            hb.clear();
            hb.file_index_base = alignmentCount;
            const size_t n = bam.read_batch(hb, BATCH);              // decode overlaps the previous batch on the GPU
            if (in_flight) { if ((rc = rsqc_wait(gpu)) != RSQC_OK) break; in_flight = false; }
            if (n == 0) break;
            if (o.verbosity) for (auto &nm : hb.bad_refid) cerr << S.prefix << "Unrecognized RefID on alignment: " << nm << endl;
            bool revisit = false;
            for (int32_t t : hb.seg_tid) visit_contig(t, revisit);
            if (hb.unsorted || revisit) warn_unsorted();
            alignmentCount += n;
            row.records = alignmentCount;
            rsqc_batch view = hb.view();
            if ((rc = rsqc_submit(gpu, &view)) != RSQC_OK) break;
            in_flight = true;
            cur ^= 1;
            if (o.verbosity > 1) cout << "Alignments processed: " << alignmentCount << endl;
        }
        if (o.cycles && rc == RSQC_OK) {                   // the records never reached the device as bytes: the reader's sums are added
            std::vector<uint64_t> base, qual;
            rsqc_cycle_info partial{};
            bam.cycles_sum(base, qual, partial);
            rc = rsqc_cycles_add(gpu, base.data(), qual.data(), &partial);
        }
        if (o.mismatches && rc == RSQC_OK) {
            std::vector<uint64_t> cyc, subst, byq;
            rsqc_mismatch_info partial{};
            bam.mismatches_sum(cyc, subst, byq, partial);
            rc = rsqc_mismatch_add(gpu, cyc.data(), subst.data(), byq.data(), &partial);
        }
        if (o.has_alleles && rc == RSQC_OK) {
            std::vector<uint64_t> counts;
            rsqc_allele_info partial{};
            bam.alleles_sum(counts, partial);
            rc = rsqc_alleles_add(gpu, counts.empty() ? nullptr : counts.data(), &partial);
        }
    }
    // (the stage ran at ingest: under --sort and --mark-duplicates the tables are those of the input)
    rsqc_cycle_info cycles{};
    const uint64_t *cycle_base = nullptr, *cycle_qual = nullptr;   // (the context's, until its next reset: the files are written below, before it)
    if (o.cycles && rc == RSQC_OK) rc = rsqc_cycles_end(gpu, &cycles, &cycle_base, &cycle_qual);
    rsqc_mismatch_info mismatches{};
    const uint64_t *mismatch_cyc = nullptr, *mismatch_subst = nullptr, *mismatch_byq = nullptr;
    if (o.mismatches && rc == RSQC_OK) rc = rsqc_mismatch_end(gpu, &mismatches, &mismatch_cyc, &mismatch_subst, &mismatch_byq);
    rsqc_allele_info alleles{};
    const uint64_t *allele_counts = nullptr;
    if (o.has_alleles && rc == RSQC_OK) rc = rsqc_alleles_end(gpu, &alleles, &allele_counts);
    rsqc_sort_info sort_info{};
    if (o.sort && rc == RSQC_OK && (rc = rsqc_sort_end(gpu, &sort_info)) == RSQC_OK) {
        // the contigs in the order the SORTED records visit them: tid as unsigned, each once (the order of coverage.tsv)
        std::sort(visit.begin(), visit.end(), [](int a, int b) { return (uint32_t)a < (uint32_t)b; });
        visit.erase(std::unique(visit.begin(), visit.end()), visit.end());
        if (o.verbosity)
            cout << "Sorted on the GPU: records " << sort_info.records << ", batches in " << sort_info.batches_in << ", batches out " << sort_info.batches_out
                 << ", moved " << sort_info.moved << ", key_ms " << sort_info.key_ms << ", sort_ms " << sort_info.sort_ms << ", gather_ms " << sort_info.gather_ms
                 << ", was_sorted " << sort_info.was_sorted << endl;
        rsqc_markdup_info md{};
        if (o.mark_duplicates && (rc = rsqc_markdup_end(gpu, &md)) == RSQC_OK && o.verbosity)
            cout << "Duplicates marked: records " << md.records << ", population " << md.population << ", anchors " << md.anchors << ", sets " << md.sets
                 << ", duplicate_fragments " << md.duplicate_fragments << ", flagged_records " << md.flagged_records << ", cleared_records " << md.cleared_records
                 << ", sig_ms " << md.sig_ms << ", sort_ms " << md.sort_ms << ", mark_ms " << md.mark_ms << endl;
        rsqc_markdup_umi_info mu{};
        if ((o.has_umi_tag || o.has_umi_qname) && rc == RSQC_OK && (rc = rsqc_markdup_umi_end(gpu, &mu)) == RSQC_OK && o.verbosity)
            cout << "UMIs in the signature: anchors_with_umi " << mu.anchors_with_umi << ", anchors_without_umi " << mu.anchors_without_umi
                 << ", position_duplicate_fragments " << mu.position_duplicate_fragments << endl;
        rsqc_markdup_umi_group_info mg{};
        if (o.umi_edits == "1" && rc == RSQC_OK && (rc = rsqc_markdup_umi_group_end(gpu, &mg)) == RSQC_OK && o.verbosity)
            cout << "UMIs grouped: umi_nodes " << mg.umi_nodes << ", merged_nodes " << mg.merged_nodes << ", exact_duplicate_fragments " << mg.exact_duplicate_fragments
                 << ", group_ms " << mg.group_ms << endl;
    }
    rsqc_results res{};
    if (rc == RSQC_OK) rc = rsqc_finalize(gpu, &res);
    rsqc_junction_table junctions{};
    if (o.junctions && rc == RSQC_OK) rc = rsqc_junctions_end(gpu, &junctions);       // (ordered and reduced inside the timed window: the price of the flag)
    rsqc_track_info track{};
    if ((o.bedgraph || o.gene_body || o.tin) && rc == RSQC_OK) rc = rsqc_track_end(gpu, &track);      // (scan and rows inside the timed window as well)
    rsqc_genebody_info gene_body{};
    GeneBodyProfile gene_body_rows;
    if (o.gene_body && rc == RSQC_OK) rc = rsqc_genebody_end(gpu, &gene_body);               // (and the stage over the scanned array)
    rsqc_tin_info tin{};
    const rsqc_tin_row *tin_rows = nullptr;                // (the context's, until its next reset: the files are written below, before it)
    TinProfile tin_values;
    if (o.tin && rc == RSQC_OK) rc = rsqc_tin_end(gpu, &tin);                                // (and the two kernels of --tin)
    S.t_loop1 = Clock::now();
    if (o.tin && rc == RSQC_OK && (rc = rsqc_tin_rows(gpu, 0, (uint32_t)tin.n_genes, &tin_rows)) == RSQC_OK)
        tin_values = tin_profile(S.gene_body.gene_len.data(), S.gene_body.gene_len.size(), tin_rows);
    if (o.gene_body && rc == RSQC_OK) {
        // the report's part, like the track's text: the sums come from the context in one window and are folded into the file's 100 rows
        const uint64_t *sums = nullptr;
        if ((rc = rsqc_genebody_sums(gpu, 0, (uint32_t)gene_body.n_genes, &sums)) == RSQC_OK) gene_body_rows = gene_body_profile(S.gene_body, sums);
    }
    if (rc == RSQC_ERR_BAD_CIGAR) throw std::invalid_argument("Unrecognized Cigar Op ");
    if (rc == RSQC_ERR_EMPTY_MEDIAN) throw std::range_error("Cannot compute median of an empty list");
    if (rc != RSQC_OK) return gpu_failed(rc);
    S.dirty = false; S.needs_reset = true;
    if (o.verbosity) {
        const double secs = seconds_between(S.t_loop0, S.t_loop1);
        cout << "Time Elapsed: " << secs << "; Alignments processed: " << alignmentCount << endl;
        if (o.verbosity > 1) cout << "Average Reads/Sec: " << (double)alignmentCount / secs << endl;
        if (o.verbosity > 1 && sam_input) cout << "(decode: " << (in.fmt == InputFormat::SamBgzf ? "BGZF inflate and SAM text parsing" : "SAM text") << " on the GPU)" << endl;
        else if (o.verbosity > 1 && device_decode) cout << "(decode: BGZF inflate and record parsing on the GPU)" << endl;
        else if (o.verbosity > 1) cout << "(decode threads: " << in.reader->inflate_threads() << " inflate + " << in.reader->parse_threads() << " parse)" << endl;
        if (o.junctions)
            cout << "Junctions: population " << junctions.population << ", instances " << junctions.instances << ", rows " << junctions.n << ", extract_ms " << junctions.extract_ms
                 << ", sort_ms " << junctions.sort_ms << ", reduce_ms " << junctions.reduce_ms << endl;
        if (o.bedgraph)
            cout << "Track: population " << track.population << ", aligned_bases " << track.aligned_bases << ", clipped_bases " << track.clipped_bases << ", rows " << track.n_rows
                 << ", events_ms " << track.events_ms << ", scan_ms " << track.scan_ms << ", rows_ms " << track.rows_ms << endl;
        if (o.gene_body)
            cout << "Gene body: genes " << gene_body.n_genes << ", measured " << gene_body.n_measured << ", eligible " << gene_body_rows.eligible << ", model_bases " << gene_body.model_bases
                 << ", depth_sum " << gene_body.depth_sum << ", bins_ms " << gene_body.bins_ms << endl;
        if (o.tin)
            cout << "TIN: genes " << tin.n_genes << ", measured " << tin.n_measured << ", eligible " << tin_values.eligible << ", model_bases " << tin.model_bases
                 << ", covered_bases " << tin.covered_bases << ", depth_sum " << tin.depth_sum << ", median " << tin_values.median << ", tin_ms " << tin.tin_ms << endl;
        if (o.cycles)
            cout << "Cycles: records " << cycles.records << ", no_seq " << cycles.no_seq_records << ", no_qual " << cycles.no_qual_records << ", bases " << cycles.bases
                 << ", beyond " << cycles.beyond_bases << ", clamped " << cycles.clamped_quals << ", cycles_ms " << cycles.cycles_ms << endl;
        if (o.mismatches)
            cout << "Mismatches: records " << mismatches.records << ", no_reference " << mismatches.no_reference_records << ", low_mapq " << mismatches.low_mapq_records
                 << ", no_seq " << mismatches.no_seq_records << ", inconsistent " << mismatches.inconsistent_records << ", compared " << mismatches.compared
                 << ", mismatched " << mismatches.mismatched << ", uncompared " << mismatches.uncompared << ", inserted " << mismatches.inserted << ", clipped " << mismatches.clipped
                 << ", deletions " << mismatches.deletions << ", beyond " << mismatches.beyond_bases << ", mismatch_ms " << mismatches.mismatch_ms << endl;
        if (o.has_alleles)
            cout << "Alleles: sites " << alleles.n_sites << ", skipped_lines " << S.sites.skipped_lines << ", off_header_lines " << sites.off_header_lines << ", duplicate_lines "
                 << sites.duplicate_lines << ", records " << alleles.records << ", hit_records " << alleles.hit_records << ", observations " << alleles.observations << ", off_contig "
                 << alleles.off_contig_records << ", low_mapq " << alleles.low_mapq_records << ", no_seq " << alleles.no_seq_records << ", inconsistent " << alleles.inconsistent_records
                 << ", no_qual " << alleles.no_qual_records << ", alleles_ms " << alleles.alleles_ms << endl;
        cout << "Estimating library complexity..." << endl;
        cout << "Generating report" << endl;
    }
    ReportConfig cfg;
    cfg.output_dir = out_dir; cfg.sample_name = sample.name; cfg.sample_given = sample.name_given;
    cfg.use_rpkm = o.rpkm; cfg.write_coverage = o.coverage; cfg.detection_threshold = (unsigned)o.detection;
    cfg.filter_tags = o.tags;
    const std::string junctions_path = out_dir + "/" + sample.name + ".junctions.tsv";
    if (o.junctions && !S.junction_index.built) S.junction_index.build(ann);
    if (o.bedgraph) {
        // the track's text comes from the context window by window: written here, on the report path, before the context's next reset
        uint64_t bytes = 0; double secs = 0; bool io_failed = false;
        rc = write_bedgraph(gpu, out_dir + "/" + sample.name + ".coverage.bedgraph", track.n_rows, bytes, secs, io_failed);
        if (rc != RSQC_OK) return gpu_failed(rc);
        if (io_failed) { cerr << S.prefix << "Filesystem error:  cannot write " << out_dir << "/" << sample.name << ".coverage.bedgraph" << endl; return 8; }
        if (o.verbosity) cout << "Track text: rows " << track.n_rows << ", bytes " << bytes << ", seconds " << secs << endl;
    }
    if (o.gene_body && !write_gene_body(out_dir + "/" + sample.name + ".gene_body.tsv", gene_body_rows)) {
        cerr << S.prefix << "Filesystem error:  cannot write " << out_dir << "/" << sample.name << ".gene_body.tsv" << endl; return 8;
    }
    if (o.tin) {
        const std::string stem = out_dir + "/" + sample.name;
        if (!write_tin(stem + ".tin.tsv", ann.gene_list, S.gene_body.gene_len.data(), tin_rows, tin_values)) { cerr << S.prefix << "Filesystem error:  cannot write " << stem << ".tin.tsv" << endl; return 8; }
        if (!write_tin_summary(stem + ".tin_summary.tsv", tin_values)) { cerr << S.prefix << "Filesystem error:  cannot write " << stem << ".tin_summary.tsv" << endl; return 8; }
    }
    if (o.cycles) {
        const std::string stem = out_dir + "/" + sample.name;
        if (!write_cycle_bases(stem + ".cycle_bases.tsv", cycle_base)) { cerr << S.prefix << "Filesystem error:  cannot write " << stem << ".cycle_bases.tsv" << endl; return 8; }
        if (!write_cycle_quality(stem + ".cycle_quality.tsv", cycle_base, cycle_qual)) { cerr << S.prefix << "Filesystem error:  cannot write " << stem << ".cycle_quality.tsv" << endl; return 8; }
    }
    if (o.mismatches) {
        const std::string stem = out_dir + "/" + sample.name;
        if (!write_mismatch_cycles(stem + ".mismatch_cycles.tsv", mismatch_cyc)) { cerr << S.prefix << "Filesystem error:  cannot write " << stem << ".mismatch_cycles.tsv" << endl; return 8; }
        if (!write_mismatch_types(stem + ".mismatch_types.tsv", mismatch_subst)) { cerr << S.prefix << "Filesystem error:  cannot write " << stem << ".mismatch_types.tsv" << endl; return 8; }
        if (!write_mismatch_quality(stem + ".mismatch_quality.tsv", mismatch_byq)) { cerr << S.prefix << "Filesystem error:  cannot write " << stem << ".mismatch_quality.tsv" << endl; return 8; }
    }
    if (o.has_alleles && !write_allele_counts(out_dir + "/" + sample.name + ".allele_counts.tsv", bam_contigs, S.sites, sites, allele_counts)) {
        cerr << S.prefix << "Filesystem error:  cannot write " << out_dir << "/" << sample.name << ".allele_counts.tsv" << endl; return 8;
    }
    if (!S.async_reports) {
        S.t_rep0 = Clock::now();
        write_reports(cfg, ann, res, visit);
        if (o.junctions) write_junctions(junctions_path, ann, S.junction_index, junctions);
        S.t_rep1 = Clock::now();
        return 0;
    }
    // a cohort: the writer gets a copy of what it reads, the context goes on to the next sample.  The row is the job's from
    // here on (the caller reads it after finish_reports()).
    S.finish_reports();
    timer.armed = false;
    std::shared_ptr<ResultsCopy> copy(new ResultsCopy(res));
    std::shared_ptr<JunctionCopy> jcopy(o.junctions ? new JunctionCopy(junctions) : nullptr);      // (the context's arrays end with its next reset)
    const JunctionIndex *jindex = &S.junction_index;
    const std::string prefix = S.prefix;
    S.report_job = std::async(std::launch::async, [cfg, &ann, copy, jcopy, jindex, junctions_path, visit, &row, t_open, prefix] {
        try { write_reports(cfg, ann, copy->res, visit); if (jcopy) write_junctions(junctions_path, ann, *jindex, jcopy->table); }
        catch (...) { row.exit_code = explain_exception(prefix); }
        row.seconds = seconds_between(t_open, Clock::now());
    });
    return 0;
}

// ---- --bam-list: the samples of a list through one context, back to back
struct ListError : std::runtime_error { using std::runtime_error::runtime_error; };      // exit 10: the list file itself

std::vector<Sample> read_bam_list(const std::string &list_path) {
    std::ifstream f(list_path);
    if (!f.is_open()) throw ListError("Unable to open the sample list: " + list_path);
    const size_t slash = list_path.find_last_of('/');
    const std::string dir = slash == std::string::npos ? "" : list_path.substr(0, slash + 1);
    std::vector<Sample> samples;
    std::string line;
    while (std::getline(f, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        const size_t tab = line.find('\t');
        Sample s;
        s.path = line.substr(0, tab);
        if (s.path.empty()) continue;
        s.name = tab == std::string::npos ? "" : line.substr(tab + 1);
        s.name_given = !s.name.empty();
        if (s.name.empty()) s.name = basename_of(s.path);                  // the one-sample rule: the path's basename
        if (s.path[0] != '/') s.path = dir + s.path;
        samples.push_back(std::move(s));
    }
    if (samples.empty()) throw ValidationError("The sample list is empty: " + list_path);
    std::map<std::string, int> seen;
    for (auto &s : samples) if (seen[s.name]++) throw ValidationError("Sample name appears twice in the list: " + s.name);
    return samples;
}

int run_cohort(const Options &o, Annotation &ann, Session &S, std::vector<Sample> &samples, const std::string &out_dir) {
    using std::cerr; using std::endl;
    std::vector<SampleRow> rows(samples.size());
    S.async_reports = true;
    S.keep_fasta = true;
    const Options *op = &o;
    auto open_ahead = [op](Sample &s) { const std::string p = s.path; s.opened = std::async(std::launch::async, [p, op] { return open_input(p, *op); }); };
    open_ahead(samples[0]);
    for (size_t k = 0; k < samples.size(); ++k) {
        // the next sample is opened, sniffed and its header read beside this one's decode; none of its records is submitted
        // before this one has been finalized and the context reset (run_sample)
        if (k + 1 < samples.size()) open_ahead(samples[k + 1]);
        SampleRow &row = rows[k];
        row.sample = samples[k].name; row.input = samples[k].path;
        S.prefix = samples[k].name + ": ";
        int code;
        try { code = run_sample(o, ann, S, samples[k], out_dir, row); }
        catch (...) { code = explain_exception(S.prefix); }
        if (code) row.exit_code = code;
        if (row.fatal) {                                // a GPU failure: nothing further is started on the device
            cerr << "Stopping after " << samples[k].name << ": the GPU failed; " << samples.size() - k - 1 << " samples were not run" << endl;
            break;
        }
    }
    S.finish_reports();
    int first = 0; bool stopped = false;
    std::ofstream t(out_dir + "/cohort.tsv");
    t << "sample\tinput\tformat\trecords\tseconds\texit_code\n";
    for (size_t k = 0; k < samples.size(); ++k) {
        SampleRow &row = rows[k];
        if (stopped) { row.sample = samples[k].name; row.input = samples[k].path; row.exit_code = 10; }
        t << row.sample << '\t' << row.input << '\t' << row.format << '\t' << row.records << '\t' << row.seconds << '\t' << row.exit_code << '\n';
        if (row.exit_code && !first) first = row.exit_code;
        if (row.fatal) stopped = true;
    }
    return first;
}

// ---- `--gpus N`: one input sharded by contig over several contexts (the first is the session's); the header has been checked and
// the annotation flattened for it, `bam` holds the index
struct ShardedRun { const Options &o; Annotation &ann; Session &S; Input &in; const std::vector<int> &devices; BamReader &bam; std::string out_dir, sample_name; };
int run_sharded(ShardedRun R) {
    using std::cerr; using std::cout; using std::endl;
    const Options &o = R.o; Annotation &ann = R.ann; Session &S = R.S; BamReader &bam = R.bam;
    const std::string &bam_path = R.in.path;
    const rsqc_params &P = S.P;
    const int n_ref_bam = (int)R.in.contigs.size();
    R.in.reader.reset();                                             // (every shard's thread opens the file itself)
    std::vector<Shard> shards(R.devices.size());
    uint64_t tail_voff = 0;
    {
        // longest-processing-time packing of the contigs on the index's record counts (compressed bytes when an index
        // carries no counts); the unplaced tail goes to the lightest shard
        const auto &idx = bam.index();
        std::vector<std::pair<uint64_t, int>> byload;
        for (int c2 = 0; c2 < n_ref_bam && (size_t)c2 < idx.size(); ++c2) if (idx[(size_t)c2].present) {
            const uint64_t load = idx[(size_t)c2].n_records ? idx[(size_t)c2].n_records : ((idx[(size_t)c2].end >> 16) - (idx[(size_t)c2].beg >> 16)) / 24 + 1;
            byload.emplace_back(load, c2);
            tail_voff = std::max(tail_voff, idx[(size_t)c2].end);
        }
        std::sort(byload.begin(), byload.end(), [](const std::pair<uint64_t, int> &x, const std::pair<uint64_t, int> &y) { return x.first != y.first ? x.first > y.first : x.second < y.second; });
        for (auto &bl : byload) {
            size_t best = 0;
            for (size_t g = 1; g < shards.size(); ++g) if (shards[g].load < shards[best].load) best = g;
            shards[best].contigs.push_back(bl.second); shards[best].load += bl.first;
        }
        size_t lightest = 0;
        for (size_t g = 1; g < shards.size(); ++g) if (shards[g].load < shards[lightest].load) lightest = g;
        shards[lightest].tail = true;
        for (auto &sh : shards) std::sort(sh.contigs.begin(), sh.contigs.end());
    }
    S.t_gpu0 = Clock::now();
    int rc = S.gpu_ready.get();
    S.t_gpu1 = Clock::now();
    if (rc != RSQC_OK) { cerr << "Unable to initialise the GPU hot path: " << rsqc_strerror(rc) << endl; return 10; }
    // (every exit below releases the contexts of the other shards and the exchange group; the first context is the session's)
    rsqc_group *xgroup = nullptr;
    std::future<int> group_ready;
    struct Release { std::vector<Shard> &shards; rsqc_group *&xgroup; std::future<int> &group_ready;
                     ~Release() { if (group_ready.valid()) (void)group_ready.get(); rsqc_group_destroy(xgroup); for (size_t g = 1; g < shards.size(); ++g) if (shards[g].gpu) rsqc_destroy(shards[g].gpu); } } release{shards, xgroup, group_ready};
    std::vector<std::vector<uint8_t>> owned_masks(shards.size());
    for (size_t g = 0; g < shards.size(); ++g) {
        Shard &sh = shards[g];
        sh.device = R.devices[g];
        if (g == 0) sh.gpu = S.gpu;
        else { rsqc_params Pg = P; Pg.device = sh.device; if ((rc = rsqc_create(&Pg, &sh.gpu)) != RSQC_OK) { cerr << "Unable to initialise GPU " << sh.device << ": " << rsqc_strerror(rc) << endl; return 10; } }
    }
    // the exchange group: the RCCL communicators come up HERE, on a thread beside the annotation upload and
    // the feeders' set-up -- not inside the `Average Reads/Sec` window that the end-of-file reduction belongs to
    {
        std::vector<rsqc_ctx *> members;
        for (auto &sh : shards) members.push_back(sh.gpu);
        group_ready = std::async(std::launch::async, [members, &xgroup]() mutable { return rsqc_group_create(members.data(), (int)members.size(), &xgroup); });
    }
    std::vector<rsqc_ctx *> ctxs;
    for (size_t g = 0; g < shards.size(); ++g) {
        Shard &sh = shards[g];
        owned_masks[g].assign(ann.contig_names.size(), 0);
        for (int c2 : sh.contigs) owned_masks[g][(size_t)c2] = 1;
        if (int code = set_annotation_and_bed(o, ann, sh.gpu, owned_masks[g].data(), g == 0, "", rc)) return code;
        ctxs.push_back(sh.gpu);
    }
    if (o.has_fasta) if (int code = set_reference(S, ann, ctxs, rc)) return code;

    // device decode needs exact range ends from the index
    bool device_decode = device_decode_wanted(R.in.is_stream);
    if (device_decode) for (auto &r : bam.index()) if (r.present && !r.end) device_decode = false;
    if (device_decode && !(getenv("RSQC_DECODE_PRERESERVE") && !atoi(getenv("RSQC_DECODE_PRERESERVE")))) {
        // the device's window buffers are set up before the loop, like the host path's page-locked batches
        for (auto &sh : shards) {
            rsqc_decode_params dp = decode_params(o, n_ref_bam, 0);
            dp.reserve_inflated_bytes = decode_reserve_bytes(R.in.file_size);
            rsqc_decode_info none{};
            if ((rc = rsqc_decode_begin(sh.gpu, &dp)) != RSQC_OK || (rc = rsqc_decode_end(sh.gpu, &none)) != RSQC_OK) {
                cerr << "Unable to set up the device decode: " << rsqc_last_error(sh.gpu) << endl; return 10;
            }
        }
    }
    // the feeders' chunk buffers are page-locked here, before the loop (see run_sample)
    std::vector<std::unique_ptr<BgzfFeeder>> feeders;
    if (device_decode) {
        const int cpu_share_threads = feeder_cpu_threads();
        for (size_t g = 0; g < shards.size(); ++g) {
            feeders.emplace_back(new BgzfFeeder());
            if (!feeders.back()->open(bam_path)) { cerr << "Unable to open BAM file: " << bam_path << endl; return 10; }
            if (cpu_share_threads > 0)             // (a shard's calls are a contig at a time: a fraction of the room)
                feeders.back()->set_cpu_share(std::max(1, cpu_share_threads / (int)shards.size()), 0.15, 0.5, ((uint64_t)1 << 30) / shards.size());
            if (feeder_prepin()) feeders.back()->reserve(std::max<size_t>(feeder_chunk_bytes() / shards.size(), (size_t)16 << 20));
        }
        feeders[0]->read_threads = getenv("RSQC_FEED_READ_THREADS") ? std::max(1, atoi(getenv("RSQC_FEED_READ_THREADS"))) : std::max(1, std::min(8, effective_cpus() / 2));
    }
    if (o.verbosity) cout << "Parsing bam..." << endl;
    const size_t BATCH = getenv("RSQC_BATCH") ? (size_t)atol(getenv("RSQC_BATCH")) : (size_t)1 << 21;
    std::vector<int> visit;
    unsigned long long alignmentCount = 0;
    bool warned_unsorted = false;
    ShardMerge merged;
    double group_init_ms = 0.0;
    {                                                        // (before the window opens)
        if ((rc = group_ready.get()) != RSQC_OK) { cerr << "Unable to set up the multi-GPU exchange: " << rsqc_strerror(rc) << endl; return 10; }
        int uses = 0; const char *note = "";
        rsqc_group_info(xgroup, &uses, &group_init_ms, nullptr, &note);
        if (o.verbosity > 1) cout << "Exchange group of " << shards.size() << " GPUs ready in " << group_init_ms << " ms ("
                                  << (uses ? "RCCL communicators" : (std::string("peer copies: ") + note).c_str()) << "), before the BAM loop" << endl;
    }
    const Clock::time_point tb0 = Clock::now();
    {
        // one reader thread per GPU; the decode threads of the process are shared out between them
        int budget = 2 * effective_cpus();
        if (const char *e = getenv("RSQC_HOST_THREADS")) budget = atoi(e);
        const int per = std::max(2, budget / (int)shards.size());
        std::vector<std::thread> th;
        for (auto &sh : shards) th.emplace_back(shard_worker, std::ref(sh), std::cref(bam_path), std::cref(o), per, std::cref(bam.index()), n_ref_bam, tail_voff, BATCH, device_decode ? feeders[(size_t)(&sh - shards.data())].get() : nullptr);
        for (auto &t : th) t.join();
    }
    rc = RSQC_OK;
    for (auto &sh : shards) {
        alignmentCount += sh.n_records;
        if (sh.rc != RSQC_OK && rc == RSQC_OK) { rc = sh.rc; if (rc != RSQC_ERR_BAD_CIGAR && rc != RSQC_ERR_EMPTY_MEDIAN) cerr << "GPU " << sh.device << ": " << sh.error << endl; }
        if (o.verbosity) for (auto &nm : sh.bad_refid) cerr << "Unrecognized RefID on alignment: " << nm << endl;
        if (sh.unsorted && !warned_unsorted) { cerr << kUnsortedWarning << endl; warned_unsorted = true; }
    }
    for (int c2 = 0; c2 < n_ref_bam && (size_t)c2 < bam.index().size(); ++c2) if (bam.index()[(size_t)c2].present) {
        visit.push_back(c2);
        if (o.has_fasta && (size_t)c2 < S.in_fasta.size() && !S.in_fasta[(size_t)c2])
            cerr << "Warning: Provided Fasta does not contain chromosome " << ann.contig_names[(size_t)c2]
                 << ". No GC statistics will be collected for this chromosome" << endl;
    }
    // the exchange step: result ranges summed onto the first GPU, order-dependent outputs composed from the summaries
    int used_rccl = 0;
    if (rc == RSQC_OK) {
        rc = rsqc_group_reduce(xgroup, &used_rccl);
        if (rc != RSQC_OK) cerr << rsqc_last_error(shards[0].gpu) << endl;
    }
    if (rc == RSQC_OK) { std::string merr; rc = merge_shards(shards, P.fragment_samples, merged, merr); if (rc != RSQC_OK) cerr << merr << endl; }
    if (o.verbosity > 1) {
        cout << "Alignments processed: " << alignmentCount << " on " << shards.size() << " GPUs (";
        for (size_t g = 0; g < shards.size(); ++g) cout << (g ? ", " : "") << shards[g].n_records;
        double reduce_ms = 0.0; rsqc_group_info(xgroup, nullptr, nullptr, &reduce_ms, nullptr);
        cout << " records); shards summed by " << (used_rccl ? "RCCL ncclReduce" : "peer copies") << " in " << reduce_ms << " ms (group set-up " << group_init_ms << " ms, outside the window)" << endl;
    }
    rsqc_results res{};
    if (rc == RSQC_OK) {
        rc = rsqc_refresh_results(S.gpu, &res);
        res.read_length = merged.read_length;
        res.n_fragment_sizes = (uint32_t)merged.fsize.size(); res.fragment_size = merged.fsize.data(); res.fragment_count = merged.fcount.data();
        res.fragment_samples_remaining = merged.remaining;
    }
    const Clock::time_point tb1 = Clock::now();
    if (rc == RSQC_ERR_BAD_CIGAR) throw std::invalid_argument("Unrecognized Cigar Op ");
    if (rc == RSQC_ERR_EMPTY_MEDIAN) throw std::range_error("Cannot compute median of an empty list");
    if (rc != RSQC_OK) { cerr << rsqc_strerror(rc) << ": " << rsqc_last_error(S.gpu) << endl; return 10; }
    if (o.verbosity) {
        const double secs = seconds_between(tb0, tb1);
        cout << "Time Elapsed: " << secs << "; Alignments processed: " << alignmentCount << endl;
        if (o.verbosity > 1) cout << "Average Reads/Sec: " << (double)alignmentCount / secs << endl;
        if (o.verbosity > 1 && device_decode) cout << "(decode: BGZF inflate and record parsing on the GPU)" << endl;
        cout << "Estimating library complexity..." << endl;
        cout << "Generating report" << endl;
    }
    ReportConfig cfg;
    cfg.output_dir = R.out_dir; cfg.sample_name = R.sample_name; cfg.sample_given = o.has_sample;
    cfg.use_rpkm = o.rpkm; cfg.write_coverage = o.coverage; cfg.detection_threshold = (unsigned)o.detection;
    cfg.filter_tags = o.tags;
    const Clock::time_point tr0 = Clock::now();
    write_reports(cfg, ann, res, visit);
    const Clock::time_point tr1 = Clock::now();
    if (group_ready.valid()) (void)group_ready.get();
    rsqc_group_destroy(xgroup); xgroup = nullptr;
    for (auto &sh : shards) { rsqc_destroy(sh.gpu); sh.gpu = nullptr; }
    S.gpu = nullptr;                                                       // (shard 0's context was the session's)
    if (o.verbosity > 1)
        // where the wall time outside the reference's `Average Reads/Sec` window goes (extension; the window itself is above)
        cout << "Wall time: " << seconds_between(S.t_start, Clock::now()) << " s = GTF " << seconds_between(S.t_gtf0, S.t_gtf1)
             << " + waiting for the GPU context " << seconds_between(S.t_gpu0, S.t_gpu1) << " + index / annotation upload / buffers " << seconds_between(S.t_gpu1, tb0)
             << " + BAM loop " << seconds_between(tb0, tb1) << " + reports " << seconds_between(tr0, tr1) << " + release " << seconds_between(tr1, Clock::now())
             << " (the GPU context and the page-locked feed buffers come up beside the GTF parse)" << endl;
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    using std::cerr; using std::cout; using std::endl;
    Session S;
    int code = 0;
    try {
        Options o = parse(argc, argv);
        if (o.version) { cout << VERSION << endl; return 0; }
        const size_t n_pos = o.has_bam_list ? 2 : 3;
        if (o.positional.size() < 1) throw ValidationError("No GTF file provided");
        if (!o.has_bam_list && o.positional.size() < 2) throw ValidationError("No BAM file provided");
        if (o.positional.size() < n_pos) throw ValidationError("No output directory provided");
        if (o.positional.size() > n_pos) throw ParseError("Passed in argument, but no positional arguments were ready to receive it: " + o.positional[n_pos]);
        const std::string gtf_path = o.positional[0], bam_path = o.has_bam_list ? "" : o.positional[1], out_dir = o.positional[n_pos - 1];
        int strand = RSQC_STRAND_UNKNOWN;
        if (o.has_stranded) {
            if (o.stranded == "RF" || o.stranded == "rf") strand = RSQC_STRAND_REVERSE;
            else if (o.stranded == "FR" || o.stranded == "fr") strand = RSQC_STRAND_FORWARD;
            else throw ValidationError("--stranded argument must be in {'RF', 'rf', 'FR', 'fr'}");
        }
        if (o.has_umi_tag && o.has_umi_qname) throw ValidationError("--umi-tag and --umi-qname name two sources of the UMI: give one");
        if (o.has_umi_tag && o.umi_tag.size() != 2) throw ValidationError("--umi-tag takes the two characters of an aux tag (e.g. RX)");
        if (o.has_umi_qname && o.umi_sep.size() != 1) throw ValidationError("--umi-qname takes one separator character (default _)");
        if (o.has_umi_edits && o.umi_edits != "0" && o.umi_edits != "1") throw ValidationError("--umi-edits takes 0 (exact match) or 1 (UMIs one substitution apart are merged)");
        if (o.has_umi_edits && !o.has_umi_tag && !o.has_umi_qname) throw ValidationError("--umi-edits needs the source of the UMI: --umi-tag or --umi-qname");
        if (o.mark_duplicates) {
            // the whole input must be resident: the stage runs on the collection of --sort, in ONE context
            if (o.has_bam_list) throw ValidationError("--mark-duplicates takes one input (it cannot be combined with --bam-list)");
            bool many_gpus = o.gpus > 1 || (getenv("RSQC_GPUS") && atoi(getenv("RSQC_GPUS")) > 1);
            if (const char *e = getenv("RSQC_GPU_LIST")) many_gpus = many_gpus || strchr(e, ',') != nullptr;
            if (many_gpus) throw ValidationError("--mark-duplicates runs on one GPU (it implies --sort: it cannot be combined with --gpus, RSQC_GPUS or RSQC_GPU_LIST above one)");
        }
        if (o.sort) {
            // the sort sits in front of ONE context's ordinary submits: contig sharding needs the index of a sorted file, cohorts are not collected
            if (o.has_bam_list) throw ValidationError("--sort takes one input (it cannot be combined with --bam-list)");
            bool many_gpus = o.gpus > 1 || (getenv("RSQC_GPUS") && atoi(getenv("RSQC_GPUS")) > 1);
            if (const char *e = getenv("RSQC_GPU_LIST")) many_gpus = many_gpus || strchr(e, ',') != nullptr;
            if (many_gpus) throw ValidationError("--sort runs on one GPU (--gpus, RSQC_GPUS and RSQC_GPU_LIST shard a coordinate-sorted, indexed BAM)");
        }
        if (o.bedgraph) {
            // one difference array per context: the arrays of shards would need adding up, and that path is not built
            bool many_gpus = o.gpus > 1 || (getenv("RSQC_GPUS") && atoi(getenv("RSQC_GPUS")) > 1);
            if (const char *e = getenv("RSQC_GPU_LIST")) many_gpus = many_gpus || strchr(e, ',') != nullptr;
            if (many_gpus) throw ValidationError("--bedgraph runs on one GPU (it cannot be combined with --gpus, RSQC_GPUS or RSQC_GPU_LIST above one)");
        }
        if (o.gene_body) {
            // the stage reads ONE context's difference array, like --bedgraph
            bool many_gpus = o.gpus > 1 || (getenv("RSQC_GPUS") && atoi(getenv("RSQC_GPUS")) > 1);
            if (const char *e = getenv("RSQC_GPU_LIST")) many_gpus = many_gpus || strchr(e, ',') != nullptr;
            if (many_gpus) throw ValidationError("--gene-body runs on one GPU (it cannot be combined with --gpus, RSQC_GPUS or RSQC_GPU_LIST above one)");
        }
        if (o.tin) {
            // the stage reads ONE context's difference array, like --gene-body (the rows are contig-local, but the track is one-GPU)
            bool many_gpus = o.gpus > 1 || (getenv("RSQC_GPUS") && atoi(getenv("RSQC_GPUS")) > 1);
            if (const char *e = getenv("RSQC_GPU_LIST")) many_gpus = many_gpus || strchr(e, ',') != nullptr;
            if (many_gpus) throw ValidationError("--tin runs on one GPU (it cannot be combined with --gpus, RSQC_GPUS or RSQC_GPU_LIST above one)");
        }
        if (o.cycles) {
            // two tables per context: the tables of shards would only need adding up, but that path is not built
            bool many_gpus = o.gpus > 1 || (getenv("RSQC_GPUS") && atoi(getenv("RSQC_GPUS")) > 1);
            if (const char *e = getenv("RSQC_GPU_LIST")) many_gpus = many_gpus || strchr(e, ',') != nullptr;
            if (many_gpus) throw ValidationError("--cycles runs on one GPU (it cannot be combined with --gpus, RSQC_GPUS or RSQC_GPU_LIST above one)");
        }
        if (o.has_mismatches_mapq && !o.mismatches) throw ValidationError("--mismatches-mapq needs --mismatches");
        if (o.has_mismatches_mapq && (o.mismatches_mapq < 0 || o.mismatches_mapq > 255)) throw ValidationError("--mismatches-mapq takes a mapping quality of 0..255");
        if (o.mismatches) {
            if (!o.has_fasta) throw ValidationError("--mismatches needs the reference: give --fasta");
            // one set of tables and one packed reference per context: the tables of shards would only need adding up, but that path is not built
            bool many_gpus = o.gpus > 1 || (getenv("RSQC_GPUS") && atoi(getenv("RSQC_GPUS")) > 1);
            if (const char *e = getenv("RSQC_GPU_LIST")) many_gpus = many_gpus || strchr(e, ',') != nullptr;
            if (many_gpus) throw ValidationError("--mismatches runs on one GPU (it cannot be combined with --gpus, RSQC_GPUS or RSQC_GPU_LIST above one)");
        }
        if ((o.has_allele_mapq || o.has_allele_baseq) && !o.has_alleles) throw ValidationError("--allele-mapq and --allele-baseq need --alleles");
        if (o.has_allele_mapq && (o.allele_mapq < 0 || o.allele_mapq > 255)) throw ValidationError("--allele-mapq takes a mapping quality of 0..255");
        if (o.has_allele_baseq && (o.allele_baseq < 0 || o.allele_baseq > 93)) throw ValidationError("--allele-baseq takes a base quality of 0..93");
        if (o.has_alleles) {
            // one table per context: the tables of shards would only need adding up, but that path is not built
            bool many_gpus = o.gpus > 1 || (getenv("RSQC_GPUS") && atoi(getenv("RSQC_GPUS")) > 1);
            if (const char *e = getenv("RSQC_GPU_LIST")) many_gpus = many_gpus || strchr(e, ',') != nullptr;
            if (many_gpus) throw ValidationError("--alleles runs on one GPU (it cannot be combined with --gpus, RSQC_GPUS or RSQC_GPU_LIST above one)");
        }
        if (o.junctions) {
            // one table per context: the per-contig tables of shards would only need concatenating, but that path is not built
            bool many_gpus = o.gpus > 1 || (getenv("RSQC_GPUS") && atoi(getenv("RSQC_GPUS")) > 1);
            if (const char *e = getenv("RSQC_GPU_LIST")) many_gpus = many_gpus || strchr(e, ',') != nullptr;
            if (many_gpus) throw ValidationError("--junctions runs on one GPU (it cannot be combined with --gpus, RSQC_GPUS or RSQC_GPU_LIST above one)");
        }
        // a cohort: the list is read and checked before anything else is touched
        std::vector<Sample> samples;
        if (o.has_bam_list) {
            if (o.has_sample) throw ValidationError("--sample cannot name the samples of a --bam-list (give the names in the list's second column)");
            bool many_gpus = o.gpus > 1 || (getenv("RSQC_GPUS") && atoi(getenv("RSQC_GPUS")) > 1);
            if (const char *e = getenv("RSQC_GPU_LIST")) many_gpus = many_gpus || strchr(e, ',') != nullptr;
            if (many_gpus) throw ValidationError("--bam-list runs on one GPU (--gpus, RSQC_GPUS and RSQC_GPU_LIST shard ONE input)");
            try { samples = read_bam_list(o.bam_list); }
            catch (ListError &e) { cerr << e.what() << endl; return 10; }
        }
        if (o.tags.size() > RSQC_MAX_FILTER_TAGS) { cerr << "at most " << RSQC_MAX_FILTER_TAGS << " --tag filters are supported" << endl; return 7; }

        rsqc_params &P = S.P;
        P.abi_version = RSQC_ABI_VERSION;
        P.device = getenv("RSQC_DEVICE") ? atoi(getenv("RSQC_DEVICE")) : 0;
        if (const char *e = getenv("RSQC_GPU_LIST")) if (*e) P.device = atoi(e);       // the first shard's context runs on the list's first device
        P.mapq_threshold = o.has_mapq ? (uint32_t)o.mapq : (o.legacy ? 4u : 255u);     // src/RNASeQC.cpp:90
        P.legacy = o.legacy ? 1 : 0;
        P.base_mismatch = (uint32_t)o.base_mismatch;
        P.chimeric_distance = (int32_t)o.chimeric_distance; P.fragment_samples = (uint32_t)o.fragment_samples;
        P.bias_offset = (int32_t)o.bias_offset; P.bias_window = (int32_t)o.bias_window; P.bias_gene_length = o.bias_gene_length;
        P.coverage_mask = (uint32_t)o.coverage_mask; P.stranded = strand; P.unpaired = o.unpaired; P.exclude_chimeric = o.exclude_chimeric;
        P.n_filter_tags = (int32_t)o.tags.size();

        // the HIP context comes up (~0.3 s) while the GTF is being parsed; its status is looked at where the
        // reference would first need it, so input errors keep their precedence and exit codes
        {
            Session *sp = &S;
            S.gpu_ready = std::async(std::launch::async, [sp] { return rsqc_create(&sp->P, &sp->gpu); });
        }
        // ... and so do the page-locked chunk buffers of the device decode's feeder: sized for the input, or for the largest
        // BAM of a cohort (every later file goes through the same buffers)
        S.t_start = Clock::now();
        {
            std::string feed_for;
            if (!o.has_bam_list) {
                struct stat st;
                const bool is_stream = stat(bam_path.c_str(), &st) == 0 && !S_ISREG(st.st_mode);
                if (device_decode_wanted(is_stream) && sniff_file(bam_path) == InputFormat::Bam && o.gpus <= 1 && !getenv("RSQC_GPUS") && !getenv("RSQC_GPU_LIST")) feed_for = bam_path;
            } else {
                for (auto &s : samples) {
                    struct stat st;
                    if (stat(s.path.c_str(), &st) != 0 || !S_ISREG(st.st_mode) || (uint64_t)st.st_size <= S.reserve_file_size) continue;
                    if (!device_decode_wanted(false) || sniff_file(s.path) != InputFormat::Bam) continue;
                    S.reserve_file_size = (uint64_t)st.st_size; feed_for = s.path;
                }
            }
            if (!feed_for.empty() && feeder_prepin()) start_early_feeder(S, feed_for);
        }
        S.t_gtf0 = Clock::now();
        Annotation ann;
        ann.legacy = o.legacy;
        if (o.has_fasta) {                                                    // src/RNASeQC.cpp:111-121: GTF openable, then Fasta::open
            { std::ifstream probe(gtf_path); if (!probe.is_open()) { cerr << "Unable to open GTF file: " << gtf_path << endl; return 10; } }
            S.fasta.open(o.fasta);                                            // FileError -> 10
            if (o.mismatches) S.keep_fasta = true;                            // (--mismatches packs the bases for the input's header, and the host reader compares with them)
            for (auto &e : S.fasta.index) ann.chromosome(e.name);             // the index names join chromosomeMap first (src/Fasta.cpp:93-94)
            if (o.verbosity > 1) cout << "A FASTA has been provided. This will enable GC-content statistics but adds additional runtime and memory costs" << endl;
            Session *sp = &S;
            S.fasta_loaded = std::async(std::launch::async, [sp] { sp->fasta.load(sp->fasta_seq); });   // read beside the GTF parse
        }
        if (o.verbosity) cout << "Reading GTF Features..." << endl;
        ann.load_gtf(gtf_path);                                               // FileError -> 10, GtfError -> 11
        if (!(ann.gene_list.size() && ann.exon_list.size())) {
            cerr << "There were either no genes or no exons in the GTF" << endl;
            cerr << ann.gene_list.size() << " genes parsed" << endl << ann.exon_list.size() << " exons parsed" << endl;
            return 11;
        }
        S.t_gtf1 = Clock::now();
        if (o.verbosity) cout << "Finished processing GTF in " << seconds_between(S.t_gtf0, S.t_gtf1) << " seconds" << endl;
        S.gtf_chrom.assign(ann.chrom_name.size() + 1, 0);
        for (auto &r : ann.rows) if (!r.excluded) S.gtf_chrom[(size_t)r.chrom] = 1;
        if (o.has_bed) {
            if (o.verbosity) cout << "Parsing BED intervals for fragment size computations..." << endl;
            ann.load_bed(o.bed);
        }
        if (o.has_alleles) {                                                  // parsed once; resolved against every input's header
            std::string error;
            const int bad = read_sites(o.alleles, S.sites, error);
            if (bad == 10) { cerr << "Unable to open the sites: " << error << endl; return 10; }
            if (bad) { cerr << "Failed to parse the sites: " << error << endl; return 11; }
        }
        S.base_chrom_id = ann.chrom_id; S.base_chrom_name = ann.chrom_name;
        if (!make_dirs(out_dir)) { cerr << "Filesystem error:  cannot create " << out_dir << endl; return 8; }

        if (o.has_bam_list) code = run_cohort(o, ann, S, samples, out_dir);
        else {
            Sample sample;
            sample.path = bam_path; sample.name = o.has_sample ? o.sample : basename_of(bam_path); sample.name_given = o.has_sample;
            // ---- GPUs: one by default; --gpus N (or RSQC_GPUS) shards the file by contig, which needs the BAM index
            std::vector<int> devices;
            const int want = o.gpus > 0 ? o.gpus : (getenv("RSQC_GPUS") ? atoi(getenv("RSQC_GPUS")) : 1);
            if (const char *e = getenv("RSQC_GPU_LIST")) { for (const char *q = e; *q;) { devices.push_back(atoi(q)); while (*q && *q != ',') ++q; if (*q) ++q; } }
            else for (int k = 0; k < std::max(1, want); ++k) devices.push_back(P.device + k);
            bool sharded = false;
            std::unique_ptr<Input> in;
            BamReader index_reader;
            if (devices.size() > 1) {
                in = open_input(bam_path, o);
                if (!in->error.empty()) { cerr << in->error << endl; return 10; }
                if (in->sam() && o.verbosity > 1) cout << "Input: " << input_format_name(in->fmt) << " (" << in->contigs.size() << " @SQ lines), parsed on the GPU" << endl;
                if (o.verbosity > 1) cout << "Checking bam header..." << endl;
                if (!shares_contigs(S, ann, in->contigs)) { cerr << "BAM file shares no contigs with GTF" << endl; return 11; }
                flatten_for(S, ann, in->contigs);
                if (in->sam() || !index_reader.load_index(bam_path + ".bai")) {        // (SAM has no index)
                    cerr << "Warning: sharding over " << devices.size() << " GPUs needs the BAM index " << bam_path << ".bai; running on one GPU" << endl;
                    devices.resize(1);
                } else sharded = true;
            }
            if (sharded) code = run_sharded(ShardedRun{o, ann, S, *in, devices, index_reader, out_dir, sample.name});
            else {
                if (in) { std::promise<std::unique_ptr<Input>> ready; sample.opened = ready.get_future(); ready.set_value(std::move(in)); }
                SampleRow row;
                code = run_sample(o, ann, S, sample, out_dir, row);
                if (code == 0 && o.verbosity > 1) {
                    // where the wall time outside the reference's `Average Reads/Sec` window goes (extension; the window itself is above)
                    const Clock::time_point t_rel0 = Clock::now();
                    rsqc_destroy(S.gpu); S.gpu = nullptr;
                    cout << "Wall time: " << seconds_between(S.t_start, Clock::now()) << " s = GTF " << seconds_between(S.t_gtf0, S.t_gtf1)
                         << " + waiting for the GPU context " << seconds_between(S.t_gpu0, S.t_gpu1) << " + index / annotation upload / buffers " << seconds_between(S.t_gpu1, S.t_loop0)
                         << " + BAM loop " << seconds_between(S.t_loop0, S.t_loop1) << " + reports " << seconds_between(S.t_rep0, S.t_rep1) << " + release " << seconds_between(t_rel0, Clock::now())
                         << " (the GPU context and the page-locked feed buffers come up beside the GTF parse)" << endl;
                }
            }
        }
    } catch (Help &) {
        usage(cout);
        code = 4;
    } catch (ParseError &e) {
        usage(cerr); cerr << endl << "Argument parsing error: " << e.what() << endl;
        code = 5;
    } catch (ValidationError &e) {
        usage(cerr); cerr << endl << "Argument validation error: " << e.what() << endl;
        code = 6;
    } catch (...) {
        code = explain_exception("");
    }
    // nothing of the process is left on the device: the context was asked for on a thread, which is waited for first
    try { S.finish_reports(); } catch (...) {}
    if (S.gpu_ready.valid()) (void)S.gpu_ready.get();
    if (S.feed_ready.valid()) (void)S.feed_ready.get();
    if (S.gpu) rsqc_destroy(S.gpu);
    return code;
}
