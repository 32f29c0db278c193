// host_api.cpp -- thin C entry points over the CLI's host-side pieces (GTF/BED ingest, BAM decode,
// report writers) so that the CPU tests can exercise them without a GPU.  Not part of the product ABI.
#include <zlib.h>

#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "bam.hpp"
#include "bgzf_feed.hpp"
#include "gtf.hpp"
#include "report.hpp"
#include "sam_feed.hpp"

using namespace rsqc_host;
#define HAPI extern "C" __attribute__((visibility("default")))

HAPI void *host_annotation_load_ex(const char *gtf, const char *bed, const char *const *bam_contigs, int n_contigs, int legacy, int *err) {
    Annotation *a = new Annotation();
    a->legacy = legacy != 0;
    *err = 0;
    try {
        a->load_gtf(gtf);
        if (bed && *bed) a->load_bed(bed);
        std::vector<std::string> c;
        for (int i = 0; i < n_contigs; ++i) c.emplace_back(bam_contigs[i]);
        a->flatten(c);
    } catch (FileError &) { *err = 10; } catch (GtfError &) { *err = 11; } catch (BedError &) { *err = 11; } catch (...) { *err = -1; }
    if (*err) { delete a; return nullptr; }
    return a;
}
HAPI void *host_annotation_load(const char *gtf, const char *bed, const char *const *bam_contigs, int n_contigs, int *err) {
    return host_annotation_load_ex(gtf, bed, bam_contigs, n_contigs, 0, err);
}
HAPI const rsqc_annotation *host_annotation_struct(void *h) { return &((Annotation *)h)->ann; }
HAPI const rsqc_bed *host_annotation_bed(void *h) { return &((Annotation *)h)->bed; }
// the BED loader alone, rows as read (file order, before flattening): returns the number of rows, -1 = cannot open,
// -2 - n = BedError after n rows (message -> err).  chrom_index = index into the '\n'-joined names (first-sight order).
HAPI long long host_bed_read(const char *path, long long cap, int32_t *chrom_index, long long *start, long long *end,
                             char *names, long long names_cap, char *err, long long err_cap) {
    Annotation a;
    bool threw = false;
    try { a.load_bed(path); }
    catch (FileError &) { return -1; }
    catch (BedError &e) { threw = true; if (err && err_cap > 0) { strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; } }
    long long n = 0;
    for (auto &r : a.bed_rows) { if (n < cap) { chrom_index[n] = r.chrom - 1; start[n] = r.start; end[n] = r.end; } ++n; }
    std::string joined;
    for (auto &s : a.chrom_name) { joined += s; joined += '\n'; }
    if (names && names_cap > 0) { strncpy(names, joined.c_str(), (size_t)names_cap - 1); names[names_cap - 1] = 0; }
    return threw ? -2 - n : n;
}
HAPI const char *host_annotation_gene_name(void *h, int listed_gene) {
    Annotation *a = (Annotation *)h; static thread_local std::string tmp; tmp = a->gene_name(a->gene_list[(size_t)listed_gene]); return tmp.c_str();
}
HAPI const char *host_annotation_gene_id(void *h, int listed_gene) { return ((Annotation *)h)->gene_list[(size_t)listed_gene].c_str(); }
HAPI const char *host_annotation_exon_id(void *h, int exon) { return ((Annotation *)h)->exon_list[(size_t)exon].c_str(); }
HAPI long long host_annotation_coding_length(void *h, int listed_gene) {
    Annotation *a = (Annotation *)h; return a->coding_length(a->gene_list[(size_t)listed_gene]);
}
HAPI void host_annotation_free(void *h) { delete (Annotation *)h; }

HAPI int host_write_reports(void *h, const rsqc_results *r, const char *out_dir, const char *sample, int sample_given,
                            int use_rpkm, int write_coverage, unsigned detection, const char *const *tags, int n_tags,
                            const int *visit, int n_visit) {
    ReportConfig cfg;
    cfg.output_dir = out_dir; cfg.sample_name = sample; cfg.sample_given = sample_given != 0; cfg.use_rpkm = use_rpkm != 0;
    cfg.write_coverage = write_coverage != 0; cfg.detection_threshold = detection;
    for (int i = 0; i < n_tags; ++i) cfg.filter_tags.emplace_back(tags[i]);
    try { write_reports(cfg, *(Annotation *)h, *r, std::vector<int>(visit, visit + n_visit)); }
    catch (std::range_error &) { return 2; } catch (...) { return -1; }
    return 0;
}

// --junctions: the `known` rule and the table writer on a GTF and a table given as columns (contigs: the input header's names)
HAPI int host_write_junctions(const char *gtf, const char *out_path, const char *const *contigs, int n_contigs, uint64_t n, const int32_t *tid, const int32_t *start,
                              const int32_t *end, const uint32_t *reads, const uint32_t *hq_reads, const uint32_t *max_overhang) {
    try {
        Annotation a;
        a.load_gtf(gtf);
        std::vector<std::string> c;
        for (int i = 0; i < n_contigs; ++i) c.emplace_back(contigs[i]);
        a.flatten(c);
        JunctionIndex ix;
        ix.build(a);
        rsqc_junction_table t{};
        t.n = n; t.tid = tid; t.start = start; t.end = end; t.reads = reads; t.hq_reads = hq_reads; t.max_overhang = max_overhang;
        write_junctions(out_path, a, ix, t);
    } catch (FileError &) { return 10; } catch (GtfError &) { return 11; } catch (...) { return -1; }
    return 0;
}

// --tin: the host arithmetic on lengths and rows given as columns.  tin, mean_depth: [n]; stats: eligible, mean, median, stdev.
// With paths (either may be NULL) the two files are written as the command line writes them; ids: n gene ids.  0, or 8 when a
// file could not be written
HAPI int host_tin_profile(uint64_t n, const uint32_t *gene_len, const rsqc_tin_row *rows, double *tin, double *mean_depth, double *stats,
                          const char *const *ids, const char *tin_path, const char *summary_path) {
    const TinProfile p = tin_profile(gene_len, (size_t)n, rows);
    for (size_t g = 0; g < (size_t)n; ++g) { tin[g] = p.tin[g]; mean_depth[g] = p.mean_depth[g]; }
    stats[0] = (double)p.eligible; stats[1] = p.mean; stats[2] = p.median; stats[3] = p.stdev;
    std::vector<std::string> names;
    for (size_t g = 0; ids && g < (size_t)n; ++g) names.emplace_back(ids[g]);
    if (tin_path && ids && !write_tin(tin_path, names, gene_len, rows, p)) return 8;
    if (summary_path && !write_tin_summary(summary_path, p)) return 8;
    return 0;
}

// --cycles: the two files as the command line writes them (either path may be NULL), from base[2][512][5] and qual[2][512][64].
// 0, or 8 when a file could not be written
HAPI int host_cycle_files(const uint64_t *base, const uint64_t *qual, const char *bases_path, const char *quality_path) {
    if (bases_path && !write_cycle_bases(bases_path, base)) return 8;
    if (quality_path && !write_cycle_quality(quality_path, base, qual)) return 8;
    return 0;
}
// --cycles: a BAM file through the host reader with set_cycles; the sums as rsqc_cycles_add takes them.  Returns the records read, -1:
// cannot open, -2: the reader threw
HAPI long long host_bam_cycles(const char *path, int threads, size_t batch_records, uint64_t *base, uint64_t *qual, rsqc_cycle_info *info) {
    try {
        BamReader r;
        if (threads > 0) r.set_threads(threads);
        r.set_cycles(true);
        if (!r.open(path)) return -1;
        long long n = 0;
        for (;;) {
            HostBatch b;
            const size_t k = r.read_batch(b, batch_records ? batch_records : 65536);
            if (!k) break;
            n += (long long)k;
        }
        std::vector<uint64_t> vb, vq;
        r.cycles_sum(vb, vq, *info);
        memcpy(base, vb.data(), vb.size() * 8); memcpy(qual, vq.data(), vq.size() * 8);
        return n;
    } catch (std::exception &) { return -2; }
}

// --mismatches: the three files as the command line writes them (any path may be NULL), from cyc[2][512][6], subst[2][4][4] and byq[64][2].
// 0, or 8 when a file could not be written
HAPI int host_mismatch_files(const uint64_t *cyc, const uint64_t *subst, const uint64_t *byq, const char *cycles_path, const char *types_path, const char *quality_path) {
    if (cycles_path && !write_mismatch_cycles(cycles_path, cyc)) return 8;
    if (types_path && !write_mismatch_types(types_path, subst)) return 8;
    if (quality_path && !write_mismatch_quality(quality_path, byq)) return 8;
    return 0;
}
// --mismatches: a BAM file through the host reader with set_mismatches over n contigs (sequence[i] NULL: the FASTA lacks it); the sums as
// rsqc_mismatch_add takes them.  Returns the records read, -1: cannot open, -2: the reader threw
HAPI long long host_bam_mismatches(const char *path, int threads, size_t batch_records, int32_t n, const uint64_t *length, const char *const *sequence, uint32_t min_mapq,
                                   uint64_t *cyc, uint64_t *subst, uint64_t *byq, rsqc_mismatch_info *info) {
    try {
        BamReader r;
        if (threads > 0) r.set_threads(threads);
        r.set_mismatches(std::vector<const char *>(sequence, sequence + n), std::vector<uint64_t>(length, length + n), min_mapq);
        if (!r.open(path)) return -1;
        long long total = 0;
        for (;;) {
            HostBatch b;
            const size_t k = r.read_batch(b, batch_records ? batch_records : 65536);
            if (!k) break;
            total += (long long)k;
        }
        std::vector<uint64_t> vc, vs, vq;
        r.mismatches_sum(vc, vs, vq, *info);
        memcpy(cyc, vc.data(), vc.size() * 8); memcpy(subst, vs.data(), vs.size() * 8); memcpy(byq, vq.data(), vq.size() * 8);
        return total;
    } catch (std::exception &) { return -2; }
}

// --alleles: the site file against n contig names.  tid / pos take up to `cap` sites, lines3 skipped_lines, off_header_lines and
// duplicate_lines, text one "id<TAB>ref<TAB>alt<LF>" per site (or the message of a malformed line).  Returns the sites, -10: the file
// cannot be opened, -11: a malformed line, -1: more sites than cap or more text than text_cap
HAPI long long host_sites_parse(const char *path, int32_t n, const char *const *names, int32_t *tid, int32_t *pos, uint64_t cap, uint64_t *lines3, char *text, uint64_t text_cap) {
    SiteFile file;
    std::string error;
    if (text_cap) text[0] = 0;
    if (const int rc = read_sites(path, file, error)) {
        if (text_cap) { strncpy(text, error.c_str(), (size_t)text_cap - 1); text[text_cap - 1] = 0; }
        return -rc;
    }
    ResolvedSites r;
    resolve_sites(file, std::vector<std::string>(names, names + n), r);
    lines3[0] = file.skipped_lines; lines3[1] = r.off_header_lines; lines3[2] = r.duplicate_lines;
    std::string meta;
    for (uint32_t k : r.line) meta += file.lines[k].id + "\t" + file.lines[k].ref + "\t" + file.lines[k].alt + "\n";
    if (r.tid.size() > cap || meta.size() + 1 > text_cap) return -1;
    for (size_t k = 0; k < r.tid.size(); ++k) { tid[k] = r.tid[k]; pos[k] = r.pos[k]; }
    memcpy(text, meta.c_str(), meta.size() + 1);
    return (long long)r.tid.size();
}
// --alleles: <sample>.allele_counts.tsv as the command line writes it, for the site file against n contig names and counts[n_sites][7] (n_sites
// as host_sites_parse returns it).  0; 8 when the file could not be written; 10 / 11 as the reader says
HAPI int host_allele_file(const char *sites_path, int32_t n, const char *const *names, const uint64_t *counts, const char *out_path) {
    SiteFile file;
    std::string error;
    if (const int rc = read_sites(sites_path, file, error)) return rc;
    const std::vector<std::string> contigs(names, names + n);
    ResolvedSites r;
    resolve_sites(file, contigs, r);
    return write_allele_counts(out_path, contigs, file, r, counts) ? 0 : 8;
}
// --alleles: a BAM file through the host reader with set_alleles (pos[n_sites], first[n_contigs + 1]); the shared table and the sums as
// rsqc_alleles_add takes them.  Returns the records read, -1: cannot open, -2: the reader threw
HAPI long long host_bam_alleles(const char *path, int threads, size_t batch_records, int32_t n_contigs, uint32_t n_sites, const int32_t *pos, const uint32_t *first,
                                uint32_t min_mapq, uint32_t min_baseq, uint64_t *counts, rsqc_allele_info *info) {
    try {
        BamReader r;
        if (threads > 0) r.set_threads(threads);
        r.set_alleles(std::vector<int32_t>(pos, pos + n_sites), std::vector<uint32_t>(first, first + n_contigs + 1), min_mapq, min_baseq);
        if (!r.open(path)) return -1;
        long long total = 0;
        for (;;) {
            HostBatch b;
            const size_t k = r.read_batch(b, batch_records ? batch_records : 65536);
            if (!k) break;
            total += (long long)k;
        }
        std::vector<uint64_t> v;
        r.alleles_sum(v, *info);
        if (!v.empty()) memcpy(counts, v.data(), v.size() * 8);
        return total;
    } catch (std::exception &) { return -2; }
}

HAPI unsigned host_library_complexity(double dup, double unique, double limit) { return library_complexity(dup, unique, limit); }

struct BamHandle { BamReader reader; HostBatch batch; rsqc_batch view; std::vector<std::string> names; };
HAPI void *host_bam_read_all(const char *path, const char *ch_tag, const char *const *tags, int n_tags) {
    BamHandle *b = new BamHandle();
    if (!b->reader.open(path)) { delete b; return nullptr; }
    std::vector<std::string> t;
    for (int i = 0; i < n_tags; ++i) t.emplace_back(tags[i]);
    b->reader.set_tags(ch_tag, t);
    try { while (b->reader.read_batch(b->batch, 1u << 20)) {} } catch (...) { delete b; return nullptr; }
    b->view = b->batch.view();
    b->names = b->reader.contigs();
    return b;
}
// same with an explicit decode-thread count and read_batch granularity (the tests sweep both)
HAPI void *host_bam_read_all_ex(const char *path, const char *ch_tag, const char *const *tags, int n_tags, int threads,
                                unsigned long long batch_records) {
    BamHandle *b = new BamHandle();
    b->reader.set_threads(threads);
    if (!b->reader.open(path)) { delete b; return nullptr; }
    std::vector<std::string> t;
    for (int i = 0; i < n_tags; ++i) t.emplace_back(tags[i]);
    b->reader.set_tags(ch_tag, t);
    try { while (b->reader.read_batch(b->batch, (size_t)batch_records)) {} } catch (...) { delete b; return nullptr; }
    b->view = b->batch.view();
    b->names = b->reader.contigs();
    return b;
}
// the records of ONE reference sequence through the BAM index (<path>.bai): BamReader::load_index + seek
HAPI void *host_bam_read_contig(const char *path, const char *ch_tag, const char *const *tags, int n_tags, int threads, int contig) {
    BamHandle *b = new BamHandle();
    b->reader.set_threads(threads);
    if (!b->reader.open(path) || !b->reader.load_index(std::string(path) + ".bai")) { delete b; return nullptr; }
    const auto &idx = b->reader.index();
    if (contig < 0 || (size_t)contig >= idx.size()) { delete b; return nullptr; }
    std::vector<std::string> t;
    for (int i = 0; i < n_tags; ++i) t.emplace_back(tags[i]);
    b->reader.set_tags(ch_tag, t);
    b->names = b->reader.contigs();
    if (idx[(size_t)contig].present) {
        if (!b->reader.seek(idx[(size_t)contig].beg, idx[(size_t)contig].end)) { delete b; return nullptr; }
        uint64_t left = idx[(size_t)contig].n_records;
        try { while (left) { const size_t got = b->reader.read_batch(b->batch, (size_t)std::min<uint64_t>(left, 1u << 20)); if (!got) break; left -= got; } }
        catch (...) { delete b; return nullptr; }
    }
    b->view = b->batch.view();
    return b;
}
HAPI int host_bam_unsorted(void *h) { return ((BamHandle *)h)->batch.unsorted ? 1 : 0; }
HAPI int host_bam_bad_refid_count(void *h) { return (int)((BamHandle *)h)->batch.bad_refid.size(); }
HAPI const char *host_bam_bad_refid(void *h, int i) { return ((BamHandle *)h)->batch.bad_refid[(size_t)i].c_str(); }
HAPI const rsqc_batch *host_bam_batch(void *h) { return &((BamHandle *)h)->view; }
HAPI int host_bam_n_contigs(void *h) { return (int)((BamHandle *)h)->names.size(); }
HAPI const char *host_bam_contig(void *h, int i) { return ((BamHandle *)h)->names[(size_t)i].c_str(); }
HAPI void host_bam_free(void *h) { delete (BamHandle *)h; }

// (the synthetic BAM writer lives in bam_write.cpp)

// ---- the device decode's host side (bgzf_feed.hpp) for the tests: chunks of framed BGZF blocks
namespace { struct FeedHandle { rsqc_host::BgzfFeeder feed; std::string error; }; }
HAPI void *host_feed_open(const char *path) {
    FeedHandle *h = new FeedHandle();
    if (!h->feed.open(path)) { delete h; return nullptr; }
    return h;
}
HAPI unsigned long long host_feed_first_voffset(void *hv) {
    FeedHandle *h = (FeedHandle *)hv;
    try { return h->feed.first_record_voffset(); } catch (std::exception &e) { h->error = e.what(); return ~0ull; }
}
HAPI void host_feed_cpu_share(void *hv, int threads, double initial_share, double max_share) { ((FeedHandle *)hv)->feed.set_cpu_share(threads, initial_share, max_share); }
// page-locks (or, without a device, allocates) the chunk buffers now; max_out != 0: sized for this file's compression, never grown
HAPI int host_feed_reserve(void *hv, unsigned long long chunk_bytes, unsigned long long max_out) {
    FeedHandle *h = (FeedHandle *)hv;
    try { h->feed.reserve((size_t)chunk_bytes, max_out); return 0; }
    catch (std::exception &e) { h->error = e.what(); return -1; }
}
HAPI int host_feed_start(void *hv, unsigned long long voff_beg, unsigned long long voff_end, unsigned long long chunk_bytes, unsigned long long max_out, int read_threads) {
    FeedHandle *h = (FeedHandle *)hv;
    try { h->feed.read_threads = read_threads; h->feed.start(voff_beg, voff_end, (size_t)chunk_bytes, max_out); return 0; }
    catch (std::exception &e) { h->error = e.what(); return -1; }
}
// 1 = a chunk, 0 = end of the range, -1 = error (host_feed_error)
HAPI int host_feed_next(void *hv, const uint8_t **data, unsigned long long *bytes, const rsqc_bgzf_block **blocks, uint32_t *n_blocks,
                        uint32_t *skip, unsigned long long *limit, int *last) {
    FeedHandle *h = (FeedHandle *)hv;
    try {
        rsqc_host::BgzfFeeder::Chunk *c = h->feed.next();
        if (!c) return 0;
        *data = c->data; *bytes = c->total_bytes; *blocks = c->blocks.data(); *n_blocks = (uint32_t)c->blocks.size(); *skip = c->skip; *limit = c->limit; *last = c->last ? 1 : 0;
        return 1;
    } catch (std::exception &e) { h->error = e.what(); return -1; }
}
HAPI const char *host_feed_error(void *hv) { return ((FeedHandle *)hv)->error.c_str(); }
HAPI void host_feed_free(void *hv) { delete (FeedHandle *)hv; }

// the input's format by content (host/sam_feed.cpp: 1 SAM text, 2 BGZF SAM, 3 BAM, -2 plain gzip, -1 unopenable, 0 unknown)
// and, for SAM, its @SQ lines as "name:length,..." in out
HAPI int host_sam_header(const char *path, char *out, int cap) {
    const InputFormat f = sniff_file(path);
    if (cap > 0) out[0] = 0;
    if (f != InputFormat::SamText && f != InputFormat::SamBgzf) return (int)f;
    SamHeader h;
    if (!read_sam_header(path, h)) return -1;
    std::string s;
    for (size_t k = 0; k < h.names.size(); ++k) s += (k ? "," : "") + h.names[k] + ":" + std::to_string(h.lengths[k]);
    if (cap > 0) { strncpy(out, s.c_str(), (size_t)cap - 1); out[cap - 1] = 0; }
    return (int)f;
}
