// report.hpp -- the report tail of the CLI: restates src/RNASeQC.cpp:397-676 and
// operator<<(ofstream&, Metrics&) (src/Metrics.cpp:342-412) on top of rsqc_results.
#pragma once

#include <string>
#include <unordered_map>
#include <vector>

#include "gtf.hpp"
#include "sites.hpp"

namespace rsqc_host {

struct ReportConfig {
    std::string output_dir, sample_name;     // SAMPLENAME (src/RNASeQC.cpp:99)
    bool sample_given = false;               // --sample given: GCT value column is the sample name
    bool use_rpkm = false, write_coverage = false;
    unsigned detection_threshold = 5;
    std::vector<std::string> filter_tags;    // names for "Filtered by tag: X"
};

// quirky computeMedian (src/Metrics.h:147-160) on an ordered sequence; throws std::range_error when empty
double compute_median(const std::vector<double> &sorted);
// getStatistics (src/Metrics.h:166-186): avg, median, std, MAD (sorts its argument)
void get_statistics(std::vector<double> &data, double &avg, double &med, double &sd, double &mad);
// Lander-Waterman search of src/RNASeQC.cpp:398-415 without the 1e9-step loop (same result)
unsigned library_complexity(double duplicates, double unique, double limit = 1e9);

// Writes every output file.  contig_visit_order: boundary contig ids in the order the BAM visited them
// (coverage.tsv row order).  Throws std::range_error exactly where the reference does.
void write_reports(const ReportConfig &cfg, Annotation &ann, const rsqc_results &r,
                   const std::vector<int> &contig_visit_order);

// --junctions: which junctions the annotation knows.  Per chromosome (chromosomeMap id) two hash sets built once from the GTF's exon
// rows: exon end -> the genes with an exon that ends there, exon start -> the genes with an exon that starts there.  A junction
// (start, end: the intron's first and last base, 1-based closed) is known when ONE gene has, on that chromosome, an exon whose end
// is start - 1 and an exon whose start is end + 1.
struct JunctionIndex {
    bool built = false;
    std::vector<std::unordered_map<long long, std::vector<uint32_t>>> ends, starts;       // [chromosomeMap id]
    void build(const Annotation &ann);
    bool known(int chrom, long long start, long long end) const;
};
// <output>/<sample>.junctions.tsv: contig (the input header's name), start, end, reads, hq_reads, max_overhang, known -- one line per
// row of the table, in table order.  `ann` is flattened for the input's header (contig_names, chrom_of_contig).
void write_junctions(const std::string &path, const Annotation &ann, const JunctionIndex &index, const rsqc_junction_table &table);

// --gene-body: the model handed to rsqc_genebody_begin, built once per input header.  For every listed gene: its exon rows
// (gene_exon_off / gene_exon_row of the flattened annotation) on the contig of the gene's first exon row, if the header has that
// contig; 1-based closed -> 0-based half-open, clipped to [0, LN), overlapping and abutting rows merged; reverse: that first row's
// strand is RSQC_STRAND_REVERSE.  (Rows parked under --legacy sit on a contig no header has.)
struct GeneBodyModel {
    std::vector<uint32_t> seg_off, seg_start, seg_end, gene_len;
    std::vector<int32_t> seg_tid;
    std::vector<uint8_t> reverse;
    void build(const Annotation &ann, const std::vector<uint64_t> &contig_lengths);
};
// the file's three columns from the sums ([n_genes][RSQC_GENEBODY_BINS]): depth_sum over the measured genes (L >= 100); eligible
// genes (L >= 100 and total depth >= L); norm_mean: the mean over the eligible genes, in gene order, of
// (sum[g][k] / len_k) / (total_g / L) with len_k = ceil((k + 1) L / 100) - ceil(k L / 100), in doubles; 0 without an eligible gene
struct GeneBodyProfile { uint64_t eligible = 0; uint64_t depth_sum[RSQC_GENEBODY_BINS] = {}; double norm_mean[RSQC_GENEBODY_BINS] = {}; };
GeneBodyProfile gene_body_profile(const GeneBodyModel &model, const uint64_t *sums);
// <output>/<sample>.gene_body.tsv: bin, depth_sum, genes, norm_mean -- 100 rows, bin 0 = the 5' end.  False: the file could not be written
bool write_gene_body(const std::string &path, const GeneBodyProfile &profile);

// --tin: the file's floating columns and the summary from the rows of rsqc_tin_rows (one per gene of the GeneBodyModel, whose
// gene_len is L).  mean_depth = S / L (0 for L = 0).  A gene is eligible when L >= 100 and S >= L; for it, in doubles,
// H = ln(S) - E ln(2) / S and tin = 100 exp(H) / L; every other gene has tin 0.  The summary covers the eligible genes' tin: mean
// (summed in gene order), median (of the sorted values; the mean of the two middle ones for an even count) and the population
// standard deviation; all three 0 without an eligible gene
struct TinProfile {
    std::vector<double> mean_depth, tin;
    std::vector<uint8_t> is_eligible;
    uint64_t eligible = 0;
    double mean = 0, median = 0, stdev = 0;
};
TinProfile tin_profile(const uint32_t *gene_len, size_t n_genes, const rsqc_tin_row *rows);
// <output>/<sample>.tin.tsv: gene_id, length, covered, depth_sum, max_depth, mean_depth, tin -- one row per listed gene, in the order
// and with the ids of gene_reads.gct.  False: the file could not be written
bool write_tin(const std::string &path, const std::vector<std::string> &gene_ids, const uint32_t *gene_len, const rsqc_tin_row *rows, const TinProfile &profile);
// <output>/<sample>.tin_summary.tsv: genes, eligible, mean, median, stdev -- one row
bool write_tin_summary(const std::string &path, const TinProfile &profile);

// --cycles: the two tables of rsqc_cycles_end, base[2][512][5] and qual[2][512][64].  For end 1 then 2, one row per cycle 1..R, R the
// highest cycle of that end with a base (a single-end run has no rows of end 2).
// <output>/<sample>.cycle_bases.tsv: end, cycle, A, C, G, T, N, total
bool write_cycle_bases(const std::string &path, const uint64_t *base);
// <output>/<sample>.cycle_quality.tsv: end, cycle, bases (n: the qualities of the cycle), mean (sum of q qual / n in doubles, %.6f), q25, median,
// q75 (quantile k: the smallest q with 4 cum(q) >= k n); all four 0 for n = 0
bool write_cycle_quality(const std::string &path, const uint64_t *base, const uint64_t *qual);

// --mismatches: the three tables of rsqc_mismatch_end, cyc[2][512][6], subst[2][4][4] and byq[64][2].
// <output>/<sample>.mismatch_cycles.tsv: end, cycle, compared, mismatches, uncompared, inserted, clipped, deletions, mismatch_rate (mismatches /
// compared in doubles, %.6f, 0 for compared = 0); for end 1 then 2, one row per cycle 1..R, R the highest cycle of that end with a non-zero column
bool write_mismatch_cycles(const std::string &path, const uint64_t *cyc);
// <output>/<sample>.mismatch_types.tsv: end, ref, read, count; 16 rows (ref then read in A C G T order) per end that has a compared base
bool write_mismatch_types(const std::string &path, const uint64_t *subst);
// <output>/<sample>.mismatch_quality.tsv: quality, compared, mismatches, mismatch_rate; one row per quality 0..63 with compared > 0
bool write_mismatch_quality(const std::string &path, const uint64_t *byq);

// --alleles: the table of rsqc_alleles_end, counts[n_sites][7], with the sites it was counted for.
// <output>/<sample>.allele_counts.tsv: contig, position (1-based), id, ref, alt, A, C, G, T, other, deleted, low_baseq, ref_count (the column of
// REF) and alt_count (the sum of the columns of the distinct single-base A C G T entries of ALT's comma list that differ from REF; 0 when
// there is none); one row per site in table order
bool write_allele_counts(const std::string &path, const std::vector<std::string> &contigs, const SiteFile &file, const ResolvedSites &sites, const uint64_t *counts);

}  // namespace rsqc_host
