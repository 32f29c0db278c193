// report.hpp -- the report tail of the CLI: restates src/RNASeQC.cpp:397-676 and
// operator<<(ofstream&, Metrics&) (src/Metrics.cpp:342-412) on top of rsqc_results.
#pragma once

#include <string>
#include <unordered_map>
#include <vector>

#include "gtf.hpp"

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

}  // namespace rsqc_host
