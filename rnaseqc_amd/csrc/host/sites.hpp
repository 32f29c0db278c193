// sites.hpp -- the reader of --alleles=FILE: the body lines of a VCF (plain, gzip or bgzip) as a list of single-base sites, and that list
// resolved against an input's header into the sorted (tid, pos) table rsqc_alleles_begin takes.
#pragma once

#include <stdint.h>
#include <string>
#include <vector>

namespace rsqc_host {

struct SiteLine { std::string chrom; int32_t pos = 0; std::string id, ref, alt; };      // pos 0-based; ALT kept as text
struct SiteFile {
    std::vector<SiteLine> lines;         // the lines kept, in file order
    uint64_t skipped_lines = 0;          // REF is not exactly one of A C G T in either case (indels, symbolic records)
};
// Tab-separated CHROM POS ID REF ALT ...; lines that start with '#' and blank lines are skipped.  0: read; 10: the file cannot be opened;
// 11: a malformed line (fewer than five fields, or a POS that is no integer in 1 .. 2^31 - 1) -- `error` is "<file>:<line>: ..."
int read_sites(const std::string &path, SiteFile &out, std::string &error);

struct ResolvedSites {
    std::vector<int32_t> tid, pos;       // strictly ascending by (tid, pos)
    std::vector<uint32_t> first;         // [n_contigs + 1]: the sites of tid are [first[tid], first[tid + 1])
    std::vector<uint32_t> line;          // per site the index of the line it keeps ID, REF and ALT of (the first of equal position)
    uint64_t off_header_lines = 0, duplicate_lines = 0;
};
// the lines whose contig the header has, sorted by (contig in header order, POS); lines of equal position are merged into one site
void resolve_sites(const SiteFile &file, const std::vector<std::string> &contigs, ResolvedSites &out);

}  // namespace rsqc_host
