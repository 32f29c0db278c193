// genemodel_emu.h -- TEST HARNESS ONLY (never loaded by the product): what genebody_emu.cpp and tin_emu.cpp restate alike of the host
// side of the stages over the track (rnaseqc_amd/csrc/rsqc_genemodel_api.cpp), with plain memory.  Include behind wavemu.h.
#pragma once

#include "../../rnaseqc_amd/csrc/rsqc_genemodel.h"

namespace gmemu {

template <class F> void launch(uint32_t grid, uint32_t threads, F &&body) {
    wavemu::grid_dim().x = grid;
    for (uint32_t b = 0; b < grid; ++b) { wavemu::block_idx().x = b; wavemu::run_block(threads, body); }
}

// What a kernel reads beside its plan: the scanned array as rsqc_track_end leaves it (contig t at off[t], one pad slot behind every contig,
// the depth of slot i at i + 1) and the model's columns -- at exactly their size (a read past one is a heap overflow under the sanitizers)
struct Input {
    std::vector<uint64_t> off;
    std::vector<uint32_t> S, seg_start, seg_end;
    std::vector<int32_t> seg_tid;
    rsqc::GeneModel model() const { return rsqc::GeneModel{seg_tid.data(), seg_start.data(), seg_end.data()}; }
};

// depth: the contigs' positions one behind the other (no pads).  Returns the rule the model breaks ("": none, and `in` is filled)
inline std::string lay_out(Input &in, int32_t n_contigs, const uint64_t *length, const uint32_t *depth, int32_t n_genes, const uint32_t *seg_off, const int32_t *seg_tid,
                           const uint32_t *seg_start, const uint32_t *seg_end) {
    in.off.assign((size_t)n_contigs + 1, 0);
    std::vector<uint32_t> len32((size_t)n_contigs + 1, 0);
    for (int32_t t = 0; t < n_contigs; ++t) { len32[(size_t)t] = (uint32_t)length[t]; in.off[(size_t)t + 1] = in.off[(size_t)t] + length[t] + 1; }
    const std::string error = rsqc::genebody_check(n_genes, seg_off, seg_tid, seg_start, seg_end, n_contigs, len32.data());
    if (!error.empty()) return error;
    in.S.assign((size_t)in.off[(size_t)n_contigs] + 1, 0u);          // total + 1 entries
    size_t at = 0;
    for (int32_t t = 0; t < n_contigs; ++t)
        for (uint64_t p = 0; p < length[t]; ++p) in.S[(size_t)(in.off[(size_t)t] + p) + 1] = depth[at++];
    const size_t n_seg = n_genes ? seg_off[n_genes] : 0;
    in.seg_tid.assign(seg_tid, seg_tid + n_seg); in.seg_start.assign(seg_start, seg_start + n_seg); in.seg_end.assign(seg_end, seg_end + n_seg);
    return error;
}

// A case file: four 64-bit words (contigs, genes, segments, schedule seed), the lengths (64-bit each), the depth of every position,
// seg_off, seg_tid, seg_start, seg_end (32-bit each) and, with_reverse, the reverse bytes
struct CaseFile {
    uint64_t seed = 0;
    std::vector<uint64_t> length;
    std::vector<uint32_t> depth, seg_off, seg_start, seg_end;
    std::vector<int32_t> seg_tid;
    std::vector<uint8_t> reverse;
};

// the stand-alone programs' argument and file: 0, or the exit code
inline int read_case(const char *program, int argc, char **argv, bool with_reverse, CaseFile &C) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASEFILE\n", program); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint64_t head[4];
    if (fread(head, 8, 4, f) != 4) return 2;
    const size_t nc = (size_t)head[0], ng = (size_t)head[1], ns = (size_t)head[2];
    C.seed = head[3];
    C.length.resize(nc);
    if (nc && fread(C.length.data(), 8, nc, f) != nc) return 2;
    size_t positions = 0;
    for (uint64_t l : C.length) positions += (size_t)l;
    C.depth.resize(positions); C.seg_off.resize(ng + 1); C.seg_tid.resize(ns); C.seg_start.resize(ns); C.seg_end.resize(ns); C.reverse.resize(with_reverse ? ng : 0);
    if ((positions && fread(C.depth.data(), 4, positions, f) != positions) || fread(C.seg_off.data(), 4, ng + 1, f) != ng + 1 ||
        (ns && (fread(C.seg_tid.data(), 4, ns, f) != ns || fread(C.seg_start.data(), 4, ns, f) != ns || fread(C.seg_end.data(), 4, ns, f) != ns)) ||
        (with_reverse && ng && fread(C.reverse.data(), 1, ng, f) != ng)) { fprintf(stderr, "short case file\n"); return 2; }
    fclose(f);
    return 0;
}

}  // namespace gmemu
