// gc_fuzz.cpp -- TEST HARNESS ONLY: a stand-alone program (own main, never loaded into Python) that feeds the entry points of gc_emu.cpp
// seeded references and candidate lists, built by tests/test_gc_host.py with the address and undefined-behaviour sanitizers.  The bit
// array, the offsets and every candidate column are heap blocks of exactly the size the product allocates, so a read of gc_count
// outside its contig's words, a shift by 64, or a write behind the bins is a finding.  Contigs of length 0, 1, 63-65 and a few hundred
// bases, some absent from the FASTA; exons and candidate ends on both sides of the contig ends; names with one to four records, now and
// then one name with more records than the LDS sort holds.
//   usage: gc_fuzz <cases> <seed>
#include "gc_emu.cpp"

#include <cstdio>
#include <cstdlib>

namespace {
struct Rng { uint64_t s; uint64_t next() { s += 0x9E3779B97F4A7C15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
             uint32_t below(uint32_t n) { return (uint32_t)((next() >> 32) * (uint64_t)n >> 32); } };
}

int main(int argc, char **argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 100;
    Rng R{argc > 2 ? strtoull(argv[2], nullptr, 10) : 1ull};
    unsigned long long fragments = 0, oversize = 0;
    for (int t = 0; t < cases; ++t) {
        if (t % 3 == 0) wavemu::set_seed(R.next() | 1ull); else wavemu::set_seed(0);
        const int nc = 1 + (int)R.below(5);
        static const uint32_t kLen[] = {0, 1, 63, 64, 65, 127, 128, 129};
        std::vector<uint64_t> L((size_t)nc);
        std::vector<int32_t> g_contig, g_start, g_end, e_contig, e_start, e_end;
        std::vector<uint8_t> g_flags, e_flags, globin;
        std::vector<uint32_t> g_id, e_id, e_gene, ge_off{0}, ge_row;
        for (int k = 0; k < nc; ++k) {
            L[(size_t)k] = R.below(3) ? 1 + R.below(700) : kLen[R.below(8)];
            if (R.below(4) == 0) continue;                                             // a contig without features
            const int ne = 1 + (int)R.below(4);
            int32_t at = 1 + (int32_t)R.below(40);
            const int32_t first = at;
            for (int j = 0; j < ne; ++j) {
                const int32_t len = 1 + (int32_t)R.below(1 + (uint32_t)L[(size_t)k] / 2 + 40);
                e_contig.push_back(k); e_start.push_back(at); e_end.push_back(at + len - 1); e_flags.push_back(0);
                e_id.push_back((uint32_t)e_id.size()); e_gene.push_back((uint32_t)g_id.size()); ge_row.push_back((uint32_t)ge_row.size());
                at += len + 1 + (int32_t)R.below(30);
            }
            g_contig.push_back(k); g_start.push_back(first); g_end.push_back(e_end.back()); g_flags.push_back(0); g_id.push_back((uint32_t)g_id.size());
            globin.push_back(0); ge_off.push_back((uint32_t)ge_row.size());
        }
        rsqc_annotation a{};
        a.n_ref = a.n_contigs = nc; a.n_genes = a.n_genes_listed = (int32_t)g_id.size(); a.n_exons = (int32_t)e_id.size();
        a.gene_row_contig = g_contig.data(); a.gene_row_start = g_start.data(); a.gene_row_end = g_end.data(); a.gene_row_flags = g_flags.data(); a.gene_row_id = g_id.data();
        a.exon_row_contig = e_contig.data(); a.exon_row_start = e_start.data(); a.exon_row_end = e_end.data(); a.exon_row_flags = e_flags.data();
        a.exon_row_id = e_id.data(); a.exon_row_gene = e_gene.data(); a.gene_is_globin = globin.data(); a.gene_exon_off = ge_off.data(); a.gene_exon_row = ge_row.data();
        // the FASTA: a shuffled subset of the contigs, random bytes with G g C c frequent
        std::vector<int32_t> r_contig; std::vector<uint64_t> r_len; std::vector<std::vector<uint8_t>> seqs; std::vector<const uint8_t *> r_seq;
        std::vector<int> order((size_t)nc);
        for (int k = 0; k < nc; ++k) order[(size_t)k] = k;
        for (int k = nc; k > 1; --k) std::swap(order[(size_t)k - 1], order[R.below((uint32_t)k)]);
        for (int k : order) {
            if (nc > 1 && R.below(4) == 0) continue;
            std::vector<uint8_t> s((size_t)L[(size_t)k]);
            for (auto &ch : s) ch = R.below(3) ? (uint8_t)"GgCcAaTtNS"[R.below(10)] : (uint8_t)R.below(256);
            r_contig.push_back(k); r_len.push_back(L[(size_t)k]); seqs.push_back(std::move(s));
        }
        for (auto &s : seqs) r_seq.push_back(s.empty() ? (const uint8_t *)"" : s.data());
        rsqc_reference ref{(int32_t)r_contig.size(), r_contig.data(), r_len.data(), r_seq.data()};
        const uint64_t words = gcemu_reference_words(&ref);
        std::vector<unsigned long long> w_out((size_t)words + 1), w_off((size_t)nc), w_len((size_t)nc);
        std::vector<double> exon_gc((size_t)a.n_exons + 1, -9.0);
        int rc = gcemu_reference(&a, &ref, w_out.data(), w_off.data(), w_len.data(), exon_gc.data());
        if (rc) { fprintf(stderr, "case %d: gcemu_reference rc %d\n", t, rc); return 1; }
        for (int e = 0; e < a.n_exons; ++e)
            if (!(exon_gc[(size_t)e] == -1.0 || (exon_gc[(size_t)e] >= 0.0 && exon_gc[(size_t)e] <= 1.0000001))) { fprintf(stderr, "case %d: exon_gc[%d] = %g\n", t, e, exon_gc[(size_t)e]); return 1; }
        // candidates on the contigs the FASTA names (the candidates kernel lets no other through)
        if (r_contig.empty()) continue;
        const uint32_t n_names = 1 + R.below(600);
        const bool hot = R.below(8) == 0;
        std::vector<uint64_t> file, q; std::vector<uint32_t> h2, row, fl; std::vector<int32_t> end, tid;
        auto add = [&](uint64_t name_q, uint32_t name_h) {
            const int k = r_contig[R.below((uint32_t)r_contig.size())];
            const int64_t len = (int64_t)L[(size_t)k];
            file.push_back(0); q.push_back(name_q); h2.push_back(name_h); row.push_back(R.below(3)); tid.push_back(k);
            end.push_back((int32_t)((int64_t)R.below((uint32_t)len + 250) - 50));
            fl.push_back(R.below(300) | (R.below(5) ? 0x80000000u : 0u));
        };
        for (uint32_t i = 0; i < n_names; ++i) {
            const uint64_t nq = i % 97 == 0 ? ~0ull : R.next(); const uint32_t nh = i % 89 == 0 ? 0xFFFFFFFFu : (uint32_t)R.next();
            const int k = 1 + (int)R.below(R.below(6) == 0 ? 4 : 2);
            for (int j = 0; j < k; ++j) add(nq, nh);
        }
        if (hot) { const uint64_t nq = R.next(); const uint32_t nh = (uint32_t)R.next(); for (int j = 0; j < 2100 + (int)R.below(900); ++j) add(nq, nh); }
        const uint32_t n = (uint32_t)file.size();
        std::vector<uint32_t> perm(n);
        for (uint32_t i = 0; i < n; ++i) perm[i] = i;
        for (uint32_t i = n; i > 1; --i) std::swap(perm[i - 1], perm[R.below(i)]);
        for (uint32_t i = 0; i < n; ++i) file[perm[i]] = 1000 + 2ull * i;
        std::vector<unsigned long long> bins((size_t)RSQC_GC_BINS + 1);
        uint64_t stats[6];
        rc = gcemu_run(nullptr, &a, nullptr, 0, n, file.data(), q.data(), h2.data(), row.data(), end.data(), fl.data(), tid.data(), bins.data(), stats);
        if (rc || stats[4]) { fprintf(stderr, "case %d: gcemu_run rc %d error %lld\n", t, rc, (long long)stats[4]); return 1; }
        unsigned long long total = 0;
        for (auto b : bins) total += b;
        if (total > n / 2 || (hot != (stats[3] > 0))) { fprintf(stderr, "case %d: %llu fragments of %u candidates, %llu listed buckets\n", t, total, n, (unsigned long long)stats[3]); return 1; }
        fragments += total; oversize += stats[3];
    }
    printf("gc_fuzz: %d cases, %llu fragments, %llu oversize buckets\n", cases, fragments, oversize);
    return 0;
}
