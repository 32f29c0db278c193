// sam_fuzz.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// The device SAM stages' per-lane bodies (rnaseqc_amd/csrc/rsqc_sam.h, rsqc_samrec.h, through sam_emu.cpp's one-lane stream)
// on mutated SAM text, built with -fsanitize=address,undefined.  Every array of the emulation is exactly as large as the C ABI
// makes it (sam_caps / sam_window_rec_cap), so an access outside one here is an access outside a device buffer there.  A
// mutated text must end in a stream of records or in a refused line, never in a crash.  The texts: header lines, records with
// CIGARs of many short operations and '*' SEQ (the most operations per byte a valid line can have), tags of every type, CRLF and
// blank lines; then byte flips towards the structural bytes, insertions, deletions, duplicated ranges and cuts; then cut into
// windows at random places.
//
//   sam_fuzz <cases> <seed>      exit 0 = nothing found
#include <cstdio>
#include <cstdlib>
#include <random>

#include "sam_emu.cpp"

namespace {
std::mt19937_64 rng;
uint64_t rnd(uint64_t n) { return n ? rng() % n : 0; }

std::string record(const char *const *names, int n_ref) {
    std::string l;
    const int q = 1 + (int)rnd(12);
    for (int k = 0; k < q; ++k) l += (char)('A' + rnd(26));
    l += "\t" + std::to_string(rnd(200) ? rnd(4096) : rnd(70000)) + "\t";
    const int t = (int)rnd(n_ref + 2) - 1;
    l += t < 0 ? "*" : t >= n_ref ? "chrZ" : names[t];
    l += "\t" + std::to_string(rnd(5) ? rnd(1000000) : rnd(3)) + "\t" + std::to_string(rnd(200) ? rnd(256) : rnd(300)) + "\t";
    uint64_t qlen = 0;
    const int nops = rnd(6) ? (int)rnd(6) : (int)rnd(3000);
    static const char ops[] = "MIDNSHP=X";
    for (int k = 0; k < nops; ++k) {
        const uint64_t len = rnd(8) ? 1 + rnd(9) : rnd(20000) ? rnd(1u << 20) : rnd(1u << 29);
        const char op = ops[rnd(9)];
        l += std::to_string(len) + op;
        if (op == 'M' || op == 'I' || op == 'S' || op == '=' || op == 'X') qlen += len;
    }
    if (!nops) l += "*";
    l += "\t" + std::string(rnd(2) ? "=" : rnd(2) ? "*" : names[rnd(n_ref)]) + "\t" + std::to_string(rnd(1000)) + "\t" + std::to_string((int64_t)rnd(2000) - 1000) + "\t";
    const bool seq = nops && qlen && qlen < 400 && rnd(3);
    l += seq ? std::string(qlen, 'A') : "*";
    l += "\t" + (seq && rnd(2) ? std::string(qlen, 'I') : std::string("*"));
    static const char *tags[] = {"NM:i:3", "NM:i:-7", "NM:i:300", "NM:f:1.5", "NM:Z:x", "ch:A:1", "ch:Z:yes", "XF:i:1", "XF:B:c,1,2",
                                 "XF:H:1AFF", "XF:f:2", "MD:Z:10A5", "NM:i:4294967295"};
    for (int k = (int)rnd(4); k > 0; --k) l += std::string("\t") + tags[rnd(sizeof tags / sizeof *tags)];
    return l;
}

std::string text_of_case(const char *const *names, int n_ref) {
    std::string t;
    if (rnd(4)) { t += "@HD\tVN:1.6\n"; for (int r = 0; r < n_ref; ++r) t += std::string("@SQ\tSN:") + names[r] + "\tLN:1000000\n"; }
    const int n = 1 + (int)rnd(40);
    const bool crlf = rnd(8) == 0;
    for (int k = 0; k < n; ++k) { t += record(names, n_ref) + (crlf ? "\r\n" : "\n"); if (!rnd(10)) t += "\n"; }
    // mutations
    static const char hot[] = "\t\n\r@*0123456789MIDNSHP=X:AZif-+x ";
    for (int m = rnd(3) ? (int)rnd(6) : 0; m > 0 && !t.empty(); --m) {
        const size_t at = rnd(t.size());
        switch (rnd(6)) {
        case 0: t[at] = hot[rnd(sizeof hot - 1)]; break;
        case 1: t.insert(at, 1, hot[rnd(sizeof hot - 1)]); break;
        case 2: t.erase(at, rnd(20)); break;
        case 3: { const size_t len = std::min<size_t>(rnd(200), t.size() - at); t.insert(at, t.substr(at, len)); break; }
        case 4: t.resize(at); break;
        default: t[at] = (char)rnd(256); break;
        }
    }
    return t;
}
}  // namespace

int main(int argc, char **argv) {
    const long cases = argc > 1 ? atol(argv[1]) : 50000;
    rng.seed(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
    static const char *const names[] = {"chrA", "chrB", "c3"};
    long refused = 0, records = 0;
    for (long c = 0; c < cases; ++c) {
        const int n_ref = 1 + (int)rnd(3);
        BamTagSpec tags{};
        tags.have_ch = 1; tags.ch0 = 'c'; tags.ch1 = 'h'; tags.n_filter = 1; tags.f0[0] = 'X'; tags.f1[0] = 'F';
        const std::string t = text_of_case(names, n_ref);
        emu_sam_begin(n_ref, names, &tags, rnd(3) ? 0 : t.size() + rnd(4096));
        int rc = 0;
        for (size_t a = 0; a < t.size() && !rc;) {
            const size_t len = rnd(3) ? 1 + rnd(t.size() - a) : 1 + rnd(64);
            const size_t l = std::min(len, t.size() - a);
            std::vector<uint8_t> piece(t.begin() + (long)a, t.begin() + (long)(a + l));      // (exactly the call's bytes)
            rc = emu_sam_submit(piece.data(), (uint32_t)l, 1 + (uint32_t)rnd(40));
            a += l;
        }
        if (!rc) rc = emu_sam_end();
        if (rc) ++refused;
        uint64_t cnt[8]; emu_sam_counts(cnt); records += (long)cnt[0];
        // one line on its own, through the host parser the ABI uses to name a refused line
        const size_t nl = t.find('\n');
        std::vector<uint8_t> line(t.begin(), nl == std::string::npos ? t.end() : t.begin() + (long)nl);
        int64_t out[16];
        std::vector<uint32_t> opsv(line.size() / 2 + 1);
        emu_sam_parse_line(line.data(), (uint32_t)line.size(), out, opsv.data(), (uint32_t)opsv.size());
    }
    printf("%ld cases, %ld refused, %ld records\n", cases, refused, records);
    return 0;
}
