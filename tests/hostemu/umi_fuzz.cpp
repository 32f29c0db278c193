// umi_fuzz.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// bam_parse_record and sam_parse_fields (through umi_emu.cpp) on seeded DAMAGED BAM records and SAM lines with each UMI source
// selected, built with -fsanitize=address,undefined.  Every record is parsed from a buffer of exactly its size, so a read past the
// record -- the tag's Z value without its NUL, an aux tail cut in the middle of a field, a name without its NUL, the backward scan
// for the name's separator -- is a finding.  Whatever the bytes are: a record or a refusal, never an access outside; and the
// fields other than the UMI key do not depend on the source.
//
//   umi_fuzz <cases> <seed>      exit 0 = nothing found
#include <cstdio>
#include <cstdlib>
#include <random>

#include "umi_emu.cpp"

namespace {
std::mt19937_64 rng;
uint64_t rnd(uint64_t n) { return n ? rng() % n : 0; }

std::string umi_text() {
    static const char alpha[] = "ACGTACGTACGTacgtN-+";
    std::string u;
    for (int k = rnd(6) ? (int)rnd(14) : (int)rnd(40); k > 0; --k) u += alpha[rnd(sizeof alpha - 1)];
    return u;
}
std::string qname() {
    std::string n;
    for (int k = 1 + (int)(rnd(8) ? rnd(20) : rnd(254)); k > 0; --k) n += (char)('A' + rnd(26));
    if (rnd(3)) { n += rnd(4) ? '_' : ':'; n += umi_text(); }
    if (n.size() > 254) n.resize(254);
    return n;
}
void put32(std::string &s, uint32_t v) { s.append((const char *)&v, 4); }

std::string bam_aux_field() {
    static const char *tagn[] = {"RX", "RX", "NM", "ch", "XF", "MD", "CG"};
    std::string f = tagn[rnd(sizeof tagn / sizeof *tagn)];
    switch (rnd(8)) {
    case 0: case 1: case 2: f += 'Z'; f += umi_text(); f += '\0'; break;
    case 3: f += 'A'; f += (char)('A' + rnd(26)); break;
    case 4: f += 'i'; put32(f, (uint32_t)rnd(1000)); break;
    case 5: { f += 'B'; f += "cCsSiIf"[rnd(7)]; put32(f, (uint32_t)(rnd(8) ? rnd(6) : rnd(1u << 31))); for (int k = (int)rnd(24); k > 0; --k) f += (char)rnd(256); break; }
    case 6: f += 'H'; f += "1AFF"; f += '\0'; break;
    default: f += (char)rnd(256); for (int k = (int)rnd(6); k > 0; --k) f += (char)rnd(256); break;       // an unknown type
    }
    return f;
}
std::string bam_record() {
    const std::string nm = qname();
    const uint32_t l_seq = (uint32_t)rnd(40), n_cig = (uint32_t)rnd(4);
    std::string r;
    put32(r, (uint32_t)((int)rnd(3) - 1)); put32(r, (uint32_t)rnd(100000));
    r += (char)(nm.size() + 1); r += (char)rnd(256); r += (char)0x48; r += (char)0x12;
    r += (char)(n_cig & 0xFF); r += (char)(n_cig >> 8); const uint32_t flag = (uint32_t)rnd(4096); r += (char)(flag & 0xFF); r += (char)(flag >> 8);
    put32(r, l_seq); put32(r, (uint32_t)-1); put32(r, (uint32_t)-1); put32(r, 0);
    r += nm; r += '\0';
    for (uint32_t k = 0; k < n_cig; ++k) put32(r, (uint32_t)((1 + rnd(50)) << 4 | rnd(9)));
    r.append((l_seq + 1) / 2, '\x11'); r.append(l_seq, '\xff');
    for (int k = (int)rnd(6); k > 0; --k) r += bam_aux_field();
    // damage: the tail cut anywhere, bytes flipped towards the structural ones, ranges removed or doubled
    static const char hot[] = "\0RXZAiB_:NM";
    for (int m = rnd(3) ? (int)rnd(5) : 0; m > 0 && !r.empty(); --m) {
        const size_t at = rnd(r.size());
        switch (rnd(6)) {
        case 0: r[at] = hot[rnd(sizeof hot - 1)]; break;
        case 1: r.resize(at); break;
        case 2: r.erase(at, rnd(12)); break;
        case 3: r.insert(at, 1, hot[rnd(sizeof hot - 1)]); break;
        case 4: { const size_t len = std::min<size_t>(rnd(40), r.size() - at); r.insert(at, r.substr(at, len)); break; }
        default: r[at] = (char)rnd(256); break;
        }
    }
    std::string out;
    // block_size: the truth, or (rarely) a lie in either direction -- umiemu_bam_record clamps it to the bytes that are there
    put32(out, rnd(10) ? (uint32_t)r.size() : (uint32_t)(r.size() + rnd(64)) - (uint32_t)rnd(32));
    return out + r;
}
std::string sam_line() {
    std::string l = qname();
    l += "\t" + std::to_string(rnd(4096)) + "\t" + (rnd(4) ? "chrA" : rnd(2) ? "chrB" : "*") + "\t" + std::to_string(rnd(100000)) + "\t" + std::to_string(rnd(256)) + "\t";
    const uint64_t len = 1 + rnd(40);
    l += std::to_string(len) + "M\t*\t0\t0\t" + std::string(len, 'A') + "\t*";
    static const char *typ[] = {"Z", "Z", "Z", "A", "i", "B", "H", "f"};
    static const char *tagn[] = {"RX", "RX", "NM", "ch", "XF"};
    for (int k = (int)rnd(5); k > 0; --k) {
        const char *t = typ[rnd(sizeof typ / sizeof *typ)];
        l += std::string("\t") + tagn[rnd(sizeof tagn / sizeof *tagn)] + ":" + t + ":" + (t[0] == 'i' ? std::to_string(rnd(1000)) : t[0] == 'B' ? std::string("c,1,2") : umi_text());
    }
    static const char hot[] = "\t:RXZ_*0AN-+";
    for (int m = rnd(3) ? (int)rnd(5) : 0; m > 0 && !l.empty(); --m) {
        const size_t at = rnd(l.size());
        switch (rnd(5)) {
        case 0: l[at] = hot[rnd(sizeof hot - 1)]; break;
        case 1: l.resize(at); break;
        case 2: l.erase(at, rnd(12)); break;
        case 3: l.insert(at, 1, hot[rnd(sizeof hot - 1)]); break;
        default: l[at] = (char)(1 + rnd(255)); break;
        }
    }
    return l;
}
bool same_but_umi(const int64_t *a, const int64_t *b) { for (int k = 0; k < 16; ++k) if (a[k] != b[k]) return false; return true; }
}  // namespace

int main(int argc, char **argv) {
    const long cases = argc > 1 ? atol(argv[1]) : 100000;
    rng.seed(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
    static const char *const names[] = {"chrA", "chrB"};
    long keyed = 0, parsed = 0, refused = 0;
    for (long c = 0; c < cases; ++c) {
        const std::string rec = bam_record(), line = sam_line();
        const uint32_t sep = rnd(4) ? (rnd(2) ? '_' : ':') : (uint32_t)(1 + rnd(255));
        int64_t off[2][18], on[18];
        umiemu_setup(2, names, 0, 0, 0, 0);
        const uint32_t rb = umiemu_bam_record((const uint8_t *)rec.data(), (uint32_t)rec.size(), off[0]);
        const uint32_t rs = umiemu_sam_line((const uint8_t *)line.data(), (uint32_t)line.size(), off[1]);
        if ((rb == 0 && (off[0][16] || off[0][17])) || (rs == 0 && (off[1][16] || off[1][17]))) { fprintf(stderr, "case %ld: a key without a source\n", c); return 2; }
        for (uint32_t src = 1; src <= 2; ++src) {
            umiemu_setup(2, names, src, 'R', 'X', sep);
            if (umiemu_bam_record((const uint8_t *)rec.data(), (uint32_t)rec.size(), on) != rb || (rb == 0 && !same_but_umi(on, off[0]))) { fprintf(stderr, "case %ld: the BAM fields depend on the source\n", c); return 3; }
            if (rb == 0) { ++parsed; if (on[16] || on[17]) ++keyed; } else ++refused;
            if (umiemu_sam_line((const uint8_t *)line.data(), (uint32_t)line.size(), on) != rs || (rs == 0 && !same_but_umi(on, off[1]))) { fprintf(stderr, "case %ld: the SAM fields depend on the source\n", c); return 4; }
            if (rs == 0) { ++parsed; if (on[16] || on[17]) ++keyed; } else ++refused;
        }
    }
    printf("%ld cases, %ld parsed, %ld refused, %ld keyed\n", cases, parsed, refused, keyed);
    return 0;
}
