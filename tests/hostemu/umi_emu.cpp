// umi_emu.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// The two places that interpret a record's bytes -- bam_parse_record (rnaseqc_amd/csrc/rsqc_bamrec.h) and sam_parse_fields
// (rsqc_samrec.h, through sam_parse_line) -- compiled with g++ and called on ONE record / ONE line with a chosen UMI source
// (BamTagSpec.umi_src): every field of BamRecOut comes back, so that a test can compare the umi key with the Python definition and
// every other field between "source selected" and "no source".  The records are copied into a buffer of exactly their size first:
// under the sanitizers of umi_fuzz.cpp a read past the record is a finding.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../rnaseqc_amd/csrc/rsqc_samrec.h"

using namespace rsqc;

#define EMU_API extern "C" __attribute__((visibility("default")))

namespace {
struct Setup {
    BamTagSpec tags{};
    std::vector<SamRefSlot> slots; std::vector<uint8_t> names; SamRefTable refs{};
} g;

void fill(const BamRecOut &o, uint32_t rc, int64_t *out) {
    const int64_t v[18] = {rc, o.tid, o.core.pos, o.core.mpos, o.core.isize, o.aux.flag, o.aux.mapq, o.l_seq, o.nm, o.n_ops, o.aux.tagbits, o.wide, o.qname_len, o.qhash2,
                           (int64_t)(o.aux.qhash & 0xFFFFFFFFull), (int64_t)(o.aux.qhash >> 32), (int64_t)(o.umi & 0xFFFFFFFFull), (int64_t)(o.umi >> 32)};
    memcpy(out, v, sizeof v);
}
}  // namespace

// the tag spec of the calls that follow: chimeric tag "ch", filter tag "XF" (as the writers of rnaseqc_amd/bamio.py name them), the
// @SQ names, and the UMI source: src 0 none, 1 the tag t0 t1, 2 the read name behind its last sep
EMU_API void umiemu_setup(int32_t n_ref, const char *const *names, uint32_t src, uint32_t t0, uint32_t t1, uint32_t sep) {
    g = Setup{};
    g.tags.n_ref = n_ref; g.tags.have_ch = 1; g.tags.ch0 = 'c'; g.tags.ch1 = 'h'; g.tags.n_filter = 1; g.tags.f0[0] = 'X'; g.tags.f1[0] = 'F';
    g.tags.umi_src = (uint8_t)src; g.tags.umi_t0 = (uint8_t)t0; g.tags.umi_t1 = (uint8_t)t1; g.tags.umi_sep = (uint8_t)sep;
    uint32_t slots = 16;
    while (slots < 2u * (uint32_t)n_ref) slots <<= 1;
    g.slots.assign(slots, SamRefSlot{0, 0, 0, -1, 0});
    for (int32_t r = 0; r < n_ref; ++r) {
        const uint32_t len = (uint32_t)strlen(names[r]);
        const uint64_t h = bam_qname_hash((const uint8_t *)names[r], len);
        uint32_t k = (uint32_t)h & (slots - 1);
        while (g.slots[k].idx >= 0) k = (k + 1) & (slots - 1);
        g.slots[k] = SamRefSlot{h, (uint32_t)g.names.size(), len, r, 0};
        g.names.insert(g.names.end(), names[r], names[r] + len);
    }
    g.names.push_back(0);
    g.refs = SamRefTable{g.slots.data(), g.names.data(), slots - 1, n_ref};
}

// out[18] = {code, tid, pos, mpos, isize, flag, mapq, l_seq, nm, n_ops, tagbits, wide, qname_len, qhash2, qhash lo, qhash hi, umi lo, umi hi}
// one BAM record: `bytes` bytes starting with block_size (the record may claim more or less than it has: block_size is what the
// caller of bam_parse_record checked against the window, so it is clamped to the bytes that are there)
EMU_API uint32_t umiemu_bam_record(const uint8_t *rec, uint32_t bytes, int64_t *out) {
    BamRecOut o{};
    if (bytes < 4) { fill(o, 1, out); return 1; }
    std::vector<uint8_t> own(rec, rec + bytes);
    uint32_t bs; memcpy(&bs, own.data(), 4);
    if (bs > bytes - 4) { bs = bytes - 4; memcpy(own.data(), &bs, 4); }
    const bool ok = bam_parse_record(own.data(), bs, g.tags, o);
    fill(o, ok ? 0 : 1, out);
    return ok ? 0 : 1;
}
// one SAM line without its '\n'
EMU_API uint32_t umiemu_sam_line(const uint8_t *s, uint32_t len, int64_t *out) {
    BamRecOut o{};
    std::vector<uint8_t> own(s, s + len);
    std::vector<uint32_t> ops(len / 2 + 1);
    const uint32_t rc = sam_parse_line(own.data(), len, g.tags, g.refs, o, ops.data(), (uint32_t)ops.size());
    fill(o, rc, out);
    return rc;
}
