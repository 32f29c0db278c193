// k5_emu.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// The fragment-size KERNELS -- rnaseqc_amd/csrc/rsqc_k5.h (partition by name hash, per-bucket LDS sort + replay of the
// reference's state machine, radix select of the first N samples by file index, size histogram + compaction), unmodified --
// compiled for the host on top of the 64-lane fiber emulation of wavemu.h and run on seeded candidates against a literal
// std::map walk in file order (src/Expression.cpp:509-538 with the --fragment-samples cut-off of src/RNASeQC.cpp:372-376).
// The host side of rsqc_fragsize.hip (launch order, the digit loop of the selection) is restated here with plain memory; the bucket count
// and the grids are the library's own plan (rsqc_k5_plan.h).
//
// k5emu_run: seeded candidates against a std::map walk inside this file.  k5emu_run_cands: candidate columns given by the caller
// (tests/k5_cases.py), everything the stages leave behind exported -- offsets, listed buckets, the path each bucket took, raw and kept
// samples, the select's state, the size table's top, the sizes beyond it, the (size, count) pairs, the error word.  k5emu_partition: the
// three partition kernels alone.  With -DK5EMU_MAIN the file is a stand-alone program over a case file (for a sanitizer build).
#include "wavemu.h"

#include <algorithm>
#include <map>
#include <vector>

#include "../../rnaseqc_amd/csrc/rsqc_read.h"
#include "../../rnaseqc_amd/csrc/rsqc_device.h"
#include "../../rnaseqc_amd/csrc/rsqc_k5_plan.h"
#include "../../rnaseqc_amd/csrc/rsqc_k5.h"

using namespace rsqc;

namespace {
struct Rng { uint64_t s; uint64_t next() { s += 0x9E3779B97F4A7C15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
             uint32_t below(uint32_t n) { return (uint32_t)((next() >> 32) * (uint64_t)n >> 32); } };
template <class F> void launch(uint32_t grid, int threads, F &&body) {
    wavemu::grid_dim().x = grid;
    for (uint32_t b = 0; b < grid; ++b) { wavemu::block_idx().x = b; wavemu::run_block(threads, body); }
}
}  // namespace

// n_names names with 1-4 candidate records each (BED interval, end position, flags and sizes at random, a few sizes beyond the
// direct table), emitted in a shuffled order like K1's atomic slots.  Returns 0 when samples kept, their (size, count) pairs and
// the kept (file index, size) set equal the literal walk; 1000 + k for check k; -code for a device error.
extern "C" __attribute__((visibility("default")))
int k5emu_run(uint64_t seed, int n_names, uint32_t max_samples, int hot /* records of ONE extra name: a bucket beyond the LDS sort; -1: a file as sequencers write
                 them -- one or two candidates per name -- plus, one name in 997, a DIFFERENT name crafted to share the 64-bit mix of the pairing set (rsqc_k5.h,
                 pair_bucket_hashed) with an earlier one */, uint64_t *stats /*[7]: candidates, samples, kept, distinct sizes, listed buckets, buckets paired through the set, buckets sorted*/) {
    Rng R{seed};
    const bool pairs_only = hot < 0; if (pairs_only) hot = 0;
    g_k5_hashed_buckets = 0; g_k5_sorted_buckets = 0;
    struct Cand { uint64_t file, q; uint32_t h2; int32_t name, endpos; uint32_t flag_size; };
    std::vector<Cand> cands;
    uint64_t file = 1000;
    for (int i = 0; i < n_names; ++i) {
        uint64_t q = R.next();
        if (i % 311 == 0) q = ~0ull;                                  // (the padding key of the LDS sort, as a real name)
        uint32_t h2 = (uint32_t)R.next();
        if (pairs_only) {
            if (i % 997 == 996 && !cands.empty()) {        // another name on an earlier name's mix: q' ^ h2' K = q ^ h2 K (the set must hand the bucket to the sort)
                const Cand &o = cands[R.below((uint32_t)cands.size())];
                // (... AND its bucket: the buckets are cut on the high bits of q, so the two mixes' difference must leave them alone)
                uint64_t d = 0;
                do { h2 = (uint32_t)R.next(); d = ((uint64_t)o.h2 * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)h2 * 0x9E3779B97F4A7C15ull); } while (h2 == o.h2 || (d >> 50) != 0);
                q = o.q ^ d;
            }
            const int k2 = 1 + (int)R.below(2);
            const int32_t iv2 = (int32_t)R.below(50);
            for (int j = 0; j < k2; ++j) {
                Cand c;
                c.q = q; c.h2 = h2; c.name = R.below(5) == 0 ? iv2 + 1 : iv2; c.endpos = 1000 + (int32_t)R.below(400);
                c.flag_size = (80u + R.below(700)) | (R.below(4) ? 0x80000000u : 0u);
                c.file = 0; cands.push_back(c);
            }
            continue;
        }
        if (i % 313 == 0 && !cands.empty()) { const Cand &o = cands[R.below((uint32_t)cands.size())]; q = o.q; h2 = o.h2; }   // a name that comes back much later
        if (i % 47 == 0 && !cands.empty()) { q = cands[R.below((uint32_t)cands.size())].q; h2 = (uint32_t)R.next() | 1u; }  // ANOTHER name with the same 64-bit hash (differs in the second hash)
        const int k = 1 + (int)R.below(R.below(8) == 0 ? 4 : 2);
        const int32_t iv = (int32_t)R.below(50);
        for (int j = 0; j < k; ++j) {
            Cand c;
            c.q = q; c.h2 = h2; c.name = R.below(5) == 0 ? iv + 1 : iv; c.endpos = 1000 + (int32_t)R.below(400);
            const uint32_t size = R.below(97) == 0 ? (1u << 20) + R.below(5000) * 1000u : 80u + R.below(700);
            c.flag_size = size | (R.below(4) ? 0x80000000u : 0u);
            c.file = 0; cands.push_back(c);
        }
    }
    if (hot > 0) {                                                    // one name with `hot` records (stripped / constant read names): all in one bucket
        const uint64_t q = R.next(); const uint32_t h2 = (uint32_t)R.next();
        for (int j = 0; j < hot; ++j) {
            Cand c; c.q = q; c.h2 = h2; c.name = (int32_t)R.below(3); c.endpos = 1000 + (int32_t)R.below(400);
            c.flag_size = (80u + R.below(700)) | (R.below(4) ? 0x80000000u : 0u); c.file = 0; cands.push_back(c);
        }
    }
    // file order = a shuffle of the candidates (mates of a name end up a random distance apart); indices are unique and sparse
    for (size_t i = cands.size(); i > 1; --i) std::swap(cands[i - 1], cands[R.below((uint32_t)i)]);
    for (auto &c : cands) { file += 1 + R.below(3); c.file = file; }
    // the literal walk, file order
    std::map<std::pair<uint64_t, uint32_t>, std::pair<int32_t, int32_t>> open_names;          // a name = (64-bit hash, second hash)
    std::vector<std::pair<uint64_t, uint32_t>> want_samples;
    for (const Cand &c : cands) {
        auto it = open_names.find({c.q, c.h2});
        if (it == open_names.end()) open_names[{c.q, c.h2}] = {c.name, c.endpos};
        else if (it->second.first == c.name) {
            if (!(c.flag_size >> 31) || c.endpos <= it->second.second) continue;
            want_samples.push_back({c.file, c.flag_size & 0x7FFFFFFFu});
            open_names.erase(it);
        }
    }
    const uint32_t want_keep = (uint32_t)std::min<size_t>(want_samples.size(), max_samples);
    std::sort(want_samples.begin(), want_samples.end());
    std::map<int64_t, uint64_t> want_hist;
    for (uint32_t i = 0; i < want_keep; ++i) want_hist[(int64_t)want_samples[i].second]++;
    // emission order differs from file order
    for (size_t i = cands.size(); i > 1; --i) std::swap(cands[i - 1], cands[R.below((uint32_t)i)]);
    const uint32_t n = (uint32_t)cands.size();
    std::vector<uint64_t> c_file(n), c_q(n); std::vector<int32_t> c_name(n), c_end(n); std::vector<uint32_t> c_fs(n), c_h2(n);
    for (uint32_t i = 0; i < n; ++i) { c_file[i] = cands[i].file; c_q[i] = cands[i].q; c_name[i] = cands[i].name; c_end[i] = cands[i].endpos; c_fs[i] = cands[i].flag_size; c_h2[i] = cands[i].h2; }
    FragCandidates fc{c_file.data(), c_q.data(), c_name.data(), c_end.data(), c_fs.data(), nullptr, n, nullptr, c_h2.data()};

    int error = 0;
    const K5Plan plan = k5_plan(n, max_samples);
    const uint32_t nb = plan.n_buckets;
    std::vector<uint32_t> count(nb + 1, 0u), off(nb + 1, 0xDEADu), cursor(nb + 1, 0xDEADu), perm(n, 0xFFFFFFFFu), big_list(PB_BIG_MAX + 1, 0u), big_idx(2 * (size_t)n + 16, 0xDEADu);
    const uint32_t G = plan.part_grid;
    launch(G, 256, [&]() { pair_bucket_count_kernel(c_q.data(), n, nb, count.data()); });
    launch(1, 1024, [&]() { pair_bucket_scan_kernel(count.data(), nb, off.data(), cursor.data(), big_list.data(), &error); });
    launch(G, 256, [&]() { pair_bucket_scatter_kernel(c_q.data(), n, nb, cursor.data(), perm.data()); });
    if (error) return -error;
    if (off[nb] != n) return 1001;
    std::vector<uint64_t> s_file(n + 1), k_file(n + 1); std::vector<uint32_t> s_size(n + 1), k_size(n + 1);
    uint32_t ns = 0;
    launch(nb, PB_THREADS, [&]() { frag_replay_kernel(fc, off.data(), perm.data(), s_file.data(), s_size.data(), &ns); });
    launch(plan.big_grid, 1024, [&]() { frag_replay_big_kernel(fc, off.data(), perm.data(), big_list.data(), big_idx.data(), s_file.data(), s_size.data(), &ns); });
    if ((hot > (int)PB_CAP) != (big_list[0] > 0)) return 1007;
    if (ns != want_samples.size()) return 1002;
    const uint32_t keep = std::min(ns, max_samples);
    uint32_t n_kept = 0;
    {   // the select as rsqc_fragsize.hip runs it: planned and decided on the "device", no counters read back in between
        uint64_t state[2] = {~0ull, ~0ull};
        std::vector<uint32_t> h(256, 0u);
        launch(1, 64, [&]() { sample_plan_kernel(&ns, max_samples, state); });
        for (int shift = 56; shift >= 0; shift -= 8) {
            launch(plan.select_grid, 256, [&]() { sample_digit_hist_kernel(s_file.data(), &ns, shift, state, h.data()); });
            launch(1, 256, [&]() { sample_digit_pick_kernel(h.data(), shift, state); });
        }
        launch(plan.keep_grid, 1024, [&]() { sample_keep_kernel(s_file.data(), s_size.data(), &ns, state, k_file.data(), k_size.data(), &n_kept); });
        if (n_kept != keep) return 1003;
    }
    {
        std::vector<std::pair<uint64_t, uint32_t>> got(n_kept);
        for (uint32_t i = 0; i < n_kept; ++i) got[i] = {k_file[i], k_size[i]};
        std::sort(got.begin(), got.end());
        for (uint32_t i = 0; i < n_kept; ++i) if (got[i] != want_samples[i]) return 1004;
    }
    std::vector<uint32_t> table(SIZE_TABLE, 0u), out_size(SIZE_TABLE), out_count(SIZE_TABLE), big(n + 1);
    uint32_t n_big = 0, n_out = 0xDEADu, top = 0;
    launch(plan.size_grid, 256, [&]() { size_hist_kernel(k_size.data(), &n_kept, table.data(), big.data(), &n_big, &top); });
    launch(1, 1024, [&]() { size_hist_compact_kernel(table.data(), &top, out_size.data(), out_count.data(), &n_out); });
    std::vector<std::pair<int64_t, uint64_t>> got_hist;
    for (uint32_t i = 0; i < n_out; ++i) got_hist.push_back({(int64_t)out_size[i], (uint64_t)out_count[i]});
    std::sort(big.begin(), big.begin() + n_big);
    for (uint32_t i = 0; i < n_big;) { uint32_t j = i + 1; while (j < n_big && big[j] == big[i]) ++j; got_hist.push_back({(int64_t)big[i], (uint64_t)(j - i)}); i = j; }
    if (got_hist.size() != want_hist.size()) return 1005;
    size_t at = 0;
    for (auto &kv : want_hist) { if (got_hist[at].first != kv.first || got_hist[at].second != kv.second) return 1006; ++at; }
    stats[0] = n; stats[1] = ns; stats[2] = n_kept; stats[3] = got_hist.size(); stats[4] = big_list[0]; stats[5] = g_k5_hashed_buckets; stats[6] = g_k5_sorted_buckets;
    return 0;
}

// ---- candidate columns given by the caller -------------------------------------------------------------------------------------------
// Every array is a heap block of the size the stage needs (never more than the library allocates: rsqc_fragsize.hip, grow_scratch) plus
// ONE guard entry that must still hold its poison afterwards: 1100 + k names the array whose guard was written.
namespace {
constexpr uint32_t kGuard32 = 0xA5C3A5C3u;
constexpr uint64_t kGuard64 = 0xA5C3A5C3A5C3A5C3ull;
struct K5Out {
    uint32_t n = 0, nb = 0, ns = 0, n_kept = 0, top = 0, n_beyond = 0, n_table = 0, big0 = 0;
    int error = 0;
    uint64_t state[2] = {0, 0};
    std::vector<uint32_t> count, off, big_list, perm, raw_size, kept_size, beyond, pair_size, pair_count;
    std::vector<unsigned char> path;                  // per bucket: 0 empty, 1 the set, 2 the LDS sort, 3 listed
    std::vector<uint64_t> raw_file, kept_file;
};
K5Out g_out;

// count / scan / scatter as partition_by_name launches them; 0, or 1100 + k
int k5_partition(const uint64_t *q, uint32_t n, K5Out &o, std::vector<uint32_t> &big_list /*[PB_BIG_MAX + 2]*/) {
    const uint32_t nb = k5_bucket_count(n), G = k5_part_grid(n);
    o.n = n; o.nb = nb;
    // (count / off / cursor: guard entries up to the last bucket a scan thread could reach without its clamp, so that such a walk is a
    //  failed check here, not a stray heap write)
    const size_t room = (size_t)((nb + 1023u) / 1024u) * 1024u + 2u;
    std::vector<uint32_t> count(room, kGuard32), off(room, kGuard32), cursor(room, kGuard32), perm((size_t)n + 1, kGuard32);
    for (uint32_t b = 0; b <= nb; ++b) count[b] = 0u;                      // (the library clears nb + 1 counters)
    big_list.assign(PB_BIG_MAX + 2, kGuard32); big_list[0] = 0u;
    launch(G, K5_PART_THREADS, [&]() { pair_bucket_count_kernel(q, n, nb, count.data()); });
    launch(1, 1024, [&]() { pair_bucket_scan_kernel(count.data(), nb, off.data(), cursor.data(), big_list.data(), &o.error); });
    launch(G, K5_PART_THREADS, [&]() { pair_bucket_scatter_kernel(q, n, nb, cursor.data(), perm.data()); });
    if (count[nb] != 0u) return 1101;
    for (size_t k = nb + 1; k < room; ++k) if (count[k] != kGuard32 || off[k] != kGuard32) return 1102;
    for (size_t k = nb; k < room; ++k) if (cursor[k] != kGuard32) return 1103;   // (the scan writes cursors of buckets only)
    if (perm[n] != kGuard32) return 1104;
    if (big_list[PB_BIG_MAX + 1] != kGuard32) return 1105;
    for (uint32_t b = 0; b < nb; ++b) if (cursor[b] != off[b + 1]) return 1106;  // every bucket filled to its end
    o.big0 = big_list[0];
    count.resize(nb); off.resize(nb + 1); perm.resize(n);
    o.count = count; o.off = off; o.perm = perm;
    const uint32_t listed = std::min(big_list[0], PB_BIG_MAX);
    o.big_list.assign(big_list.begin() + 1, big_list.begin() + 1 + listed);
    return 0;
}

int k5_run_columns(const uint64_t *file, const uint64_t *q, const uint32_t *h2, const int32_t *name, const int32_t *endpos, const uint32_t *fs,
                   uint32_t n, uint32_t max_samples, K5Out &o) {
    o = K5Out{};
    g_k5_hashed_buckets = 0; g_k5_sorted_buckets = 0;
    if (n == 0) return 0;                                                  // (run_fragment_sizes)
    std::vector<uint32_t> big_list;
    if (const int rc = k5_partition(q, n, o, big_list)) return rc;
    const K5Plan plan = k5_plan(n, max_samples);
    const uint32_t nb = plan.n_buckets, cap = plan.ns_bound;
    FragCandidates fc{(uint64_t *)file, (uint64_t *)q, (int32_t *)name, (int32_t *)endpos, (uint32_t *)fs, nullptr, n, nullptr, (uint32_t *)h2};
    std::vector<uint64_t> s_file((size_t)cap + 1, kGuard64), k_file((size_t)cap + 1, kGuard64);
    std::vector<uint32_t> s_size((size_t)cap + 1, kGuard32), k_size((size_t)cap + 1, kGuard32), big_idx(2 * (size_t)n + 1, kGuard32);
    o.path.assign(nb + 1, 0); o.path[nb] = 0xEE;
    g_k5_bucket_path = o.path.data();
    uint32_t ns = 0;
    launch(nb, PB_THREADS, [&]() { frag_replay_kernel(fc, o.off.data(), o.perm.data(), s_file.data(), s_size.data(), &ns); });
    g_k5_bucket_path = nullptr;
    launch(plan.big_grid, 1024, [&]() { frag_replay_big_kernel(fc, o.off.data(), o.perm.data(), big_list.data(), big_idx.data(), s_file.data(), s_size.data(), &ns); });
    if (o.path[nb] != 0xEE) return 1107;
    o.path.resize(nb);
    for (uint32_t b : o.big_list) { if (b >= nb || o.path[b] != 2) return 1108; o.path[b] = 3; }     // (a listed bucket is beyond the set: the LDS sort declines it)
    if (s_file[cap] != kGuard64 || s_size[cap] != kGuard32) return 1109;
    if (big_idx[2 * (size_t)n] != kGuard32) return 1110;
    if (ns > cap) return 1111;
    o.ns = ns;
    o.raw_file.assign(s_file.begin(), s_file.begin() + ns); o.raw_size.assign(s_size.begin(), s_size.begin() + ns);
    if (max_samples == 0) return 0;                                        // (run_fragment_sizes: nothing to keep)
    uint32_t n_kept = 0;
    std::vector<uint32_t> h(257, 0u); h[256] = kGuard32;
    o.state[0] = ~0ull; o.state[1] = ~0ull;
    launch(1, 64, [&]() { sample_plan_kernel(&ns, max_samples, o.state); });
    for (int shift = 56; shift >= 0; shift -= 8) {
        launch(plan.select_grid, 256, [&]() { sample_digit_hist_kernel(s_file.data(), &ns, shift, o.state, h.data()); });
        launch(1, 256, [&]() { sample_digit_pick_kernel(h.data(), shift, o.state); });
    }
    launch(plan.keep_grid, 1024, [&]() { sample_keep_kernel(s_file.data(), s_size.data(), &ns, o.state, k_file.data(), k_size.data(), &n_kept); });
    if (h[256] != kGuard32) return 1112;
    if (k_file[cap] != kGuard64 || k_size[cap] != kGuard32) return 1113;
    std::vector<uint32_t> table((size_t)SIZE_TABLE + 1, 0u), out_size((size_t)SIZE_TABLE + 1, kGuard32), out_count((size_t)SIZE_TABLE + 1, kGuard32), beyond((size_t)n + 1, kGuard32);
    table[SIZE_TABLE] = kGuard32;
    uint32_t n_beyond = 0, n_out = kGuard32, top = 0;
    launch(plan.size_grid, 256, [&]() { size_hist_kernel(k_size.data(), &n_kept, table.data(), beyond.data(), &n_beyond, &top); });
    launch(1, 1024, [&]() { size_hist_compact_kernel(table.data(), &top, out_size.data(), out_count.data(), &n_out); });
    if (table[SIZE_TABLE] != kGuard32 || out_size[SIZE_TABLE] != kGuard32 || out_count[SIZE_TABLE] != kGuard32 || beyond[n] != kGuard32) return 1114;
    // the host's read-back (run_fragment_sizes): no samples, nothing; the selection keeps exactly min(samples, max_samples)
    if (!ns) return 0;
    if (n_kept != std::min(ns, max_samples)) return 1115;
    if (n_out > SIZE_TABLE || n_beyond > n) return 1116;
    o.n_kept = n_kept; o.top = top; o.n_beyond = n_beyond; o.n_table = n_out;
    o.kept_file.assign(k_file.begin(), k_file.begin() + n_kept); o.kept_size.assign(k_size.begin(), k_size.begin() + n_kept);
    o.pair_size.assign(out_size.begin(), out_size.begin() + n_out); o.pair_count.assign(out_count.begin(), out_count.begin() + n_out);
    o.beyond.assign(beyond.begin(), beyond.begin() + n_beyond);
    std::sort(o.beyond.begin(), o.beyond.end());                           // sizes of 2^20 and more: all behind the table's
    for (uint32_t i = 0; i < n_beyond;) { uint32_t j = i + 1; while (j < n_beyond && o.beyond[j] == o.beyond[i]) ++j; o.pair_size.push_back(o.beyond[i]); o.pair_count.push_back(j - i); i = j; }
    return 0;
}
}  // namespace

// seed: wavemu.h's seeded schedule (0: round-robin) -- the order of the set's atomicCAS decides which member of a slot is 0 and which 1.
// Returns 0, or 1100 + k for a failed internal check; the results stay in this library until the next call (k5emu_info / k5emu_fetch).
extern "C" __attribute__((visibility("default")))
int k5emu_run_cands(const uint64_t *file, const uint64_t *q, const uint32_t *h2, const int32_t *name, const int32_t *endpos, const uint32_t *flag_size,
                    uint32_t n, uint32_t max_samples, uint64_t seed) {
    wavemu::set_seed(seed);
    const int rc = k5_run_columns(file, q, h2, name, endpos, flag_size, n, max_samples, g_out);
    wavemu::set_seed(0);
    return rc;
}
// the three partition kernels alone (the bucket counts whose replay would take the emulation minutes)
extern "C" __attribute__((visibility("default")))
int k5emu_partition(const uint64_t *q, uint32_t n, uint64_t seed) {
    wavemu::set_seed(seed);
    g_out = K5Out{};
    std::vector<uint32_t> big_list;
    const int rc = n ? k5_partition(q, n, g_out, big_list) : 0;
    wavemu::set_seed(0);
    return rc;
}
// [0] candidates [1] buckets [2] samples [3] kept [4] top [5] sizes beyond the table [6] (size, count) pairs, merged [7] error word
// [8] big[0] as the scan left it [9] [10] the select's state (prefix = last kept file index, rank still wanted) [11] pairs from the table
extern "C" __attribute__((visibility("default")))
void k5emu_info(uint64_t *out) {
    const K5Out &o = g_out;
    const uint64_t v[12] = {o.n, o.nb, o.ns, o.n_kept, o.top, o.n_beyond, o.pair_size.size(), (uint64_t)(int64_t)o.error, o.big0, o.state[0], o.state[1], o.n_table};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
}
// 0 count[nb] 1 off[nb + 1] 2 listed buckets 3 path[nb] (bytes) 4 / 5 raw samples' file index (64-bit) / size 6 / 7 kept 8 sizes beyond the table,
// ascending 9 / 10 the pairs' size / count 11 perm[n]
extern "C" __attribute__((visibility("default")))
void k5emu_fetch(int what, void *dst) {
    const K5Out &o = g_out;
    auto put = [&](const void *p, size_t bytes) { if (bytes) memcpy(dst, p, bytes); };
    switch (what) {
    case 0: put(o.count.data(), o.count.size() * 4); break;
    case 1: put(o.off.data(), o.off.size() * 4); break;
    case 2: put(o.big_list.data(), o.big_list.size() * 4); break;
    case 3: put(o.path.data(), o.path.size()); break;
    case 4: put(o.raw_file.data(), o.raw_file.size() * 8); break;
    case 5: put(o.raw_size.data(), o.raw_size.size() * 4); break;
    case 6: put(o.kept_file.data(), o.kept_file.size() * 8); break;
    case 7: put(o.kept_size.data(), o.kept_size.size() * 4); break;
    case 8: put(o.beyond.data(), o.beyond.size() * 4); break;
    case 9: put(o.pair_size.data(), o.pair_size.size() * 4); break;
    case 10: put(o.pair_count.data(), o.pair_count.size() * 4); break;
    case 11: put(o.perm.data(), o.perm.size() * 4); break;
    default: break;
    }
}

#if defined(K5EMU_MAIN)
// k5_emu CASEFILE: four 64-bit words (candidates, max_samples, schedule seed, 1 = the partition kernels alone), then the columns file index,
// name hash (64-bit each), second hash, BED row, end position, flag_size (32-bit each).  Prints what the stages left and exits 0, or 1 with
// the failed check.  Built with sanitizers by tests/test_k5_edges_host.py: __shared__ is static storage here, so a store one entry past
// an LDS array is a global-buffer-overflow.
int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: k5_emu CASEFILE\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint64_t head[4];
    if (fread(head, 8, 4, f) != 4) return 2;
    const uint32_t n = (uint32_t)head[0];
    std::vector<uint64_t> file(n), q(n); std::vector<uint32_t> h2(n), fs(n); std::vector<int32_t> name(n), endpos(n);
    if (n && (fread(file.data(), 8, n, f) != n || fread(q.data(), 8, n, f) != n || fread(h2.data(), 4, n, f) != n || fread(name.data(), 4, n, f) != n ||
              fread(endpos.data(), 4, n, f) != n || fread(fs.data(), 4, n, f) != n)) { fprintf(stderr, "short case file\n"); return 2; }
    fclose(f);
    const int rc = head[3] ? k5emu_partition(q.data(), n, head[2]) : k5emu_run_cands(file.data(), q.data(), h2.data(), name.data(), endpos.data(), fs.data(), n, (uint32_t)head[1], head[2]);
    uint64_t v[12];
    k5emu_info(v);
    printf("k5_emu: rc=%d n=%llu buckets=%llu samples=%llu kept=%llu top=%llu beyond=%llu pairs=%llu error=%lld listed=%llu\n", rc, (unsigned long long)v[0], (unsigned long long)v[1],
           (unsigned long long)v[2], (unsigned long long)v[3], (unsigned long long)v[4], (unsigned long long)v[5], (unsigned long long)v[6], (long long)v[7], (unsigned long long)v[8]);
    return rc ? 1 : 0;
}
#endif
