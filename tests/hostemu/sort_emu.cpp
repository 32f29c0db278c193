// sort_emu.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// The KERNELS of --sort -- rnaseqc_amd/csrc/rsqc_sort.h (key build, key reduction, per-tile digit histogram, scan, ballot-ranked
// scatter, gather into output batches), unmodified -- compiled for the host on top of the 64-lane fiber emulation of wavemu.h and
// run against std::stable_sort.  The host side of rsqc_sort_api.cpp (which digit positions run, the ping-pong of the passes, the
// batch loop of the gather) is restated here with plain memory.
#include "wavemu.h"

#include <algorithm>
#include <numeric>
#include <vector>

#include "../../rnaseqc_amd/csrc/rsqc_sort.h"

using namespace rsqc;

namespace {
struct Rng { uint64_t s; uint64_t next() { s += 0x9E3779B97F4A7C15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
             uint32_t below(uint32_t n) { return (uint32_t)((next() >> 32) * (uint64_t)n >> 32); } };
template <class F> void launch(uint32_t grid, F &&body) {
    wavemu::grid_dim().x = grid;
    for (uint32_t b = 0; b < grid; ++b) { wavemu::block_idx().x = b; wavemu::run_block(RSQC_SORT_THREADS, body); }
}
uint32_t blocks_for(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

void emu_scan(uint32_t *data, uint64_t m, std::vector<unsigned long long> &chunk_sum, unsigned long long *total) {
    const uint32_t chunks = blocks_for(m, RSQC_SCAN_CHUNK);
    chunk_sum.assign((size_t)chunks + 1, 0xDEADull);
    if (chunks) launch(chunks, [&]() { sort_scan_sum_kernel(data, m, chunk_sum.data()); });
    launch(1, [&]() { sort_scan_top_kernel(chunk_sum.data(), chunks, total); });
    if (chunks) launch(chunks, [&]() { sort_scan_apply_kernel(data, m, chunk_sum.data()); });
}

// keys in place -> sorted keys; idx = the permutation.  prep_grid: workgroups of the key reduction.  Returns the passes run (-1: in order already)
int emu_sort(std::vector<uint64_t> &key, std::vector<uint32_t> &idx, uint32_t prep_grid, uint64_t *or_and) {
    const uint64_t n = key.size();
    idx.assign((size_t)n + 1, 0xFFFFFFFFu);
    if (!n) { idx.resize(0); return -1; }
    prep_grid = std::min<uint32_t>(prep_grid, blocks_for(n, RSQC_SORT_THREADS));
    std::vector<unsigned long long> part((size_t)prep_grid * 3, 0);
    launch(prep_grid, [&]() { sort_prepare_kernel(key.data(), n, idx.data(), part.data()); });
    uint64_t o = 0, a = ~0ull; bool disorder = false;
    for (uint32_t k = 0; k < prep_grid; ++k) { o |= part[3 * k]; a &= part[3 * k + 1]; disorder = disorder || part[3 * k + 2]; }
    if (or_and) { or_and[0] = o; or_and[1] = a; }
    idx.resize((size_t)n);
    if (!disorder) return -1;
    int shift[8];
    const int n_pass = sort_live_digits(o, a, shift);
    const uint32_t tiles = blocks_for(n, RSQC_SORT_TILE);
    std::vector<uint64_t> key1((size_t)n, 0); std::vector<uint32_t> idx1((size_t)n, 0), hist((size_t)256 * tiles, 0);
    std::vector<unsigned long long> chunk_sum; unsigned long long total = 0;
    uint64_t *kb[2] = {key.data(), key1.data()}; uint32_t *ib[2] = {idx.data(), idx1.data()};
    int cur = 0;
    for (int p = 0; p < n_pass; ++p) {
        const int sh = shift[p];
        launch(tiles, [&]() { sort_hist_kernel(kb[cur], n, sh, hist.data(), tiles); });
        emu_scan(hist.data(), (uint64_t)256 * tiles, chunk_sum, &total);
        if (total != n) return -100;
        launch(tiles, [&]() { sort_scatter_kernel(kb[cur], ib[cur], kb[cur ^ 1], ib[cur ^ 1], n, sh, hist.data(), tiles); });
        cur ^= 1;
    }
    if (cur) { key = key1; idx = idx1; }
    return n_pass;
}
}  // namespace

extern "C" __attribute__((visibility("default"))) void sortemu_set_schedule_seed(unsigned long long seed) { wavemu::set_seed(seed); }

// the radix sort alone: perm_out[r] = input index of rank r; stats[0] = passes run (-1 as 2^64 - 1: input in order), [1] OR, [2] AND of the keys.
// Returns 0 when the permutation equals std::stable_sort's and the keys come out in order, 1000 + k for check k
extern "C" __attribute__((visibility("default")))
int sortemu_sort(const uint64_t *keys, uint64_t n, uint32_t prep_grid, uint32_t *perm_out, uint64_t *stats) {
    std::vector<uint64_t> key(keys, keys + n);
    std::vector<uint32_t> idx;
    uint64_t oa[2] = {0, 0};
    const int passes = emu_sort(key, idx, prep_grid, oa);
    if (passes == -100) return 1001;                                     // a histogram that does not add up to n
    stats[0] = (uint64_t)(int64_t)passes; stats[1] = oa[0]; stats[2] = oa[1];
    std::vector<uint32_t> want((size_t)n);
    std::iota(want.begin(), want.end(), 0u);
    std::stable_sort(want.begin(), want.end(), [&](uint32_t x, uint32_t y) { return keys[x] < keys[y]; });
    for (uint64_t r = 0; r < n; ++r) {
        perm_out[r] = idx[(size_t)r];
        if (idx[(size_t)r] != want[(size_t)r]) return 1002;
        if (key[(size_t)r] != keys[want[(size_t)r]]) return 1003;
    }
    return 0;
}

// the keys sort_append_kernel builds for one batch (tid from the segment table, pos from the records)
extern "C" __attribute__((visibility("default")))
int sortemu_keys(const int32_t *pos, uint64_t n, const int32_t *seg_tid, const uint64_t *seg_start, uint32_t n_seg, uint64_t *key_out) {
    std::vector<rsqc_rec_core> core((size_t)n + 1, rsqc_rec_core{0, 0, 0, 0});
    for (uint64_t i = 0; i < n; ++i) core[(size_t)i].pos = pos[i];
    if (n) launch(blocks_for(n, RSQC_SORT_THREADS), [&]() { sort_append_kernel(core.data(), n, seg_tid, seg_start, n_seg, key_out, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr); });
    return 0;
}

// the whole way: `n` records in `n_in` input batches of unequal sizes (random contigs incl. -1 and one beyond n_ref, positions incl. -1,
// 0-5 operations per record, some records with escape values and wide entries, one of them with 300 operations), collected with
// sort_append_kernel, sorted, and gathered into output batches of `out_batch` records.  Every output batch is compared with the
// stably sorted input: record halves, cigar_off and operations, segment table, wide table, qhash2.  0 = equal, 2000 + k for check k
extern "C" __attribute__((visibility("default")))
int sortemu_gather(uint64_t seed, uint32_t n, uint32_t n_in, uint32_t out_batch, int in_order, uint64_t *stats /*[3]: output batches, moved, passes*/) {
    Rng R{seed};
    struct Rec { int32_t tid; rsqc_rec_core c; rsqc_rec_aux a; uint32_t h2; std::vector<uint32_t> ops; int32_t nm, lq; bool wide; };
    std::vector<Rec> recs((size_t)n);
    const int32_t tids[6] = {0, 1, 2, 7, -1, 1};
    for (uint32_t i = 0; i < n; ++i) {
        Rec &r = recs[(size_t)i];
        r.tid = tids[R.below(6)];
        r.c = rsqc_rec_core{R.below(50) == 0 ? -1 : (int32_t)R.below(3000), (int32_t)R.below(3000), (int32_t)R.below(500), 0u};
        uint32_t k = R.below(6);
        if (i == n / 3) k = 300;
        for (uint32_t j = 0; j < k; ++j) r.ops.push_back(((1u + R.below(90)) << 4) | R.below(4));
        r.nm = R.below(40) == 0 ? 255 + (int32_t)R.below(100) : (int32_t)R.below(8);
        r.lq = R.below(60) == 0 ? 70000 : 76;
        r.wide = k >= 255 || r.nm >= 255 || r.lq >= 65535;
        r.a = rsqc_rec_aux{R.next(), (uint16_t)R.below(4096), (uint16_t)(r.lq >= 65535 ? 0xFFFF : r.lq), (uint8_t)R.below(256), (uint8_t)(r.nm >= 255 ? 0xFF : r.nm), (uint8_t)R.below(8), (uint8_t)(k >= 255 ? 0xFF : k)};
        r.h2 = (uint32_t)R.next();
    }
    auto key_of = [&](const Rec &r) { return sort_key(r.tid, r.c.pos); };
    if (in_order) std::stable_sort(recs.begin(), recs.end(), [&](const Rec &x, const Rec &y) { return key_of(x) < key_of(y); });
    // ---- collect: input batches with their own pools, segment tables and wide tables
    std::vector<rsqc_rec_core> c_core; std::vector<rsqc_rec_aux> c_aux; std::vector<uint32_t> c_h2, c_cigar, c_wnc; std::vector<uint64_t> c_key((size_t)n + 1, 0), c_wi, rec0, pool0;
    std::vector<int32_t> c_wnm, c_wlq;
    uint32_t at = 0;
    for (uint32_t b = 0; b < n_in && at < n; ++b) {
        const uint32_t left = n - at, m = b + 1 == n_in ? left : std::min(left, 1u + R.below(2 * n / n_in + 1));
        std::vector<rsqc_rec_core> core; std::vector<int32_t> seg_tid, wnm, wlq; std::vector<uint64_t> seg_start, wi; std::vector<uint32_t> pool, wnc;
        for (uint32_t i = 0; i < m; ++i) {
            const Rec &r = recs[(size_t)(at + i)];
            if (i == 0 || r.tid != recs[(size_t)(at + i - 1)].tid) { seg_tid.push_back(r.tid); seg_start.push_back(i); }
            rsqc_rec_core c = r.c; c.cigar_off = (uint32_t)pool.size();
            core.push_back(c); c_core.push_back(c); c_aux.push_back(r.a); c_h2.push_back(r.h2);
            pool.insert(pool.end(), r.ops.begin(), r.ops.end());
            if (r.wide) { wi.push_back(i); wnm.push_back(r.nm); wlq.push_back(r.lq); wnc.push_back((uint32_t)r.ops.size()); }
        }
        seg_start.push_back(m);
        rec0.push_back(at); pool0.push_back(c_cigar.size());
        const size_t w0 = c_wi.size();
        c_wi.resize(w0 + wi.size() + 1); c_wnm.resize(w0 + wi.size() + 1); c_wlq.resize(w0 + wi.size() + 1); c_wnc.resize(w0 + wi.size() + 1);
        wi.push_back(0); wnm.push_back(0); wlq.push_back(0); wnc.push_back(0);
        const uint32_t nw = (uint32_t)wi.size() - 1;
        launch(blocks_for(std::max(m, nw), RSQC_SORT_THREADS), [&]() {
            sort_append_kernel(core.data(), m, seg_tid.data(), seg_start.data(), (uint32_t)seg_tid.size(), c_key.data() + at, at, wi.data(), wnm.data(), wlq.data(), wnc.data(), nw,
                               c_wi.data() + w0, c_wnm.data() + w0, c_wlq.data() + w0, c_wnc.data() + w0);
        });
        c_wi.resize(w0 + nw); c_wnm.resize(w0 + nw); c_wlq.resize(w0 + nw); c_wnc.resize(w0 + nw);
        c_cigar.insert(c_cigar.end(), pool.begin(), pool.end());
        at += m;
    }
    c_key.resize((size_t)n);
    for (uint32_t i = 0; i < n; ++i) if (c_key[(size_t)i] != key_of(recs[(size_t)i])) return 2001;
    // ---- sort
    std::vector<uint64_t> key = c_key; std::vector<uint32_t> idx;
    const int passes = emu_sort(key, idx, 3, nullptr);
    if (passes == -100) return 2002;
    if (in_order && passes != -1) return 2003;
    std::vector<uint32_t> want((size_t)n);
    std::iota(want.begin(), want.end(), 0u);
    std::stable_sort(want.begin(), want.end(), [&](uint32_t x, uint32_t y) { return c_key[x] < c_key[y]; });
    if (idx != want) return 2004;
    // ---- gather
    std::vector<uint64_t> tab(rec0); tab.push_back(n); const size_t nb = rec0.size(); tab.insert(tab.end(), pool0.begin(), pool0.end());
    c_wi.push_back(~0ull); c_wnm.push_back(0); c_wlq.push_back(0); c_wnc.push_back(0); c_cigar.push_back(0);
    SortCollection C{c_core.data(), c_aux.data(), c_h2.data(), c_cigar.data(), tab.data(), tab.data() + nb + 1, (uint32_t)nb, c_wi.data(), c_wnm.data(), c_wlq.data(), c_wnc.data(), c_wi.size() - 1, c_cigar.size() - 1};
    uint64_t moved = 0, batches = 0;
    std::vector<unsigned long long> chunk_sum;
    for (uint32_t r0 = 0; r0 < n; r0 += out_batch) {
        const uint32_t m = std::min(out_batch, n - r0), blocks = blocks_for(m, RSQC_SORT_THREADS);
        std::vector<uint32_t> n_ops((size_t)m + 1, 0xAAAAAAAAu), seg_mark((size_t)m + 1, 0xAAAAAAAAu), wide_mark((size_t)m + 1, 0xAAAAAAAAu), moved_part(blocks, 0);
        launch(blocks, [&]() { sort_gather_count_kernel(C, key.data(), idx.data(), r0, m, n_ops.data(), seg_mark.data(), wide_mark.data(), moved_part.data()); });
        unsigned long long tot[3] = {0, 0, 0};
        emu_scan(n_ops.data(), m, chunk_sum, &tot[0]); emu_scan(seg_mark.data(), m, chunk_sum, &tot[1]); emu_scan(wide_mark.data(), m, chunk_sum, &tot[2]);
        if (n_ops[(size_t)m] != 0xAAAAAAAAu || seg_mark[(size_t)m] != 0xAAAAAAAAu) return 2005;       // a write past the batch
        for (uint32_t k = 0; k < blocks; ++k) moved += moved_part[k];
        std::vector<rsqc_rec_core> o_core((size_t)m); std::vector<rsqc_rec_aux> o_aux((size_t)m); std::vector<uint32_t> o_h2((size_t)m), o_cig((size_t)tot[0] + 1, 0xBBBBBBBBu), o_wnc((size_t)tot[2] + 1);
        std::vector<int32_t> o_seg_tid((size_t)tot[1] + 1), o_wnm((size_t)tot[2] + 1), o_wlq((size_t)tot[2] + 1); std::vector<uint64_t> o_seg_start((size_t)tot[1] + 2, ~0ull), o_wi((size_t)tot[2] + 1);
        SortOutput O{o_core.data(), o_aux.data(), o_h2.data(), o_cig.data(), o_seg_tid.data(), o_seg_start.data(), o_wi.data(), o_wnm.data(), o_wlq.data(), o_wnc.data()};
        launch(blocks, [&]() { sort_gather_kernel(C, key.data(), idx.data(), r0, m, n_ops.data(), seg_mark.data(), wide_mark.data(), (uint32_t)tot[0], (uint32_t)tot[1], O); });
        // the batch as a reader of rsqc_batch sees it, against the sorted records
        if (o_cig[(size_t)tot[0]] != 0xBBBBBBBBu) return 2006;
        uint32_t seg = 0, wide = 0, pool_at = 0;
        if (o_seg_start[(size_t)tot[1]] != m) return 2007;
        for (uint32_t j = 0; j < m; ++j) {
            const Rec &r = recs[(size_t)want[(size_t)(r0 + j)]];
            if (j == 0 || r.tid != recs[(size_t)want[(size_t)(r0 + j - 1)]].tid) {
                if (seg >= tot[1] || o_seg_tid[seg] != r.tid || o_seg_start[seg] != j) return 2008;
                ++seg;
            }
            const rsqc_rec_core &c = o_core[(size_t)j];
            if (c.pos != r.c.pos || c.mpos != r.c.mpos || c.isize != r.c.isize || c.cigar_off != pool_at) return 2009;
            if (memcmp(&o_aux[(size_t)j], &r.a, sizeof(rsqc_rec_aux)) || o_h2[(size_t)j] != r.h2) return 2010;
            for (size_t k = 0; k < r.ops.size(); ++k) if (o_cig[(size_t)pool_at + k] != r.ops[k]) return 2011;
            pool_at += (uint32_t)r.ops.size();
            if (r.wide) {
                if (wide >= tot[2] || o_wi[wide] != j || o_wnm[wide] != r.nm || o_wlq[wide] != r.lq || o_wnc[wide] != r.ops.size()) return 2012;
                ++wide;
            }
        }
        if (seg != tot[1] || wide != tot[2] || pool_at != tot[0]) return 2013;
        ++batches;
    }
    uint64_t want_moved = 0;
    for (uint32_t r = 0; r < n; ++r) want_moved += want[(size_t)r] != r;
    if (moved != want_moved) return 2014;
    stats[0] = batches; stats[1] = moved; stats[2] = (uint64_t)(int64_t)passes;
    return 0;
}
