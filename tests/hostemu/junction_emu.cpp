// junction_emu.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// The KERNELS of --junctions -- rnaseqc_amd/csrc/rsqc_junction.h (extract, widen, permute, head marks, segmented reduce) and the
// radix pass and scan of rnaseqc_amd/csrc/rsqc_sort.h they are ordered with, unmodified -- compiled for the host on top of the 64-lane
// fiber emulation of wavemu.h.  The host side of rsqc_junction_api.cpp (the growth of the collection to the host's bound, which digit
// positions run, the two stages and their ping-pong, the row count) is restated here with plain memory.  The expected table is NOT
// computed here: tests/junction_ref.py restates the contract in Python and the test compares.
#include "wavemu.h"

#include <algorithm>
#include <vector>

#include "../../rnaseqc_amd/csrc/rsqc_sort.h"
#include "../../rnaseqc_amd/csrc/rsqc_junction.h"

using namespace rsqc;

namespace {
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
// one stable pass (launch_sort_pass): false when the histogram does not add up
bool emu_pass(const uint64_t *kin, const uint32_t *iin, uint64_t *kout, uint32_t *iout, uint64_t n, int sh, std::vector<uint32_t> &hist, std::vector<unsigned long long> &chunk_sum) {
    const uint32_t tiles = blocks_for(n, RSQC_SORT_TILE);
    hist.assign((size_t)256 * tiles, 0);
    unsigned long long total = 0;
    launch(tiles, [&]() { sort_hist_kernel(kin, n, sh, hist.data(), tiles); });
    emu_scan(hist.data(), (uint64_t)256 * tiles, chunk_sum, &total);
    if (total != n) return false;
    launch(tiles, [&]() { sort_scatter_kernel(kin, iin, kout, iout, n, sh, hist.data(), tiles); });
    return true;
}

constexpr uint64_t kGuard64 = 0xA5A5A5A5A5A5A5A5ull;
constexpr uint32_t kGuard32 = 0xA5A5A5A5u;
struct State {
    uint64_t cap = 0, cap0 = 0, bound = 0, grown = 0;
    int32_t n_contigs = 0; uint32_t mapq_threshold = 0;
    std::vector<uint64_t> key_hi; std::vector<uint32_t> end, info;       // cap entries + one guard each
    unsigned long long cursor[2] = {0, 0};
    int error = 0;
    std::vector<int32_t> tid, start, end_h; std::vector<uint32_t> reads, hq, ov;
} S;
}  // namespace

#define EMU_API extern "C" __attribute__((visibility("default")))

EMU_API void juncemu_set_schedule_seed(unsigned long long seed) { wavemu::set_seed(seed); }

EMU_API void juncemu_begin(uint64_t cap0, int32_t n_contigs, uint32_t mapq_threshold) {
    S = State{};
    S.cap0 = cap0; S.n_contigs = n_contigs; S.mapq_threshold = mapq_threshold;
}

// one batch: the growth step of junction_extract (rsqc_junction_api.cpp), then the kernel.  Returns 1 when a guard word was written
EMU_API int juncemu_add_batch(const rsqc_rec_core *core, const rsqc_rec_aux *aux, uint64_t n, const uint32_t *cigar, uint64_t n_ops,
                              const int32_t *seg_tid, const uint64_t *seg_start, uint32_t n_seg, const uint64_t *wide_index, const uint32_t *wide_n_cigar, uint32_t n_wide) {
    S.bound += n_ops / 2;
    const uint64_t need = std::max(S.bound, S.cap0);
    if (need > S.cap || S.key_hi.empty()) {
        const uint64_t ncap = std::max(need, 2 * S.cap);
        S.key_hi.resize((size_t)S.cap); S.end.resize((size_t)S.cap); S.info.resize((size_t)S.cap);       // (drop the guards)
        S.key_hi.resize((size_t)ncap + 1, kGuard64); S.end.resize((size_t)ncap + 1, kGuard32); S.info.resize((size_t)ncap + 1, kGuard32);
        S.key_hi[(size_t)ncap] = kGuard64; S.end[(size_t)ncap] = kGuard32; S.info[(size_t)ncap] = kGuard32;
        S.cap = ncap; S.grown += 1;
    }
    if (!n) return 0;
    JunctionBatch B{core, aux, cigar, n, n_ops, seg_tid, seg_start, n_seg, wide_index, wide_n_cigar, n_wide};
    JunctionCollection C{S.key_hi.data(), S.end.data(), S.info.data(), S.cap, S.cursor};
    launch(blocks_for(n, RSQC_JUNC_THREADS), [&]() { junction_extract_kernel(B, S.n_contigs, S.mapq_threshold, C, &S.error); });
    return (S.key_hi[(size_t)S.cap] != kGuard64 || S.end[(size_t)S.cap] != kGuard32 || S.info[(size_t)S.cap] != kGuard32) ? 1 : 0;
}

// order and reduce.  stats: [0] rows, [1] instances, [2] contributing records, [3] the error flag, [4] passes of stage 1, [5] of stage 2,
// [6] growth steps, [7] capacity.  Returns 0, or 3000 + k for check k of the harness itself
EMU_API int juncemu_end(uint64_t *stats) {
    const uint64_t N = S.cursor[0];
    stats[0] = 0; stats[1] = N; stats[2] = S.cursor[1]; stats[3] = (uint64_t)(int64_t)S.error; stats[4] = stats[5] = 0; stats[6] = S.grown; stats[7] = S.cap;
    S.tid.clear(); S.start.clear(); S.end_h.clear(); S.reads.clear(); S.hq.clear(); S.ov.clear();
    if (S.error || N > S.cap) { stats[3] = (uint64_t)(int64_t)RSQC_ERR_CAPACITY; return 0; }
    if (!N) return 0;
    const uint32_t prep_grid = std::min<uint32_t>(3, blocks_for(N, RSQC_SORT_THREADS));
    std::vector<uint64_t> kb[2] = {std::vector<uint64_t>((size_t)N + 1, kGuard64), std::vector<uint64_t>((size_t)N + 1, kGuard64)};
    std::vector<uint32_t> ib[2] = {std::vector<uint32_t>((size_t)N + 1, kGuard32), std::vector<uint32_t>((size_t)N + 1, kGuard32)};
    std::vector<unsigned long long> part((size_t)prep_grid * 6, 0), chunk_sum;
    std::vector<uint32_t> hist;
    launch(blocks_for(N, RSQC_JUNC_THREADS), [&]() { junction_widen_kernel(S.end.data(), N, kb[0].data()); });
    launch(prep_grid, [&]() { sort_prepare_kernel(S.key_hi.data(), N, ib[1].data(), part.data() + (size_t)prep_grid * 3); });
    launch(prep_grid, [&]() { sort_prepare_kernel(kb[0].data(), N, ib[0].data(), part.data()); });
    uint64_t oa[2][2] = {{0, ~0ull}, {0, ~0ull}};
    for (int h = 0; h < 2; ++h)
        for (uint32_t k = 0; k < prep_grid; ++k) { oa[h][0] |= part[(size_t)h * prep_grid * 3 + 3 * k]; oa[h][1] &= part[(size_t)h * prep_grid * 3 + 3 * k + 1]; }
    int shift[8], kc = 0, ic = 0;
    const int n_end = sort_live_digits(oa[0][0], oa[0][1], shift);
    for (int p = 0; p < n_end; ++p) {
        if (!emu_pass(kb[kc].data(), ib[ic].data(), kb[kc ^ 1].data(), ib[ic ^ 1].data(), N, shift[p], hist, chunk_sum)) return 3001;
        kc ^= 1; ic ^= 1;
    }
    kc ^= 1;
    launch(blocks_for(N, RSQC_JUNC_THREADS), [&]() { junction_permute_kernel(S.key_hi.data(), ib[ic].data(), N, kb[kc].data()); });
    const int n_hi = sort_live_digits(oa[1][0], oa[1][1], shift);
    for (int p = 0; p < n_hi; ++p) {
        if (!emu_pass(kb[kc].data(), ib[ic].data(), kb[kc ^ 1].data(), ib[ic ^ 1].data(), N, shift[p], hist, chunk_sum)) return 3002;
        kc ^= 1; ic ^= 1;
    }
    stats[4] = (uint64_t)n_end; stats[5] = (uint64_t)n_hi;
    for (int h = 0; h < 2; ++h) if (kb[h][(size_t)N] != kGuard64 || ib[h][(size_t)N] != kGuard32) return 3003;       // a write past the columns
    std::vector<uint32_t> mark((size_t)N + 1, kGuard32);
    launch(blocks_for(N, RSQC_JUNC_THREADS), [&]() { junction_heads_kernel(kb[kc].data(), ib[ic].data(), S.end.data(), N, mark.data()); });
    unsigned long long rows = 0;
    emu_scan(mark.data(), N, chunk_sum, &rows);
    if (mark[(size_t)N] != kGuard32) return 3004;
    if (rows == 0 || rows > N) return 3005;
    S.tid.assign((size_t)rows + 1, (int32_t)kGuard32); S.start.assign((size_t)rows + 1, (int32_t)kGuard32); S.end_h.assign((size_t)rows + 1, (int32_t)kGuard32);
    S.reads.assign((size_t)rows + 1, 0); S.hq.assign((size_t)rows + 1, 0); S.ov.assign((size_t)rows + 1, 0);
    JunctionRows R{S.tid.data(), S.start.data(), S.end_h.data(), S.reads.data(), S.hq.data(), S.ov.data()};
    launch(blocks_for(N, RSQC_JUNC_THREADS), [&]() { junction_reduce_kernel(kb[kc].data(), ib[ic].data(), S.end.data(), S.info.data(), N, mark.data(), &rows, R); });
    if (S.tid[(size_t)rows] != (int32_t)kGuard32 || S.reads[(size_t)rows] != 0 || S.hq[(size_t)rows] != 0 || S.ov[(size_t)rows] != 0) return 3006;
    stats[0] = rows;
    return 0;
}

EMU_API void juncemu_rows(int32_t *tid, int32_t *start, int32_t *end, uint32_t *reads, uint32_t *hq, uint32_t *ov) {
    const size_t n = S.tid.empty() ? 0 : S.tid.size() - 1;
    for (size_t k = 0; k < n; ++k) { tid[k] = S.tid[k]; start[k] = S.start[k]; end[k] = S.end_h[k]; reads[k] = S.reads[k]; hq[k] = S.hq[k]; ov[k] = S.ov[k]; }
}
