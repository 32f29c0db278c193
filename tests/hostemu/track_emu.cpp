// track_emu.cpp -- TEST HARNESS ONLY (never loaded by the product).
//
// The KERNELS of --bedgraph -- rnaseqc_amd/csrc/rsqc_track.h (events, head count, rows, line lengths, format) and the scan of
// rnaseqc_amd/csrc/rsqc_sort.h they use, unmodified -- compiled for the host on top of the 64-lane fiber emulation of wavemu.h.  The
// host side of rsqc_track_api.cpp (the layout of the difference array, the order of the stages, the row count) is restated here with
// plain memory.  The expected track is NOT computed here: tests/track_ref.py restates the contract in Python and the test compares.
#include "wavemu.h"

#include <algorithm>
#include <string>
#include <vector>

#include "../../rnaseqc_amd/csrc/rsqc_sort.h"
#include "../../rnaseqc_amd/csrc/rsqc_track.h"

using namespace rsqc;

namespace {
template <class F> void launch(uint32_t grid, F &&body) {
    wavemu::grid_dim().x = grid;
    for (uint32_t b = 0; b < grid; ++b) { wavemu::block_idx().x = b; wavemu::run_block(RSQC_TRACK_THREADS, body); }
}
uint32_t blocks_for(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

void emu_scan(uint32_t *data, uint64_t m, std::vector<unsigned long long> &chunk_sum, unsigned long long *total) {
    const uint32_t chunks = blocks_for(m, RSQC_SCAN_CHUNK);
    chunk_sum.assign((size_t)chunks + 1, 0xDEADull);
    if (chunks) launch(chunks, [&]() { sort_scan_sum_kernel(data, m, chunk_sum.data()); });
    launch(1, [&]() { sort_scan_top_kernel(chunk_sum.data(), chunks, total); });
    if (chunks) launch(chunks, [&]() { sort_scan_apply_kernel(data, m, chunk_sum.data()); });
}

constexpr uint32_t kGuard32 = 0xA5A5A5A5u;
struct State {
    int32_t n = 0; uint64_t total = 0; bool merge_later = false;
    std::vector<uint64_t> off; std::vector<uint32_t> length, name_off; std::string names;
    std::vector<uint32_t> diff;                        // total + 1 slots + one guard
    unsigned long long sums[3] = {0, 0, 0};
    std::vector<int32_t> tid; std::vector<uint32_t> start, end, depth;       // rows + one guard each
    std::vector<char> text;
} S;

// line lengths, their scan, the lines: rows [first, first + n) of R into S.text.  Returns 0, or 4000 + k for check k
int format_window(const TrackRows &R, uint64_t first, uint32_t n) {
    S.text.clear();
    if (!n) return 0;
    std::vector<uint32_t> len((size_t)n + 1, kGuard32);
    std::vector<unsigned long long> chunk_sum;
    launch(blocks_for(n, RSQC_TRACK_THREADS), [&]() { track_linelen_kernel(R, first, n, S.name_off.data(), len.data()); });
    unsigned long long bytes = 0;
    emu_scan(len.data(), n, chunk_sum, &bytes);
    if (len[(size_t)n] != kGuard32) return 4001;
    S.text.assign((size_t)bytes + 8, (char)0x7F);
    launch(blocks_for(n, RSQC_TRACK_THREADS), [&]() { track_format_kernel(R, first, n, S.name_off.data(), S.names.data(), len.data(), S.text.data()); });
    for (size_t k = (size_t)bytes; k < S.text.size(); ++k) if (S.text[k] != (char)0x7F) return 4002;       // a write past the window
    for (size_t k = 0; k < (size_t)bytes; ++k) if (S.text[k] == (char)0x7F) return 4003;                   // a byte no line wrote
    S.text.resize((size_t)bytes);
    return 0;
}
}  // namespace

#define EMU_API extern "C" __attribute__((visibility("default")))

EMU_API void trackemu_set_schedule_seed(unsigned long long seed) { wavemu::set_seed(seed); }

// names: the contigs' names one behind the other, name_len[t] bytes each
EMU_API void trackemu_begin(int32_t n, const uint64_t *length, const char *names, const uint32_t *name_len, int merge_later) {
    S = State{};
    S.n = n; S.merge_later = merge_later != 0;
    S.off.assign((size_t)n + 1, 0); S.length.assign((size_t)n + 1, 0); S.name_off.assign((size_t)n + 1, 0);
    for (int32_t t = 0; t < n; ++t) {
        S.length[(size_t)t] = (uint32_t)length[t];
        S.off[(size_t)t + 1] = S.off[(size_t)t] + length[t] + 1;
        S.name_off[(size_t)t + 1] = S.name_off[(size_t)t] + name_len[t];
    }
    S.names.assign(names, S.name_off[(size_t)n]);
    S.total = S.off[(size_t)n];
    S.diff.assign((size_t)S.total + 2, 0);
    S.diff[(size_t)S.total + 1] = kGuard32;
}

// one batch through the events kernel.  Returns 1 when the guard word was written
EMU_API int trackemu_add_batch(const rsqc_rec_core *core, const rsqc_rec_aux *aux, uint64_t n, const uint32_t *cigar, uint64_t n_ops,
                               const int32_t *seg_tid, const uint64_t *seg_start, uint32_t n_seg, const uint64_t *wide_index, const uint32_t *wide_n_cigar, uint32_t n_wide) {
    if (!n) return 0;
    TrackBatch B{core, aux, cigar, n, n_ops, seg_tid, seg_start, n_seg, wide_index, wide_n_cigar, n_wide};
    TrackArray A{S.diff.data(), S.off.data(), S.length.data(), S.n, S.sums};
    if (S.merge_later) launch(blocks_for(n, RSQC_TRACK_THREADS), [&]() { track_events_kernel<true>(B, A); });
    else launch(blocks_for(n, RSQC_TRACK_THREADS), [&]() { track_events_kernel<false>(B, A); });
    return S.diff[(size_t)S.total + 1] != kGuard32 ? 1 : 0;
}

// scan, count, rows.  stats: [0] rows, [1] population, [2] aligned bases, [3] clipped bases, [4] positions, [5] chunks of the row
// kernels.  Returns 0, or 3000 + k for check k of the harness itself
EMU_API int trackemu_end(uint64_t *stats) {
    stats[0] = 0; stats[1] = S.sums[0]; stats[2] = S.sums[1]; stats[3] = S.sums[2]; stats[4] = S.total - (uint64_t)S.n; stats[5] = 0;
    S.tid.clear(); S.start.clear(); S.end.clear(); S.depth.clear();
    if (!S.total) return 0;
    // every contig's slots sum to zero: the pads read 0 after the scan
    std::vector<unsigned long long> chunk_sum;
    unsigned long long all = 0, rows = 0;
    emu_scan(S.diff.data(), S.total + 1, chunk_sum, &all);
    if (S.diff[(size_t)S.total + 1] != kGuard32) return 3001;
    for (int32_t t = 0; t < S.n; ++t) if (S.diff[(size_t)(S.off[(size_t)t + 1] - 1) + 1] != 0u) return 3002;       // (the depth of slot i is at i + 1)
    const uint32_t chunks = blocks_for(S.total, RSQC_TRACK_CHUNK);
    stats[5] = chunks;
    std::vector<uint32_t> count((size_t)chunks + 1, kGuard32);
    launch(chunks, [&]() { track_count_kernel(S.diff.data(), S.total, count.data()); });
    emu_scan(count.data(), chunks, chunk_sum, &rows);
    if (count[(size_t)chunks] != kGuard32) return 3003;
    S.tid.assign((size_t)rows + 1, (int32_t)kGuard32); S.start.assign((size_t)rows + 1, kGuard32); S.end.assign((size_t)rows + 1, kGuard32); S.depth.assign((size_t)rows + 1, kGuard32);
    TrackRows R{S.tid.data(), S.start.data(), S.end.data(), S.depth.data()};
    launch(chunks, [&]() { track_rows_kernel(S.diff.data(), S.total, count.data(), S.off.data(), S.n, rows, R); });
    if (S.tid[(size_t)rows] != (int32_t)kGuard32 || S.start[(size_t)rows] != kGuard32 || S.end[(size_t)rows] != kGuard32 || S.depth[(size_t)rows] != kGuard32) return 3004;
    stats[0] = rows;
    return 0;
}

EMU_API void trackemu_rows(int32_t *tid, uint32_t *start, uint32_t *end, uint32_t *depth) {
    const size_t n = S.tid.empty() ? 0 : S.tid.size() - 1;
    for (size_t k = 0; k < n; ++k) { tid[k] = S.tid[k]; start[k] = S.start[k]; end[k] = S.end[k]; depth[k] = S.depth[k]; }
}

// the text of rows [first, first + n) of the pass's table; returns its bytes (negative: a check of the harness failed)
EMU_API long long trackemu_text(uint64_t first, uint32_t n) {
    TrackRows R{S.tid.data(), S.start.data(), S.end.data(), S.depth.data()};
    const int rc = format_window(R, first, n);
    return rc ? -(long long)rc : (long long)S.text.size();
}
// the text of INJECTED rows (coordinates the suite cannot reach through a difference array), with the names of trackemu_begin
EMU_API long long trackemu_text_injected(uint32_t n, int32_t *tid, uint32_t *start, uint32_t *end, uint32_t *depth) {
    TrackRows R{tid, start, end, depth};
    const int rc = format_window(R, 0, n);
    return rc ? -(long long)rc : (long long)S.text.size();
}
EMU_API void trackemu_text_copy(char *out) { if (!S.text.empty()) memcpy(out, S.text.data(), S.text.size()); }
