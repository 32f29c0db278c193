// rsqc_track.hip -- launchers of the --bedgraph kernels (rsqc_track.h); the host side that drives them is rsqc_track_api.cpp.
#define RSQC_TRACK_KERNELS
#include "rsqc_track.h"

namespace rsqc {

static inline uint32_t blocks_for(uint64_t n, uint32_t per_block) { return (uint32_t)((n + per_block - 1) / per_block); }

void launch_track_events(hipStream_t s, const TrackBatch &B, const TrackArray &A, bool merge_later) {
    if (!B.n) return;
    if (merge_later) track_events_kernel<true><<<blocks_for(B.n, RSQC_TRACK_THREADS), RSQC_TRACK_THREADS, 0, s>>>(B, A);
    else track_events_kernel<false><<<blocks_for(B.n, RSQC_TRACK_THREADS), RSQC_TRACK_THREADS, 0, s>>>(B, A);
}
void launch_track_count(hipStream_t s, const uint32_t *S, uint64_t total, uint32_t *count) {
    if (total) track_count_kernel<<<blocks_for(total, RSQC_TRACK_CHUNK), RSQC_TRACK_THREADS, 0, s>>>(S, total, count);
}
void launch_track_rows(hipStream_t s, const uint32_t *S, uint64_t total, const uint32_t *heads_before, const uint64_t *off, int32_t n_contigs, uint64_t n_rows, const TrackRows &R) {
    if (total) track_rows_kernel<<<blocks_for(total, RSQC_TRACK_CHUNK), RSQC_TRACK_THREADS, 0, s>>>(S, total, heads_before, off, n_contigs, n_rows, R);
}
void launch_track_linelen(hipStream_t s, const TrackRows &R, uint64_t first, uint32_t n, const uint32_t *name_off, uint32_t *len) {
    if (n) track_linelen_kernel<<<blocks_for(n, RSQC_TRACK_THREADS), RSQC_TRACK_THREADS, 0, s>>>(R, first, n, name_off, len);
}
void launch_track_format(hipStream_t s, const TrackRows &R, uint64_t first, uint32_t n, const uint32_t *name_off, const char *names, const uint32_t *at, char *text) {
    if (n) track_format_kernel<<<blocks_for(n, RSQC_TRACK_THREADS), RSQC_TRACK_THREADS, 0, s>>>(R, first, n, name_off, names, at, text);
}

}  // namespace rsqc
