// rsqc_sam.hip -- device-side SAM text decode on MI355X (gfx950): the kernels around the per-lane bodies of rsqc_sam.h and
// their launches.  Input: one window of text in the decode's window buffer (plain SAM copied up, or BGZF-compressed SAM
// after bgzf_inflate_kernel); output: the DecodeWindow columns and DecodeSummary the BAM path fills (rsqc_decode.h).
// No lane walks SEQ or QUAL: the bitmap stage reads every byte once, coalesced, and the later stages hop the tab bitmap.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rsqc_sam.h"

namespace rsqc {

// exclusive sums of a workgroup of 256 threads (one value per thread; the total in `total`)
__device__ __forceinline__ uint32_t sam_block_scan(uint32_t v, uint32_t *lds /* [256] */, uint32_t &total) {
    const uint32_t t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 256u; d <<= 1) {
        const uint32_t x = t >= d ? lds[t - d] : 0u;
        __syncthreads();
        lds[t] += x;
        __syncthreads();
    }
    total = lds[255];
    const uint32_t incl = lds[t];
    __syncthreads();
    return incl - v;
}
__device__ __forceinline__ uint32_t sam_count(const uint32_t *n_dev, uint32_t n_cap) {
    if (!n_dev) return n_cap;
    const uint32_t n = *n_dev;
    return n < n_cap ? n : n_cap;
}

// ---- bitmap: one lane per 64-byte word, one workgroup per segment of 256 words ---------------------------------------
__global__ __launch_bounds__(256) void sam_bitmap_kernel(SamWindow S) {
    __shared__ uint32_t s_rec, s_nl, s_last;
    if (threadIdx.x == 0) { s_rec = 0; s_nl = 0; s_last = 0; }
    __syncthreads();
    const uint32_t w = blockIdx.x * SAM_SEG_WORDS + threadIdx.x;
    if (w < S.n_words) {
        const SamWordCounts c = sam_bitmap_word(S, w);
        if (c.rec) atomicAdd(&s_rec, c.rec);
        if (c.nl) { atomicAdd(&s_nl, c.nl); atomicMax(&s_last, c.last_nl1); }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        S.seg_cnt[blockIdx.x] = s_rec;
        if (s_nl) { atomicAdd(&S.st->n_nl, s_nl); atomicMax(&S.st->last_nl1, s_last); }
    }
}

// ---- exclusive scan of n values (n on the device when n_dev != null, at most n_cap): sums per 256, one workgroup over
// those, then the positions inside every workgroup
__global__ __launch_bounds__(256) void sam_scan_sums_kernel(const uint32_t *in, const uint32_t *n_dev, uint32_t n_cap, uint32_t *blk) {
    __shared__ uint32_t lds[256];
    const uint32_t n = sam_count(n_dev, n_cap);
    if (blockIdx.x * 256u >= n) return;                                  // (uniform: grids are sized for n_cap)
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t tot;
    (void)sam_block_scan(i < n ? in[i] : 0u, lds, tot);
    if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}
__global__ __launch_bounds__(1024) void sam_scan_top_kernel(uint32_t *blk, const uint32_t *n_dev, uint32_t n_cap, uint32_t *total_out) {
    __shared__ uint32_t s[1024];
    const uint32_t t = threadIdx.x, n = sam_count(n_dev, n_cap), n_blk = (n + 255u) / 256u;
    const uint32_t per = (n_blk + 1023u) / 1024u, lo = min(n_blk, t * per), hi = min(n_blk, lo + per);
    uint32_t a = 0;
    for (uint32_t k = lo; k < hi; ++k) a += blk[k];
    s[t] = a;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint32_t x = t >= d ? s[t - d] : 0u;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    uint32_t r = s[t] - a;
    for (uint32_t k = lo; k < hi; ++k) { const uint32_t x = blk[k]; blk[k] = r; r += x; }
    if (t == 0 && total_out) *total_out = s[1023];
}
__global__ __launch_bounds__(256) void sam_scan_place_kernel(const uint32_t *in, const uint32_t *n_dev, uint32_t n_cap, const uint32_t *blk, uint32_t *out) {
    __shared__ uint32_t lds[256];
    const uint32_t n = sam_count(n_dev, n_cap);
    if (blockIdx.x * 256u >= n) return;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t tot;
    const uint32_t x = sam_block_scan(i < n ? in[i] : 0u, lds, tot);
    if (i < n) out[i] = blk[blockIdx.x] + x;
}

// ---- lines: the '\n' of every record line, in order ------------------------------------------------------------------
__global__ __launch_bounds__(256) void sam_lines_kernel(SamWindow S) {
    __shared__ uint32_t lds[256];
    const uint32_t w = blockIdx.x * SAM_SEG_WORDS + threadIdx.x;
    const uint32_t c = w < S.n_words ? (uint32_t)__popcll(S.ebits[w]) : 0u;
    uint32_t tot;
    const uint32_t k = sam_block_scan(c, lds, tot);
    if (c) sam_lines_word(S, w, S.seg_k0[blockIdx.x] + k);
}

// ---- header: lines in front of the stream's first record that start with '@' ---------------------------------------
__global__ __launch_bounds__(256) void sam_header_kernel(SamWindow S) {
    if (S.sc->records_seen) return;
    const uint32_t n = min(S.st->n_lines, S.rec_cap);
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u)
        if (!sam_is_header_line(S, i)) { atomicMin(&S.st->hdr_end, i); break; }
}
__global__ void sam_settle_kernel(SamWindow S) { sam_settle(S); }

// ---- fields / parse / marks: one lane per record ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void sam_fields_kernel(SamWindow S) {
    const uint32_t n = S.W.sum->n_rec;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < n; j += gridDim.x * 256u) S.nops[j] = sam_fields_one(S, j);
}
__global__ __launch_bounds__(256) void sam_parse_kernel(SamWindow S) {
    const uint32_t n = S.W.sum->n_rec;
    uint32_t first = SAM_NONE, code = 0;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < n; j += gridDim.x * 256u) {
        const uint32_t rc = sam_parse_one(S, j);
        if (rc != SAM_OK && j < first) { first = j; code = rc; }
    }
    if (first != SAM_NONE) {
        atomicOr(&S.W.sum->status, DEC_ST_BAD_RECORD);
        atomicMin(&S.st->first_bad, first);
        S.st->bad_code = code;                                           // (one of the codes; the host re-parses the first bad line)
    }
}
__global__ __launch_bounds__(256) void sam_mark_kernel(SamWindow S) {
    if (S.W.sum->status) return;
    const uint32_t n = S.W.sum->n_rec;
    bool unsorted = false;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < n; j += gridDim.x * 256u) sam_mark_one(S, j, unsorted);
    if (unsorted) S.W.sum->unsorted = 1u;
}

// ---- lists: rsqc_decode.hip's three-launch shape, SAM write step ----------------------------------------------------
constexpr uint32_t SAM_LIST_PER_THREAD = 32, SAM_LIST_BLOCK = 256 * SAM_LIST_PER_THREAD;
struct SamListBlock { uint32_t seg, wide, bad; int32_t last_judged; };
__global__ __launch_bounds__(256) void sam_lists_count_kernel(SamWindow S, SamListBlock *blk) {
    __shared__ uint32_t lds[256];
    __shared__ int32_t s_last;
    if (S.W.sum->status) return;
    const uint32_t n = S.W.sum->n_rec;
    const uint32_t first = blockIdx.x * SAM_LIST_BLOCK;
    if (first >= n) return;
    const uint32_t lo = min(n, first + threadIdx.x * SAM_LIST_PER_THREAD), hi = min(n, lo + SAM_LIST_PER_THREAD);
    if (threadIdx.x == 0) s_last = -1;
    DecodeListCounts c;
    decode_lists_count(S.W, lo, hi, c);
    uint32_t ts, tw, tb;
    (void)sam_block_scan(c.seg, lds, ts); (void)sam_block_scan(c.wide, lds, tw); (void)sam_block_scan(c.bad, lds, tb);
    if (c.last_judged >= 0) atomicMax(&s_last, c.last_judged);
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = SamListBlock{ts, tw, tb, s_last};
}
__global__ __launch_bounds__(1024) void sam_lists_top_kernel(SamWindow S, SamListBlock *blk) {
    __shared__ uint32_t s_seg[1024], s_wide[1024], s_bad[1024];
    __shared__ int32_t s_last;
    if (S.W.sum->status) return;
    const uint32_t t = threadIdx.x, n = S.W.sum->n_rec, n_blk = (n + SAM_LIST_BLOCK - 1) / SAM_LIST_BLOCK;
    const uint32_t per = (n_blk + 1023u) / 1024u, lo = min(n_blk, t * per), hi = min(n_blk, lo + per);
    if (t == 0) s_last = -1;
    __syncthreads();
    uint32_t a = 0, b = 0, d = 0; int32_t last = -1;
    for (uint32_t k = lo; k < hi; ++k) { a += blk[k].seg; b += blk[k].wide; d += blk[k].bad; if (blk[k].last_judged >= 0) last = blk[k].last_judged; }
    s_seg[t] = a; s_wide[t] = b; s_bad[t] = d;
    if (last >= 0) atomicMax(&s_last, last);
    __syncthreads();
    for (uint32_t st = 1; st < 1024u; st <<= 1) {
        const uint32_t x = t >= st ? s_seg[t - st] : 0u, y = t >= st ? s_wide[t - st] : 0u, z = t >= st ? s_bad[t - st] : 0u;
        __syncthreads();
        s_seg[t] += x; s_wide[t] += y; s_bad[t] += z;
        __syncthreads();
    }
    uint32_t ra = s_seg[t] - a, rb = s_wide[t] - b, rd = s_bad[t] - d;
    for (uint32_t k = lo; k < hi; ++k) {
        const SamListBlock x = blk[k];
        blk[k] = SamListBlock{ra, rb, rd, x.last_judged};
        ra += x.seg; rb += x.wide; rd += x.bad;
    }
    if (t == 0) sam_lists_finish(S, n, DecodeListCounts{s_seg[1023], s_wide[1023], s_bad[1023], s_last});
}
__global__ __launch_bounds__(256) void sam_lists_write_kernel(SamWindow S, const SamListBlock *blk) {
    __shared__ uint32_t lds[256];
    if (S.W.sum->status) return;
    const uint32_t n = S.W.sum->n_rec;
    const uint32_t first = blockIdx.x * SAM_LIST_BLOCK;
    if (first >= n) return;
    const uint32_t lo = min(n, first + threadIdx.x * SAM_LIST_PER_THREAD), hi = min(n, lo + SAM_LIST_PER_THREAD);
    DecodeListCounts c;
    decode_lists_count(S.W, lo, hi, c);
    uint32_t tot;
    const uint32_t s0 = sam_block_scan(c.seg, lds, tot), w0 = sam_block_scan(c.wide, lds, tot), b0 = sam_block_scan(c.bad, lds, tot);
    if (c.seg | c.wide | c.bad) {
        const SamListBlock base = blk[blockIdx.x];
        sam_lists_write(S, lo, hi, DecodeListCounts{base.seg + s0, base.wide + w0, base.bad + b0, -1});
    }
}

// ---- launches ----------------------------------------------------------------------------------------------------
void launch_sam_window(hipStream_t s, const SamWindow &S, uint32_t *scratch) {
    // scratch: [0, 16) unused, then the per-workgroup sums of the line scan, of the operation scan, the lists' blocks
    const uint32_t rec_blocks = (S.rec_cap + 255u) / 256u;
    const uint32_t seg_sum_blocks = (S.n_seg + 255u) / 256u;
    uint32_t *blk_ops = scratch + 16, *blk_seg = blk_ops + rec_blocks + 1024;
    SamListBlock *lblk = (SamListBlock *)(blk_seg + seg_sum_blocks + 1024);
    const uint32_t rec_grid = std::min<uint32_t>(std::max<uint32_t>(rec_blocks, 1u), 256u * 16u);
    if (S.n_seg) {
        sam_bitmap_kernel<<<S.n_seg, 256, 0, s>>>(S);
        sam_scan_sums_kernel<<<seg_sum_blocks, 256, 0, s>>>(S.seg_cnt, nullptr, S.n_seg, blk_seg);
    }
    sam_scan_top_kernel<<<1, 1024, 0, s>>>(blk_seg, nullptr, S.n_seg, &S.st->n_lines);
    if (S.n_seg) {
        sam_scan_place_kernel<<<seg_sum_blocks, 256, 0, s>>>(S.seg_cnt, nullptr, S.n_seg, blk_seg, S.seg_k0);
        sam_lines_kernel<<<S.n_seg, 256, 0, s>>>(S);
    }
    sam_header_kernel<<<rec_grid, 256, 0, s>>>(S);
    sam_settle_kernel<<<1, 1, 0, s>>>(S);
    sam_fields_kernel<<<rec_grid, 256, 0, s>>>(S);
    const uint32_t *n_rec = &S.W.sum->n_rec;
    sam_scan_sums_kernel<<<rec_blocks, 256, 0, s>>>(S.nops, n_rec, S.rec_cap, blk_ops);
    sam_scan_top_kernel<<<1, 1024, 0, s>>>(blk_ops, n_rec, S.rec_cap, &S.W.sum->n_ops);
    sam_scan_place_kernel<<<rec_blocks, 256, 0, s>>>(S.nops, n_rec, S.rec_cap, blk_ops, S.W.ops_at);
    sam_parse_kernel<<<rec_grid, 256, 0, s>>>(S);
    sam_mark_kernel<<<rec_grid, 256, 0, s>>>(S);
    const uint32_t list_blocks = (S.rec_cap + SAM_LIST_BLOCK - 1) / SAM_LIST_BLOCK;
    sam_lists_count_kernel<<<list_blocks, 256, 0, s>>>(S, lblk);
    sam_lists_top_kernel<<<1, 1024, 0, s>>>(S, lblk);
    sam_lists_write_kernel<<<list_blocks, 256, 0, s>>>(S, lblk);
}

}  // namespace rsqc
