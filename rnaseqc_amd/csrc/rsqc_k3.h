// rsqc_k3.h -- K3, the end-of-file coverage stage (src/Metrics.cpp:132-151,160-235,265-337): per gene, the difference array
// becomes the stitched coverage vector, then per-exon CV, the 3'/5' bias windows and the gene's mean / std / CV.
// Device code only, included by rsqc_kernels.hip -- and, unmodified, by the host SIMT emulation of the tests
// (tests/hostemu/k3_emu.cpp), which runs it on the CPU against the oracle.
#pragma once

namespace rsqc {

// ------------------------------------------------------------------ K3
// barrier of a T-thread workgroup; a one-wave "workgroup" only needs its LDS traffic ordered (it is executed in order)
template <int T> __device__ __forceinline__ void k3_sync() {
    if constexpr (T > 64) __syncthreads();
    else { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); }
}
// One workgroup per gene, longest genes first.  cov[] holds the per-base DIFFERENCE array of the
// gene's exons, contiguous in exonsForGene order (+1 pad slot), so a plain prefix sum yields the
// stitched transcript vector of computeCoverage (src/Metrics.cpp:306-308).
// A gene is one latency-bound chain, so the stage's time is (genes / genes in flight) x (length of a gene's chain): the
// workgroup is sized to the gene.  Most genes have a few thousand coding bases and run as ONE WAVE each (T = 64: barriers
// degenerate to in-order LDS traffic and thousands of genes are in flight); longer ones get 256 or 1024 threads.
// The chain of a gene that fits its instance (k3_gene_in_registers): one scan that also yields the maximum, the non-zero
// count and the masked sums; one pass per exon; when the gate opens, one register pass per byte of the select, one for the
// trim, the two window medians, and one more over the trimmed range -- each closed by one combined reduction.
// A gene that does not fit (longer than the instance's LDS, or deeper than its 16-bit cells) runs the general path below from
// memory: one pass per statistic (maximum, non-zero count, select, trim, mean, deviation; two per exon).
template <int T_, int WIN_, class CovT_, int LDSCAP_>
struct K3Shared {
    static constexpr int T = T_, WIN = WIN_, W = T_ / 64, LDSCAP = LDSCAP_;
    CovT_ covbuf[LDSCAP_ > 0 ? LDSCAP_ : 1];         // the gene's coverage vector when it fits (see the kernel)
    unsigned long long u64[W];
    double f64[W];
    uint32_t u32a[W], u32b[W];
    uint32_t hist[256];
    uint32_t win[2][WIN];
    uint32_t bc_u32[4]; double bc_f64[2];
};

template <class SH> __device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, SH &S) {
    constexpr int T = SH::T;
    v = wave_sum(v);
    k3_sync<T>();
    if (lane_id() == 0) S.u64[threadIdx.x >> 6] = v;
    k3_sync<T>();
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < (T / 64); ++w) t += S.u64[w];
    return t;
}
template <class SH> __device__ __forceinline__ double block_sum_f64(double v, SH &S) {
    constexpr int T = SH::T;
    v = wave_sum(v);
    k3_sync<T>();
    if (lane_id() == 0) S.f64[threadIdx.x >> 6] = v;
    k3_sync<T>();
    double t = 0;
#pragma unroll
    for (int w = 0; w < (T / 64); ++w) t += S.f64[w];
    return t;
}
template <class SH> __device__ __forceinline__ uint32_t block_min_u32(uint32_t v, SH &S) {
    constexpr int T = SH::T;
    v = wave_min_u32(v);
    k3_sync<T>();
    if (lane_id() == 0) S.u32a[threadIdx.x >> 6] = v;
    k3_sync<T>();
    uint32_t t = 0xFFFFFFFFu;
#pragma unroll
    for (int w = 0; w < (T / 64); ++w) t = S.u32a[w] < t ? S.u32a[w] : t;
    return t;
}
template <class SH> __device__ __forceinline__ uint32_t block_max_u32(uint32_t v, SH &S) {
    constexpr int T = SH::T;
    v = wave_max_u32(v);
    k3_sync<T>();
    if (lane_id() == 0) S.u32a[threadIdx.x >> 6] = v;
    k3_sync<T>();
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < (T / 64); ++w) t = S.u32a[w] > t ? S.u32a[w] : t;
    return t;
}

// quirky computeMedian (src/Metrics.h:147-160) of a window held in LDS (unsorted): the two middle
// order statistics are found by rank counting.  Called by the whole block; result broadcast.
template <class SH> __device__ __forceinline__ bool window_median(const uint32_t *w, uint32_t n, double *out, SH &S) {
    constexpr int T = SH::T;
    if (n == 0) return false;
    if (n == 1) { *out = (double)w[0]; return true; }
    const uint32_t mid = (n - 1) / 2;
    k3_sync<T>();
    for (uint32_t i = threadIdx.x; i < n; i += T) {
        const uint32_t v = w[i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; ++j) { const uint32_t u = w[j]; rank += (u < v || (u == v && j < i)) ? 1u : 0u; }
        if (rank == mid) S.bc_u32[0] = v;
        if (rank == mid + 1) S.bc_u32[1] = v;
    }
    k3_sync<T>();
    *out = (n & 1u) ? ((double)S.bc_u32[0] + (double)S.bc_u32[1]) / 2.0 : (double)S.bc_u32[0];
    return true;
}

// ------------------------------------------------------------------ a gene that fits its instance: the vector stays in registers
// sum of a 64-bit value over the wave (all 64 lanes active), in every lane: the six DPP steps of wave_sum_u32_full on both halves
__device__ __forceinline__ unsigned long long wave_sum_u64_full(unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
#define RSQC_DPP_ADD64(ctrl, rmask) { const uint32_t lo_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, ctrl, rmask, 0xf, false); \
                                      const uint32_t hi_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), ctrl, rmask, 0xf, false); \
                                      v += ((unsigned long long)hi_ << 32) | lo_; }
    RSQC_DPP_ADD64(0x111, 0xf) RSQC_DPP_ADD64(0x112, 0xf) RSQC_DPP_ADD64(0x114, 0xf) RSQC_DPP_ADD64(0x118, 0xf)
    RSQC_DPP_ADD64(0x142, 0xa) RSQC_DPP_ADD64(0x143, 0xc)
#undef RSQC_DPP_ADD64
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
    return ((unsigned long long)hi << 32) | lo;
#else
    return wave_sum(v);
#endif
}
__device__ __forceinline__ int k3_bits(uint32_t v) { return v ? 32 - __builtin_clz(v) : 0; }
// may the squares of n depths of at most vmax be summed in 64 bits?  (n x vmax^2 < 2^(bits(n) + 2 bits(vmax)))
__device__ __forceinline__ bool k3_exact(uint32_t n, uint32_t vmax) { return k3_bits(n) + 2 * k3_bits(vmax) <= 64; }
// the population standard deviation of n integers from their exact sums: sqrt(n x sxx - sx^2) / n, the difference formed in 128 bits
// (n x sxx < 2^81 under k3_exact, and n x sxx >= sx^2) and rounded ONCE to a double: the top 64 bits, the bits below them kept as a
// sticky bit.  No cancellation: a flat vector gives exactly 0, depth 60 000 with a deviation below 1 keeps every digit.
__device__ __forceinline__ double k3_sd_exact(uint32_t n, unsigned long long sx, unsigned long long sxx) {
    const unsigned __int128 d = (unsigned __int128)n * sxx - (unsigned __int128)sx * sx;
    const unsigned long long hi = (unsigned long long)(d >> 64), lo = (unsigned long long)d;
    double dd;
    if (hi == 0) dd = (double)lo;
    else {
        const int s = __builtin_clzll(hi);
        const unsigned long long m = s ? (hi << s) | (lo >> (64 - s)) : hi, rest = s ? lo << s : lo;
        dd = (double)(m | (rest != 0ull ? 1ull : 0ull)) * __longlong_as_double((long long)(1023 + 64 - s) << 52);
    }
    return sqrt(dd) / (double)n;
}

// rounds of T x 16 bases that cover the instance's capacity: the registers a lane keeps its share of the vector in
template <int T, int LDSCAP> struct K3Reg {
    static constexpr int PER = 16;
    static constexpr int ROUNDS = LDSCAP > 0 ? (LDSCAP + T * PER - 1) / (T * PER) : 0;
    static constexpr int NV = ROUNDS * PER;
};
// the instances that keep every round in registers: 1 .. 4 rounds for one wave, 2 / 3 for 256 threads, 2 for the 64 KB class of 1024.
// The 146 KB class would need 5 rounds = 80 registers beside the passes' own, more than the 128 a 1024-thread workgroup's lanes
// have (the compiler spills ~360 of them): it keeps one round in registers while scanning and its passes read the LDS copy.
#ifndef RSQC_K3_REG_ROUNDS
#define RSQC_K3_REG_ROUNDS 4
#endif
template <int T, int LDSCAP> constexpr bool K3_IN_REGISTERS = K3Reg<T, LDSCAP>::ROUNDS >= 1 && K3Reg<T, LDSCAP>::ROUNDS <= RSQC_K3_REG_ROUNDS;

#ifdef RSQC_K1_PROF
#define RSQC_K3_PROF_SHAPE(in_lds_) do { if (first == 0 && threadIdx.x == 0) { s_fin_stamp[9] = coding; s_fin_stamp[10] = n_ex; s_fin_stamp[11] = (in_lds_); } } while (0)
#define RSQC_K3_PROF_PUBLISH do { if (first == 0 && threadIdx.x == 0) {                                                          \
        const unsigned long long tot = s_fin_stamp[8] - s_fin_stamp[0];                                                           \
        if (atomicMax(&g_fin_prof[31], tot) < tot) {                                                                              \
            for (int k = 0; k < 9; ++k) g_fin_prof[k] = s_fin_stamp[k];                                                           \
            g_fin_prof[28] = s_fin_stamp[9]; g_fin_prof[29] = s_fin_stamp[10]; g_fin_prof[30] = s_fin_stamp[11]; g_fin_prof[27] = blockIdx.x; \
        } } } while (0)
#else
#define RSQC_K3_PROF_SHAPE(in_lds_)
#define RSQC_K3_PROF_PUBLISH
#endif

// A counted gene of at most LDSCAP bases.  Lane l of wave w holds base rd x T x 16 + w x 1024 + k x 64 + l in r[rd x 16 + k] (the layout
// of the scan's loads, ascending in the register index) for every round, fully unrolled; the LDS copy serves what needs random access:
// exon rows, the gate window and the two bias windows.  The scan itself finds the maximum (lowest index among equal ones), the non-zero
// count and the integer sums of x and x^2 over the masked range, combined in ONE block reduction; the select, the trim and the sums of a
// trimmed range read registers; mean and deviation come from the two integer sums (k3_sd_exact), per exon too.
// KEEP = false (the 146 KB class): r[] holds the round being scanned only, and the same passes read the LDS copy instead.
// Returns false (for the whole workgroup, nothing written) when a depth does not fit the LDS cell: the caller runs the gene from memory.
template <int T, int WIN, class CovT, int LDSCAP, bool KEEP, class SH>
__device__ __forceinline__ bool k3_gene_in_registers(const GeneCovArgs &A, const uint32_t first, const int gene, const uint32_t coding, SH &S) {
    using RG = K3Reg<T, LDSCAP>;
    constexpr int PER = RG::PER, ROUNDS = RG::ROUNDS, NV = RG::NV;
    constexpr uint32_t RSTEP = (uint32_t)(T * PER), NW = (uint32_t)(T / 64);
    constexpr int UNR = KEEP ? NV : PER;                                    // (registers are indexed at compile time; LDS reads need not be)
    const int tid = (int)threadIdx.x;
    const int l = lane_id();
    const int wv = tid >> 6;
    const uint32_t e0 = A.ge_off[gene], e1 = A.ge_off[gene + 1], n_ex = e1 - e0;
    const uint32_t *const D = A.cov + A.gene_cov_off[gene];
    const uint32_t MASK = A.mask;
    const uint32_t W = (uint32_t)A.bias_window, OFF = (uint32_t)A.bias_offset;
    const uint32_t lo_t = MASK, hi_t = coding > MASK ? coding - MASK : 0;       // the masked range of the untrimmed vector
    const uint32_t jl = (uint32_t)wv * (64u * PER) + (uint32_t)l;
#define K3_POS(i) (jl + (uint32_t)((i) / PER) * RSTEP + (uint32_t)((i) % PER) * 64u)
#define K3_R(i) (KEEP ? (i) : (i) % PER)
#define K3_VALID(i) ((uint32_t)((i) / PER) < last_rd || ((uint32_t)((i) / PER) == last_rd && (uint32_t)((i) % PER) < cnt_last))
#define K3_VAL(i) (KEEP ? r[K3_R(i)] : (uint32_t)S.covbuf[K3_POS(i)])
    // combines per-lane partial sums over the workgroup (both in every thread)
    auto block_sum2 = [&](unsigned long long &a, unsigned long long &b) {
        a = wave_sum_u64_full(a); b = wave_sum_u64_full(b);
        if constexpr (T > 64) {
            k3_sync<T>();
            if (l == 0) { uint32_t *h = S.hist + wv * 4; h[0] = (uint32_t)a; h[1] = (uint32_t)(a >> 32); h[2] = (uint32_t)b; h[3] = (uint32_t)(b >> 32); }
            k3_sync<T>();
            a = 0; b = 0;
#pragma unroll 4
            for (uint32_t w = 0; w < NW; ++w) { const uint32_t *h = S.hist + w * 4; a += ((unsigned long long)h[1] << 32) | h[0]; b += ((unsigned long long)h[3] << 32) | h[2]; }
        }
    };
    // a lane's bases ascend with the register index, so "position below X" is "index below below(X)": the passes compare the
    // (compile-time) index with a few per-lane bounds and keep no positions
    auto below = [&](uint32_t X) -> uint32_t {
        const uint32_t q = X / RSTEP, rem = X - q * RSTEP;
        const uint32_t part = rem > jl ? (rem - jl + 63u) >> 6 : 0u;
        return q * (uint32_t)PER + (part < (uint32_t)PER ? part : (uint32_t)PER);
    };
    auto pos_of = [&](uint32_t i) -> uint32_t { return jl + (i / (uint32_t)PER) * RSTEP + (i % (uint32_t)PER) * 64u; };
    // this lane's bases are its first below(coding) registers: every one of the rounds before the gene's last, cnt_last of that one
    const uint32_t last_rd = (coding + RSTEP - 1u) / RSTEP - 1u;            // (uniform; coding >= 1)
    const uint32_t cnt_last = below(coding) - last_rd * (uint32_t)PER;
    RSQC_FIN_STAMP(0);
    // (1) every round's share of the difference array in flight at once (KEEP; else round by round), then the block-wide inclusive
    //     scan round by round.  (32-bit byte offsets from the gene's uniform base: coding <= LDSCAP.)
    uint32_t r[KEEP ? NV : PER];
    auto load_round = [&](int rd) {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = rd * PER + k;
            r[K3_R(i)] = K3_VALID(i) ? *(const uint32_t *)((const char *)D + (K3_POS(i) << 2)) : 0u;
        }
    };
    if constexpr (KEEP) {
#pragma unroll
        for (int rd = 0; rd < ROUNDS; ++rd) load_round(rd);
    }
    const uint32_t m_lo = below(lo_t), m_hi = below(hi_t);                  // the masked range, as indices
    uint32_t carry = 0, best = 0, best_k = 0xFFFFFFFFu, nnz = 0;
    unsigned long long sx = 0, sxx = 0;
#pragma unroll
    for (int rd = 0; rd < ROUNDS; ++rd) {
        if ((uint32_t)rd * RSTEP < coding) {                                // (uniform)
            if constexpr (!KEEP) load_round(rd);
            uint32_t run = 0;
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const uint32_t inc = wave_inclusive_scan_u32_dpp(r[K3_R(rd * PER + k)]);
                r[K3_R(rd * PER + k)] = inc + run;
                run += lane_value(inc, 63);
            }
            uint32_t before = carry, total = run;
            if constexpr (T > 64) {
                k3_sync<T>();
                if (l == 0) S.u32b[wv] = run;
                k3_sync<T>();
                total = 0;
#pragma unroll 4
                for (uint32_t w = 0; w < NW; ++w) { const uint32_t t = S.u32b[w]; if (w < (uint32_t)wv) before += t; total += t; }
            }
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int i = rd * PER + k;
                if (K3_VALID(i)) {
                    const uint32_t x = r[K3_R(i)] + before;
                    r[K3_R(i)] = x;
                    S.covbuf[K3_POS(i)] = (CovT)x;
                    if (x > best) { best = x; best_k = (uint32_t)i; }       // (a lane's positions ascend: the first of equal maxima stays)
                    nnz += x != 0u;
                    if ((uint32_t)i >= m_lo && (uint32_t)i < m_hi) { sx += x; sxx += (unsigned long long)x * x; }
                } else r[K3_R(i)] = 0u;
            }
            carry += total;
        }
    }
    uint32_t best_i = best_k == 0xFFFFFFFFu ? 0xFFFFFFFFu : pos_of(best_k);
    {
        const uint32_t wbest = wave_max_u32_full(best);
        best_i = wave_min_u32_full(best == wbest ? best_i : 0xFFFFFFFFu);
        best = wbest;
        nnz = wave_sum_u32_full(nnz); sx = wave_sum_u64_full(sx); sxx = wave_sum_u64_full(sxx);
        if constexpr (T > 64) {
            k3_sync<T>();
            if (l == 0) {
                uint32_t *h = S.hist + wv * 8;
                h[0] = best; h[1] = best_i; h[2] = nnz; h[3] = (uint32_t)sx; h[4] = (uint32_t)(sx >> 32); h[5] = (uint32_t)sxx; h[6] = (uint32_t)(sxx >> 32);
            }
            k3_sync<T>();
            best = 0; best_i = 0xFFFFFFFFu; nnz = 0; sx = 0; sxx = 0;
#pragma unroll 4
            for (uint32_t w = 0; w < NW; ++w) {
                const uint32_t *h = S.hist + w * 8;
                const uint32_t ob = h[0], oi = h[1];
                if (ob > best || (ob == best && oi < best_i)) { best = ob; best_i = oi; }
                nnz += h[2]; sx += ((unsigned long long)h[4] << 32) | h[3]; sxx += ((unsigned long long)h[6] << 32) | h[5];
            }
        }
    }
    if constexpr (sizeof(CovT) < 4) { if (best > (uint32_t)(CovT)~(CovT)0) { RSQC_FIN_STAMP(1); return false; } }    // (uniform)
    __threadfence_block();
    k3_sync<T>();
    RSQC_FIN_STAMP(2);
    RSQC_K3_PROF_SHAPE(2);
    // (2) per-exon CV over transcript positions [MASK, coding-MASK): one wave per exon at a time, ONE pass with two integer sums
    if (hi_t > lo_t) {
        const uint32_t gcov = A.gene_cov_off[gene];
        for (uint32_t k0 = (uint32_t)wv; k0 < n_ex; k0 += 64u * NW) {
            const uint32_t mine = k0 + (uint32_t)l * NW;
            uint32_t r_t0 = 0, r_len = 0, r_id = 0;
            if (mine < n_ex) {
                const uint32_t row = A.ge_row[e0 + mine];
                const ExonRow er = A.ex[row];
                r_t0 = er.cov - gcov; r_len = (uint32_t)(er.end - er.start + 1); r_id = A.ex_id[row];
            }
            const uint32_t left = (n_ex - k0 + NW - 1) / NW;
            const uint32_t cnt = left < 64u ? left : 64u;
            for (uint32_t i = 0; i < cnt; ++i) {
                const uint32_t t0 = lane_value(r_t0, (int)i), len = lane_value(r_len, (int)i), id = lane_value(r_id, (int)i);
                const uint32_t a0 = t0 > lo_t ? t0 : lo_t, b0 = (uint64_t)t0 + len < hi_t ? t0 + len : hi_t;
                if (b0 > a0) {
                    const uint32_t n = b0 - a0;
                    unsigned long long sm = 0, sq = 0;
#pragma unroll 4
                    for (uint32_t j = a0 + (uint32_t)l; j < b0; j += 64) { const uint32_t x = (uint32_t)S.covbuf[j]; sm += x; sq += (unsigned long long)x * x; }
                    sm = wave_sum_u64_full(sm);
                    const double mean = (double)sm / (double)n;
                    double cv;
                    if (k3_exact(n, best)) cv = k3_sd_exact(n, sm, wave_sum_u64_full(sq)) / mean;
                    else {
                        double q = 0.0;
#pragma unroll 4
                        for (uint32_t j = a0 + (uint32_t)l; j < b0; j += 64) { const double d = (double)(uint32_t)S.covbuf[j] - mean; q += d * d; }
                        cv = sqrt(wave_sum(q) / (double)n) / mean;
                    }
                    if (l == 0 && !(isnan(cv) || isinf(cv))) { A.e_cv[id] = cv; A.e_cv_valid[id] = 1; }
                }
            }
        }
    }
#ifdef RSQC_K1_PROF
    k3_sync<T>();
    RSQC_FIN_STAMP(3);
#endif
    // (3) bias on the stitched, unmasked coverage vector [0, coding)
    uint32_t v0 = 0, v1 = coding;
    if (coding >= A.bias_gene_length) {
        const uint32_t pp = best == 0 ? 0u : best_i;
        uint32_t cur = pp + W / 2 < coding ? pp + W / 2 : coding;
        const uint32_t n = W < cur ? W : cur;
        cur -= n;
        double gate = 0.0;
        if (n == 0) { if (tid == 0) atomicExch(A.error, RSQC_ERR_EMPTY_MEDIAN); }
        else if (n == 1) gate = (double)(uint32_t)S.covbuf[cur];
        else {
            const uint32_t mid = (n - 1) / 2;
            gate = (n & 1u) ? ((double)(uint32_t)S.covbuf[cur + mid] + (double)(uint32_t)S.covbuf[cur + mid + 1]) / 2.0 : (double)(uint32_t)S.covbuf[cur + mid];
        }
        RSQC_FIN_STAMP(4);
        if (n != 0 && gate >= 100.0) {
            // 5th percentile of the non-zero coverage = order statistic R of the whole vector: MSB-first radix select, values from registers
            uint32_t R = (coding - nnz) + (uint32_t)((double)nnz * 0.05);
            uint32_t prefix = 0, pmask = 0;
            const int top = best >> 24 ? 24 : best >> 16 ? 16 : best >> 8 ? 8 : 0;
            pmask = top == 24 ? 0u : 0xFFFFFFFFu << (top + 8);
            for (int shift = top; shift >= 0; shift -= 8) {
                k3_sync<T>();
                for (int h = tid; h < 256; h += T) S.hist[h] = 0;
                k3_sync<T>();
#pragma unroll UNR
                for (int i = 0; i < NV; ++i) {
                    if (K3_VALID(i)) { const uint32_t v = K3_VAL(i); if ((v & pmask) == prefix) atomicAdd(&S.hist[(v >> shift) & 0xFF], 1u); }
                }
                k3_sync<T>();
                if (wv == 0) {                                       // wave 0: lane x scans 4 bins
                    const uint32_t h0 = S.hist[4 * l], h1 = S.hist[4 * l + 1], h2 = S.hist[4 * l + 2], h3 = S.hist[4 * l + 3];
                    const uint32_t tot = h0 + h1 + h2 + h3;
                    const uint32_t inc = wave_inclusive_scan_u32_dpp(tot);
                    const uint32_t exc = inc - tot;
                    if (R >= exc && R < inc) {
                        uint32_t digit, rbase;
                        if (R < exc + h0) { digit = 4 * l; rbase = exc; }
                        else if (R < exc + h0 + h1) { digit = 4 * l + 1; rbase = exc + h0; }
                        else if (R < exc + h0 + h1 + h2) { digit = 4 * l + 2; rbase = exc + h0 + h1; }
                        else { digit = 4 * l + 3; rbase = exc + h0 + h1 + h2; }
                        S.bc_u32[2] = digit; S.bc_u32[3] = rbase;
                    }
                }
                k3_sync<T>();
                R -= S.bc_u32[3];
                prefix |= S.bc_u32[2] << shift; pmask |= 0xFFu << shift;
            }
            const uint32_t lower = prefix;
            RSQC_FIN_STAMP(5);
            // trim leading / trailing entries <= lower
            uint32_t first_k = 0xFFFFFFFFu, last_k = 0;
#pragma unroll UNR
            for (int i = 0; i < NV; ++i) {
                if (K3_VALID(i) && K3_VAL(i) > lower) { if (first_k == 0xFFFFFFFFu) first_k = (uint32_t)i; last_k = (uint32_t)i; }
            }
            uint32_t first_gt = wave_min_u32_full(first_k == 0xFFFFFFFFu ? 0xFFFFFFFFu : pos_of(first_k));
            uint32_t last_gt = wave_max_u32_full(first_k == 0xFFFFFFFFu ? 0u : pos_of(last_k) + 1u);
            if constexpr (T > 64) {
                k3_sync<T>();
                if (l == 0) { S.u32a[wv] = first_gt; S.u32b[wv] = last_gt; }
                k3_sync<T>();
#pragma unroll 4
                for (uint32_t w = 0; w < NW; ++w) { const uint32_t f = S.u32a[w], e = S.u32b[w]; first_gt = f < first_gt ? f : first_gt; last_gt = e > last_gt ? e : last_gt; }
            }
            if (first_gt == 0xFFFFFFFFu) { v0 = coding; v1 = coding; } else { v0 = first_gt; v1 = last_gt; }
            const uint32_t tlen = v1 - v0;
            RSQC_FIN_STAMP(6);
            if (tlen >= A.bias_gene_length) {
                // left window [OFF, min(OFF+W, tlen)), right window [tlen-W-OFF, tlen-OFF)
                const uint32_t lhi = OFF + W < tlen ? OFF + W : tlen;
                const uint32_t nl = OFF < lhi ? lhi - OFF : 0u;
                uint32_t nr = 0, rlo = 0;
                if ((uint64_t)W + OFF <= tlen) { rlo = tlen - W - OFF; nr = W; }
                k3_sync<T>();
                for (uint32_t j = tid; j < nl; j += T) S.win[0][j] = (uint32_t)S.covbuf[v0 + OFF + j];
                for (uint32_t j = tid; j < nr; j += T) S.win[1][j] = (uint32_t)S.covbuf[v0 + rlo + j];
                k3_sync<T>();
                double ml = 0.0, mr = 0.0;
                const bool okl = window_median(S.win[0], nl, &ml, S);
                const bool okr = window_median(S.win[1], nr, &mr, S);
                if (!(okl && okr)) { if (tid == 0) atomicExch(A.error, RSQC_ERR_EMPTY_MEDIAN); }
                else if (tid == 0) {
                    const bool fwd = (A.gene_flags[gene] & RSQC_FF_STRAND_MASK) == RSQC_STRAND_FORWARD;
                    A.bias3[gene] = (unsigned long long)(fwd ? mr : ml);      // unsigned long += double: truncation
                    A.bias5[gene] = (unsigned long long)(fwd ? ml : mr);
                }
            }
        }
    }
    RSQC_FIN_STAMP(7);
    // (4) gene mean / std / CV on positions [v0, v1) with MASK bases removed at both ends: the scan's sums when nothing was trimmed
    {
        const uint32_t len = v1 - v0;
        uint32_t a = v0, bnd = v1;
        if (MASK) {
            if (len > 2 * (uint64_t)MASK) { a = v0 + MASK; bnd = v1 - MASK; } else { a = bnd = v0; }
        }
        if (bnd > a) {
            const uint32_t n = bnd - a;
            const bool exact = k3_exact(n, best);
            const uint32_t t_lo = below(a), t_hi = below(bnd);              // (bnd <= coding)
            if (v0 != 0 || v1 != coding) {
                sx = 0; sxx = 0;
#pragma unroll UNR
                for (int i = 0; i < NV; ++i) {
                    if ((uint32_t)i >= t_lo && (uint32_t)i < t_hi) { const uint32_t x = K3_VAL(i); sx += x; sxx += (unsigned long long)x * x; }
                }
                block_sum2(sx, sxx);
            }
            const double mean = (double)sx / (double)n;
            double sd;
            if (exact) sd = k3_sd_exact(n, sx, sxx);
            else {
                double q = 0.0;
#pragma unroll UNR
                for (int i = 0; i < NV; ++i) {
                    if ((uint32_t)i >= t_lo && (uint32_t)i < t_hi) { const double d = (double)K3_VAL(i) - mean; q += d * d; }
                }
                sd = sqrt(block_sum_f64(q, S) / (double)n);
            }
            if (tid == 0) { A.g_valid[gene] = 1; A.g_mean[gene] = mean; A.g_std[gene] = sd; A.g_cv[gene] = sd / mean; }
        } else if (tid == 0) { A.g_valid[gene] = 0; A.g_mean[gene] = 0.0; A.g_std[gene] = 0.0; A.g_cv[gene] = 0.0; }
    }
#undef K3_POS
#undef K3_R
#undef K3_VALID
#undef K3_VAL
    RSQC_FIN_STAMP(8);
    RSQC_K3_PROF_PUBLISH;
    return true;
}

template <int T, int WIN, class CovT, int LDSCAP>
__global__ void __launch_bounds__(T)
gene_coverage_kernel(GeneCovArgs A, uint32_t first) {
    __shared__ K3Shared<T, WIN, CovT, LDSCAP> S;
    const int tid = (int)threadIdx.x;
    const int l = lane_id();
    const int wv = tid >> 6;
    const int gene = (int)A.gene_order[first + blockIdx.x];
    if (!A.gene_owned[gene]) return;
    const uint32_t coding = A.gene_coding[gene];
    const uint32_t e0 = A.ge_off[gene], e1 = A.ge_off[gene + 1], n_ex = e1 - e0;
    // Every later pass re-reads the coverage vector; a gene that fits keeps it in LDS (the difference array is
    // read from memory once and never written back: nothing downstream needs it) -- as 32-bit values, or as
    // 16-bit values for the longest genes (160 KB of LDS hold 73 k bases) as long as no base is covered 65 536
    // times or more.  Otherwise the scan runs in place in memory and the passes rely on unrolled, independent loads.
    uint32_t *const D = A.cov + A.gene_cov_off[gene];
    bool in_lds = LDSCAP > 0 && coding <= (uint32_t)LDSCAP;
    auto Cget = [&](uint32_t j) -> uint32_t { return in_lds ? (uint32_t)S.covbuf[j] : D[j]; };
    const uint32_t MASK = A.mask;
    const uint32_t W = (uint32_t)A.bias_window, OFF = (uint32_t)A.bias_offset;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);

    if (A.gene_reads[gene] == 0ull) {
        // never counted: all-zero coverage -> mean 0, std 0, cv NaN; no exon CV; the bias gate reads zeros
        if (tid == 0) {
            if (coding >= A.bias_gene_length) {
                const uint32_t cur = W / 2 < coding ? W / 2 : coding;
                if ((W < cur ? W : cur) == 0) atomicExch(A.error, RSQC_ERR_EMPTY_MEDIAN);
            }
            const bool pushed = MASK ? coding > 2 * (uint64_t)MASK : coding > 0;
            A.g_valid[gene] = pushed ? 1 : 0;
            A.g_mean[gene] = 0.0; A.g_std[gene] = 0.0; A.g_cv[gene] = pushed ? qnan : 0.0;
        }
        return;
    }
#ifdef RSQC_K1_PROF
    if (first == 0 && threadIdx.x == 0) for (int k = 0; k < 12; ++k) s_fin_stamp[k] = 0ull;
#endif
    // a gene that fits its instance: everything from registers and one LDS copy (above); one too deep for a 16-bit cell comes back
    if constexpr (LDSCAP > 0) {
        if (in_lds && coding > 0) {
            if (k3_gene_in_registers<T, WIN, CovT, LDSCAP, K3_IN_REGISTERS<T, LDSCAP>>(A, first, gene, coding, S)) return;
            in_lds = false;                                                 // (uniform)
        }
    }
    // The general path: the gene runs from memory (LDSCAP = 0, a gene longer than its instance's capacity -- the plan's clamps can
    // place one -- or too deep for 16-bit cells), or from LDS in an instance without the register path.
    RSQC_FIN_STAMP(0);
    // (1) difference array -> coverage: block-wide inclusive scan.  A round covers T x 16 bases; wave w of the round takes 1024
    //     consecutive bases as 16 rows of 64 (lane l loads base row * 64 + l: one 256-byte line run per instruction -- 16
    //     consecutive bases per LANE cost the texture addresser 64 separate lines per instruction and made the scan of a long gene
    //     the longest stage of the kernel), scans each row across the lanes and chains the rows; the next round's rows are in flight
    //     while this one is scanned.
    auto scan = [&]() -> bool {                        // returns false when a value does not fit the LDS cell type
        constexpr int PER = 16;
        uint32_t carry = 0, vmax = 0;
        uint32_t v[PER], nx[PER];
        auto load_round = [&](uint32_t base, uint32_t (&o)[PER]) {
            const uint32_t j0 = base + (uint32_t)wv * (64u * PER) + (uint32_t)l;
#pragma unroll
            for (int k = 0; k < PER; ++k) { const uint32_t j = j0 + (uint32_t)k * 64u; o[k] = j < coding ? D[j] : 0u; }
        };
        load_round(0u, v);
        for (uint32_t base = 0; base < coding; base += T * PER) {
            if (base + T * PER < coding) load_round(base + T * PER, nx);
            // rows scanned across the lanes, each row offset by the total of the rows before it
            uint32_t run = 0;
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const uint32_t inc = wave_inclusive_scan_u32(v[k]);
                v[k] = inc + run;
                run += lane_value(inc, 63);
            }
            k3_sync<T>();
            if (l == 0) S.u32b[wv] = run;
            k3_sync<T>();
            uint32_t before = carry, total = 0;
#pragma unroll
            for (int w = 0; w < (T / 64); ++w) { const uint32_t t = S.u32b[w]; if (w < wv) before += t; total += t; }
            const uint32_t j0 = base + (uint32_t)wv * (64u * PER) + (uint32_t)l;
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const uint32_t j = j0 + (uint32_t)k * 64u;
                if (j < coding) {
                    const uint32_t x = v[k] + before;
                    vmax = x > vmax ? x : vmax;
                    if (in_lds) S.covbuf[j] = (CovT)x; else D[j] = x;
                }
            }
            carry += total;
#pragma unroll
            for (int k = 0; k < PER; ++k) v[k] = nx[k];
        }
        if constexpr (sizeof(CovT) < 4) { if (in_lds) return block_max_u32(vmax, S) <= (uint32_t)(CovT)~(CovT)0; }
        return true;
    };
    if (!scan()) { in_lds = false; RSQC_FIN_STAMP(1); scan(); }           // (uniform: block_max_u32 broadcasts) too deep for 16 bits: in memory
    __threadfence_block();
    k3_sync<T>();
    RSQC_FIN_STAMP(2);
#ifdef RSQC_K1_PROF
    if (first == 0 && threadIdx.x == 0) { s_fin_stamp[9] = coding; s_fin_stamp[10] = n_ex; s_fin_stamp[11] = in_lds; }
#endif
    // (2) per-exon CV over transcript positions [MASK, coding-MASK) (src/Metrics.cpp:267-305): one wave per
    //     exon at a time (an exon's bases are contiguous in C): register sums, no shared accumulators.  The rows of the next
    //     64 exons of a wave are gathered by its lanes in one go (exon k of the wave in lane k: two dependent gathers per 64
    //     exons instead of per exon) and handed to the wave one by one.
    {
        const uint64_t lo_t = MASK, hi_t = coding > MASK ? coding - MASK : 0;
        if (hi_t > lo_t) {
            constexpr uint32_t W = (uint32_t)(T / 64);
            const uint32_t gcov = A.gene_cov_off[gene];
            for (uint32_t k0 = (uint32_t)wv; k0 < n_ex; k0 += 64u * W) {
                const uint32_t mine = k0 + (uint32_t)l * W;
                uint32_t r_t0 = 0, r_len = 0, r_id = 0;
                if (mine < n_ex) {
                    const uint32_t row = A.ge_row[e0 + mine];
                    const ExonRow er = A.ex[row];
                    r_t0 = er.cov - gcov; r_len = (uint32_t)(er.end - er.start + 1); r_id = A.ex_id[row];
                }
                const uint32_t left = (n_ex - k0 + W - 1) / W;
                const uint32_t cnt = left < 64u ? left : 64u;
                for (uint32_t i = 0; i < cnt; ++i) {
                    const uint32_t t0 = lane_value(r_t0, (int)i), len = lane_value(r_len, (int)i), id = lane_value(r_id, (int)i);
                    const uint64_t a0 = t0 > lo_t ? t0 : lo_t, b0 = (uint64_t)t0 + len < hi_t ? (uint64_t)t0 + len : hi_t;
                    if (b0 > a0) {
                        const double size = (double)(b0 - a0);
                        unsigned long long sm = 0;
#pragma unroll 4
                        for (uint32_t j = (uint32_t)a0 + (uint32_t)l; j < b0; j += 64) sm += Cget(j);
                        const double mean = (double)wave_sum(sm) / size;
                        double q = 0.0;
#pragma unroll 4
                        for (uint32_t j = (uint32_t)a0 + (uint32_t)l; j < b0; j += 64) { const double d = (double)Cget(j) - mean; q += d * d; }
                        const double cv = sqrt(wave_sum(q) / size) / mean;
                        if (l == 0 && !(isnan(cv) || isinf(cv))) { A.e_cv[id] = cv; A.e_cv_valid[id] = 1; }
                    }
                }
            }
        }
    }
#ifdef RSQC_K1_PROF
    k3_sync<T>();
    RSQC_FIN_STAMP(3);
#endif
    // (3) bias (src/Metrics.cpp:160-235) on the stitched, unmasked coverage vector [0, coding)
    uint32_t v0 = 0, v1 = coding;          // the (possibly trimmed) vector the gene stats use (Q14)
    if (coding >= A.bias_gene_length) {
        uint32_t best = 0, best_i = 0xFFFFFFFFu;
        unsigned long long nz = 0;
#pragma unroll 8
        for (uint32_t j = tid; j < coding; j += T) { const uint32_t v = Cget(j); nz += v != 0u; if (v > best) { best = v; best_i = j; } }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t ob = __shfl_xor(best, o, 64), oi = __shfl_xor(best_i, o, 64);
            if (ob > best || (ob == best && oi < best_i)) { best = ob; best_i = oi; }
        }
        k3_sync<T>();
        if (l == 0) { S.u32a[wv] = best; S.u32b[wv] = best_i; }
        k3_sync<T>();
        best = 0; best_i = 0xFFFFFFFFu;
#pragma unroll
        for (int w = 0; w < (T / 64); ++w) { const uint32_t ob = S.u32a[w], oi = S.u32b[w]; if (ob > best || (ob == best && oi < best_i)) { best = ob; best_i = oi; } }
        const uint32_t pp = best == 0 ? 0u : best_i;
        uint32_t cur = pp + W / 2 < coding ? pp + W / 2 : coding;
        const uint32_t n = W < cur ? W : cur;
        cur -= n;
        double gate = 0.0;
        if (n == 0) { if (tid == 0) atomicExch(A.error, RSQC_ERR_EMPTY_MEDIAN); }
        else if (n == 1) gate = (double)Cget(cur);
        else {
            const uint32_t mid = (n - 1) / 2;
            gate = (n & 1u) ? ((double)Cget(cur + mid) + (double)Cget(cur + mid + 1)) / 2.0 : (double)Cget(cur + mid);
        }
        RSQC_FIN_STAMP(4);
        if (n != 0 && gate >= 100.0) {
            // 5th percentile of the non-zero coverage = order statistic R of the whole vector
            const uint32_t nnz = (uint32_t)block_sum_u64(nz, S);
            uint32_t R = (coding - nnz) + (uint32_t)((double)nnz * 0.05);
            uint32_t prefix = 0, pmask = 0;
            // MSB-first radix select; bytes above the top non-zero byte of the maximum are zero for every entry
            const int top = best >> 24 ? 24 : best >> 16 ? 16 : best >> 8 ? 8 : 0;
            pmask = top == 24 ? 0u : 0xFFFFFFFFu << (top + 8);
            for (int shift = top; shift >= 0; shift -= 8) {
                k3_sync<T>();
                for (int h = tid; h < 256; h += T) S.hist[h] = 0;
                k3_sync<T>();
#pragma unroll 8
                for (uint32_t j = tid; j < coding; j += T) {            // (same-bin LDS atomics of a wave serialise inside ONE
                    const uint32_t v = Cget(j);                            //  instruction, ~1 cycle per lane: cheaper than merging them)
                    if ((v & pmask) == prefix) atomicAdd(&S.hist[(v >> shift) & 0xFF], 1u);
                }
                k3_sync<T>();
                if (wv == 0) {                                       // wave 0: lane x scans 4 bins
                    const uint32_t h0 = S.hist[4 * l], h1 = S.hist[4 * l + 1], h2 = S.hist[4 * l + 2], h3 = S.hist[4 * l + 3];
                    const uint32_t tot = h0 + h1 + h2 + h3;
                    const uint32_t inc = wave_inclusive_scan_u32(tot);
                    const uint32_t exc = inc - tot;
                    if (R >= exc && R < inc) {
                        uint32_t digit, rbase;
                        if (R < exc + h0) { digit = 4 * l; rbase = exc; }
                        else if (R < exc + h0 + h1) { digit = 4 * l + 1; rbase = exc + h0; }
                        else if (R < exc + h0 + h1 + h2) { digit = 4 * l + 2; rbase = exc + h0 + h1; }
                        else { digit = 4 * l + 3; rbase = exc + h0 + h1 + h2; }
                        S.bc_u32[2] = digit; S.bc_u32[3] = rbase;
                    }
                }
                k3_sync<T>();
                R -= S.bc_u32[3];
                prefix |= S.bc_u32[2] << shift; pmask |= 0xFFu << shift;
            }
            const uint32_t lower = prefix;
            RSQC_FIN_STAMP(5);
            // trim leading / trailing entries <= lower (in place in the reference: Q14)
            uint32_t first_gt = 0xFFFFFFFFu, last_gt = 0;
#pragma unroll 8
            for (uint32_t j = tid; j < coding; j += T) if (Cget(j) > lower) { if (first_gt == 0xFFFFFFFFu) first_gt = j; last_gt = j + 1; }
            first_gt = block_min_u32(first_gt, S);
            last_gt = block_max_u32(last_gt, S);
            if (first_gt == 0xFFFFFFFFu) { v0 = coding; v1 = coding; } else { v0 = first_gt; v1 = last_gt; }
            const uint32_t tlen = v1 - v0;
            RSQC_FIN_STAMP(6);
            if (tlen >= A.bias_gene_length) {
                // left window [OFF, min(OFF+W, tlen)), right window [tlen-W-OFF, tlen-OFF)
                const uint32_t lhi = OFF + W < tlen ? OFF + W : tlen;
                const uint32_t nl = OFF < lhi ? lhi - OFF : 0u;
                uint32_t nr = 0, rlo = 0;
                if ((uint64_t)W + OFF <= tlen) { rlo = tlen - W - OFF; nr = W; }
                k3_sync<T>();
                for (uint32_t j = tid; j < nl; j += T) S.win[0][j] = Cget(v0 + OFF + j);
                for (uint32_t j = tid; j < nr; j += T) S.win[1][j] = Cget(v0 + rlo + j);
                k3_sync<T>();
                double ml = 0.0, mr = 0.0;
                const bool okl = window_median(S.win[0], nl, &ml, S);
                const bool okr = window_median(S.win[1], nr, &mr, S);
                if (!(okl && okr)) { if (tid == 0) atomicExch(A.error, RSQC_ERR_EMPTY_MEDIAN); }
                else if (tid == 0) {
                    const bool fwd = (A.gene_flags[gene] & RSQC_FF_STRAND_MASK) == RSQC_STRAND_FORWARD;
                    A.bias3[gene] = (unsigned long long)(fwd ? mr : ml);      // unsigned long += double: truncation
                    A.bias5[gene] = (unsigned long long)(fwd ? ml : mr);
                }
            }
        }
    }
    RSQC_FIN_STAMP(7);
    // (4) gene mean / std / CV on positions [v0, v1) with MASK bases removed at both ends
    {
        const uint32_t len = v1 - v0;
        uint32_t a = v0, bnd = v1;
        if (MASK) {
            if (len > 2 * (uint64_t)MASK) { a = v0 + MASK; bnd = v1 - MASK; } else { a = bnd = v0; }
        }
        if (bnd > a) {
            const double size = (double)(bnd - a);
            unsigned long long sm = 0;
#pragma unroll 8
            for (uint32_t j = a + tid; j < bnd; j += T) sm += Cget(j);
            const double mean = (double)block_sum_u64(sm, S) / size;
            double q = 0.0;
#pragma unroll 8
            for (uint32_t j = a + tid; j < bnd; j += T) { const double d = (double)Cget(j) - mean; q += d * d; }
            const double sd = sqrt(block_sum_f64(q, S) / size);
            if (tid == 0) { A.g_valid[gene] = 1; A.g_mean[gene] = mean; A.g_std[gene] = sd; A.g_cv[gene] = sd / mean; }
        } else if (tid == 0) { A.g_valid[gene] = 0; A.g_mean[gene] = 0.0; A.g_std[gene] = 0.0; A.g_cv[gene] = 0.0; }
    }
    RSQC_FIN_STAMP(8);
#ifdef RSQC_K1_PROF
    if (first == 0 && threadIdx.x == 0) {
        const unsigned long long tot = s_fin_stamp[8] - s_fin_stamp[0];
        if (atomicMax(&g_fin_prof[31], tot) < tot) {
            for (int k = 0; k < 9; ++k) g_fin_prof[k] = s_fin_stamp[k];
            g_fin_prof[28] = s_fin_stamp[9]; g_fin_prof[29] = s_fin_stamp[10]; g_fin_prof[30] = s_fin_stamp[11]; g_fin_prof[27] = blockIdx.x;
        }
    }
#endif
}

}  // namespace rsqc
