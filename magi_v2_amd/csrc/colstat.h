// What the per-column statistics units share (summary.hip, elpd.hip): one 256-thread workgroup per column of C R draws gathered to
// chunk[column][C R]; the fixed-order reductions over that workgroup; the order-preserving key of a double and the radix select on it;
// the limits of C and R.  Every sum runs in one fixed order (lane-strided partials, a butterfly, the four waves added as
// (w0 + w1) + (w2 + w3)) and the only atomics are integer ones: results are bit-identical from run to run.
#pragma once
#include "scratch.h"

#include <algorithm>
#include <cmath>
#include <string>

namespace colstat {

constexpr int SUM_WG = 256;
constexpr int G_TILE = 64;            // the gathers: 64 x 64 doubles per workgroup of 64 x 4 threads
constexpr int SUM_LDS = 2048;         // doubles of LDS a statistics kernel sorts / stages (16 KiB: four workgroups per CU and more)
constexpr size_t CHUNK_DOUBLES = (size_t)1 << 23;

constexpr int MAX_Q = 16;

struct SumLB { double v[MAGI_MAX_D]; };
struct SumProbs { double p[MAX_Q]; };

// how a block's columns are read and reported: as they are, or a sample row's X, sigma or theta block on its natural scale
enum { MODE_PLAIN = 0, MODE_X = 1, MODE_SIGMA = 2, MODE_THETA = 3 };

// the reductions over the workgroup, each in one fixed order; every thread receives the result
__device__ __forceinline__ double wg_sum(double v, double* red /* LDS [4] */) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    __syncthreads();                                           // (the previous use of red is over)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ double wg_min(double v, double* red) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
}
// (the butterfly: not the DPP wave_sum of magi_internal.h, whose order differs)
__device__ __forceinline__ double wave_bsum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// where column j of a block goes in the caller's arrays: the X block is walked in the samples' order [D][N] and reported in the host
// layout [N][D]
__device__ __forceinline__ long long out_index(int mode, long long j, int N, int D) {
    return mode == MODE_X ? (j % N) * (long long)D + j / N : j;
}

// order-preserving key of a finite double and its inverse
__device__ __forceinline__ unsigned long long to_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
__device__ __forceinline__ double from_key(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? k ^ 0x8000000000000000ull : ~k;
    return __longlong_as_double((long long)b);
}

// key of rank `rank` (0-based) among the S keys key_of(0 .. S - 1), `bits` wide (a multiple of 8); every thread returns it
template <class KeyOf>
__device__ __forceinline__ unsigned long long radix_select_keys(KeyOf key_of, int S, int rank, int bits, int* hist /* LDS [256] */) {
    unsigned long long prefix = 0, mask = 0;
    for (int shift = bits - 8; shift >= 0; shift -= 8) {
        hist[threadIdx.x] = 0;                                 // (SUM_WG == 256 bins)
        __syncthreads();
        for (int e = threadIdx.x; e < S; e += SUM_WG) {
            const unsigned long long key = key_of(e);
            if ((key & mask) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255)], 1);
        }
        __syncthreads();
        int cum = 0, b = 0;
        for (; b < 255; ++b) {                                 // (the rank lies in one of the bins: b stops at 255 at the latest)
            const int c = hist[b];
            if (cum + c > rank) break;
            cum += c;
        }
        rank -= cum;
        prefix |= (unsigned long long)b << shift;
        mask |= 0xFFull << shift;
        __syncthreads();                                       // (every thread has read hist before it is cleared again)
    }
    return prefix;
}

// key of the order statistic of rank `rank` (0-based) among the S finite values of row; every thread returns it
__device__ inline unsigned long long radix_select(const double* __restrict__ row, int S, int rank, int* hist /* LDS [256] */) {
    return radix_select_keys([row](int e) { return to_key(row[e]); }, S, rank, 64, hist);
}

// the limits of a column's draws the entry points share
inline int check_draws(magi_handle* h, const char* who, long long C, long long R) {
    if (C < 1 || C > 4096) return magi_fail(h, MAGI_E_BADARG, std::string(who) + ": 1 <= C <= 4096 chains");
    if (R < 1 || R > (1 << 20)) return magi_fail(h, MAGI_E_BADARG, std::string(who) + ": 1 <= R <= 2^20 draws per chain");
    if (C * R > (1 << 22)) return magi_fail(h, MAGI_E_BADARG, std::string(who) + ": C R exceeds 2^22 draws per column");
    return MAGI_OK;
}

// the quantile probabilities every summarising entry point takes; fills pr
inline int check_probs(magi_handle* h, const char* who, int n_q, const double* probs, SumProbs& pr) {
    if (n_q < 0 || n_q > MAX_Q) return magi_fail(h, MAGI_E_BADARG, std::string(who) + ": 0 <= n_q <= 16 probabilities");
    if (n_q > 0 && !probs) return magi_fail(h, MAGI_E_BADARG, std::string(who) + ": probs is NULL");
    for (int q = 0; q < MAX_Q; ++q) pr.p[q] = 0.0;
    for (int q = 0; q < n_q; ++q) {
        if (!std::isfinite(probs[q]) || probs[q] < 0.0 || probs[q] > 1.0)
            return magi_fail(h, MAGI_E_BADARG, std::string(who) + ": probs[" + std::to_string(q) + "] is not a finite number in [0, 1]");
        pr.p[q] = probs[q];
    }
    return MAGI_OK;
}

// columns per chunk of a block of K columns of S draws (at most 2^23 doubles; the test switch summary_chunk_cols forces small chunks)
inline size_t chunk_cols(const magi_handle* h, size_t S, size_t K) {
    size_t cc = std::max<size_t>(1, CHUNK_DOUBLES / S);
    cc = std::min<size_t>({cc, K, (size_t)1 << 21});                     // (the gathers: at most 2^15 tiles along grid.y)
    if (h->opt.summary_chunk_cols > 0) cc = std::min<size_t>(cc, (size_t)h->opt.summary_chunk_cols);
    return cc;
}

}  // namespace colstat

// summary.hip: the statistics of magi_summarize for K columns of C x R draws on the device in chunk layout (chunk[column][C R], what
// k_sum_gather produces and what gp.hip's GEMM writes).  take: declares the result arrays in the caller's scratch (before its alloc());
// chunk: k_sum_moments / k_sum_ess / k_sum_order on columns [k0, k0 + nc), reported at out_index(mode, column, N, D); down: queues the
// downloads the caller wants (null: not) and that of the count of columns with a non-finite draw, to be read after s.finish().
struct MagiColStats {
    int C, R, n_q, max_lag, max_cols;
    long long K;
    bool want_ess, want_q;
    colstat::SumProbs probs;
    double *yb, *col, *mean, *sd, *rhat, *ess, *mcse, *quant;
    int* count;
    int n_bad;                        // the downloaded count
};
void magi_colstats_take(MagiScratch& s, MagiColStats& st, int C, int R, long long K, int max_cols, int n_q, const colstat::SumProbs& probs, int max_lag,
                        bool want_ess, bool want_quant);
int magi_colstats_chunk(magi_handle* h, const char* who, const MagiColStats& st, const double* dchunk, int nc, long long k0, int mode, int N, int D);
void magi_colstats_down(MagiScratch& s, MagiColStats& st, double* mean, double* sd, double* quant, double* rhat, double* ess, double* mcse);
// summary.hip: k_sum_gather on nc columns of S rows (column j of row r at src[r ld + j]) -> chunk[nc][S], on the natural scale of `mode`
// (lb0: the block's first column in lb / tsup / prior), for the units that work on the same chunks (rank.hip)
int magi_sum_gather(magi_handle* h, int S, int nc, const double* src, long long ld, int mode, int lb0, const colstat::SumLB& lb, const double2* tsup,
                    const double4* prior, double* chunk);
