// Posterior summaries and convergence diagnostics (magi_summarize, magi_sampler_summarize): per scalar column of C chains x R draws the
// pooled mean, sd (ddof 1) and quantiles (exact order statistics, linear interpolation), split R-hat, ESS (Geyer's initial monotone
// sequence over the split chains' autocovariances) and the Monte-Carlo standard error of the mean -- definitions in include/magi_hip.h and DESIGN.md 4.4.
// A sample row is [D][N] | sig_pre[D] | th_pre[P] | pad: the draws of one column lie dimp doubles apart.  So
//   k_sum_gather    tiled gather + transpose through an LDS tile (as k_transpose): rows x columns of the source -> chunk[column][C R],
//                   the natural-scale transform (softplus_ref + LB for sigma, the parameter's support for theta) applied on the way.  Columns go in chunks of at most 2^23
//                   doubles (64 MiB; the host route stages its strided upload in a second buffer of that size).
//   k_sum_moments   one workgroup per column: non-finite / constant detection, mean, sd (two passes), then one WAVE per split chain for
//                   its mean and variance (no barrier inside), W, B/n, var+, R-hat.
//   k_sum_ess       one workgroup per column: the lag loop, two lags (one pair P_k) per pass over the centred series -- staged in LDS
//                   when the M n doubles fit, read from the chunk otherwise -- and it stops at the first negative pair.
//   k_sum_order     one workgroup per column: exact order statistics.  C R <= SUM_LDS: bitonic sort in LDS.  Larger: radix select (8 passes
//                   of 8 bits, LDS histogram) on the order-preserving 64-bit key, then one pass for the next-larger order statistic.
// Every sum runs in one fixed order (lane-strided partials, a butterfly, the four waves added as (w0 + w1) + (w2 + w3)); the only atomics
// are integer ones: the results are bit-identical from run to run.  Does not depend on the drift (jit._DRIFT_FREE).
// Also the home of what the trajectory calls need that does not depend on the drift either (ode.hip, ode_adaptive.hip and gp.hip launch them
// through magi_ode_stats, magi_ode_transpose, magi_transpose), so that a traced drift's library reuses this unit's object:
//   k_ode_stats     mean and sample standard deviation per (j, d) over the draws with status 0: two passes, lane-strided partial sums,
//                   then a butterfly -- one fixed summation order, bit-identical from run to run.
//   k_transpose     in[rows][ld_in] -> out[cols][ld_out] through an LDS tile, guarded on both sides: trj[T D][S_pad] -> the host layout
//                   [S][T D], and gp.hip's chunk[(m, d)][S] -> [S][(m, d)].
// and of magi_finished_chains, the chain range of a finished sampler that magi_sampler_summarize / _elpd / _gp_predict work on.
#include "colstat.h"

#include <cmath>
#include <vector>

namespace {

using namespace colstat;              // SUM_WG, G_TILE, SUM_LDS, the workgroup reductions, to_key / radix_select, the MODE_*, check_draws / check_probs

__global__ __launch_bounds__(G_TILE * 4) void k_sum_gather(int S, int nc, const double* __restrict__ src /* rows ld apart, nc columns */,
                                                           long long ld, int mode, int lb0, SumLB lb, const double2* __restrict__ tsup /* MODE_THETA: the parameters' supports, or null */,
                                                           const double4* __restrict__ prior /* MODE_SIGMA: the prior table (a fixed sigma^2 reports its constant), or null */,
                                                           double* __restrict__ chunk /* [nc][S] */) {
    __shared__ double tile[G_TILE][G_TILE + 1];               // (+1: the column reads below fall on 32 different bank pairs)
    const int r0 = blockIdx.x * G_TILE, c0 = blockIdx.y * G_TILE, tx = threadIdx.x, ty = threadIdx.y;
    for (int r = ty; r < G_TILE; r += 4)
        if (r0 + r < S && c0 + tx < nc) {
            double v = src[(size_t)(r0 + r) * (size_t)ld + c0 + tx];
            if (mode == MODE_SIGMA) {
                v = softplus_ref(v) + lb.v[lb0 + c0 + tx];                              // (lb0 + nc <= D: the sigma block has D columns)
                if (prior) { const double4 pe = prior[lb0 + c0 + tx]; if (Prior::fixed(pe)) v = pe.y; }
            }
            else if (mode == MODE_THETA) v = ThetaSup::theta(tsup != nullptr, ThetaSup::load(tsup, lb0 + c0 + tx), v, softplus_ref(v));      // (lb0 + nc <= P)
            tile[r][tx] = v;
        }
    __syncthreads();
    for (int c = ty; c < G_TILE; c += 4)
        if (c0 + c < nc && r0 + tx < S) chunk[(size_t)(c0 + c) * S + r0 + tx] = tile[tx][c];
}

// first row of split chain m in a column of C chains x R draws (n = R / 2: an odd R drops the middle draw)
__device__ __forceinline__ int split_start(int m, int R, int n) { return (m >> 1) * R + ((m & 1) ? R - n : 0); }

// per chunk column: col[4] = { W, var+, sd, flag } with flag 0: diagnostics defined, 1: a non-finite draw, 2: constant column or R < 4
__global__ __launch_bounds__(SUM_WG) void k_sum_moments(int C, int R, const double* __restrict__ chunk, double* __restrict__ ybar /* [nc][2 C] */,
                                                        double* __restrict__ col /* [nc][4] */, long long k0, int mode, int N, int D,
                                                        double* __restrict__ mean, double* __restrict__ sd, double* __restrict__ rhat,
                                                        int* __restrict__ n_nonfinite) {
    __shared__ double red[SUM_WG / 64];
    const int S = C * R, tid = threadIdx.x;
    const double* row = chunk + (size_t)blockIdx.x * S;
    double* cl = col + (size_t)blockIdx.x * 4;
    const long long o = out_index(mode, k0 + blockIdx.x, N, D);
    const double nan = __builtin_nan("");
    double s = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
    int bad = 0;
    for (int e = tid; e < S; e += SUM_WG) {
        const double v = row[e];
        bad |= !isfinite(v);
        s += v;
        mn = fmin(mn, v);
        mx = fmax(mx, v);
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0) {
            mean[o] = nan; sd[o] = nan; rhat[o] = nan;
            cl[0] = nan; cl[1] = nan; cl[2] = nan; cl[3] = 1.0;
            atomicAdd(n_nonfinite, 1);
        }
        return;
    }
    s = wg_sum(s, red);
    mn = wg_min(mn, red);
    mx = -wg_min(-mx, red);
    const double mu = s / (double)S;
    double ss = 0.0;
    for (int e = tid; e < S; e += SUM_WG) {
        const double dv = row[e] - mu;
        ss += dv * dv;
    }
    ss = wg_sum(ss, red);
    const bool constant = mn == mx;
    const double sdv = S < 2 ? nan : constant ? 0.0 : sqrt(ss / (double)(S - 1));
    if (R < 4 || constant) {
        if (tid == 0) {
            mean[o] = mu; sd[o] = sdv; rhat[o] = nan;
            cl[0] = nan; cl[1] = nan; cl[2] = sdv; cl[3] = 2.0;
        }
        return;
    }
    // split chains: wave w takes m = w, w + 4, ...; its lanes stride over the n draws
    const int n = R / 2, M = 2 * C, w = tid >> 6, lane = tid & 63;
    double* yb = ybar + (size_t)blockIdx.x * M;
    double wacc = 0.0;
    for (int m = w; m < M; m += SUM_WG / 64) {
        const double* y = row + split_start(m, R, n);
        double a = 0.0;
        for (int i = lane; i < n; i += 64) a += y[i];
        const double ym = wave_bsum(a) / (double)n;
        double q = 0.0;
        for (int i = lane; i < n; i += 64) {
            const double dv = y[i] - ym;
            q += dv * dv;
        }
        wacc += wave_bsum(q) / (double)(n - 1);
        if (lane == 0) yb[m] = ym;
    }
    __syncthreads();                                           // (yb is read below by other waves of this workgroup)
    if (lane == 0) red[w] = wacc;
    __syncthreads();
    const double W = ((red[0] + red[1]) + (red[2] + red[3])) / (double)M;
    double a = 0.0;
    for (int m = tid; m < M; m += SUM_WG) a += yb[m];
    const double ymean = wg_sum(a, red) / (double)M;
    double q = 0.0;
    for (int m = tid; m < M; m += SUM_WG) {
        const double dv = yb[m] - ymean;
        q += dv * dv;
    }
    const double Bn = wg_sum(q, red) / (double)(M - 1);
    const double varp = (double)(n - 1) / (double)n * W + Bn;
    if (tid == 0) {
        mean[o] = mu; sd[o] = sdv; rhat[o] = sqrt(varp / W);
        cl[0] = W; cl[1] = varp; cl[2] = sdv; cl[3] = 0.0;
    }
}

template <bool LDS>
__device__ __forceinline__ double centred(const double* z, const double* row, const double* yb, int m, int i, int R, int n) {
    return LDS ? z[m * n + i] : row[split_start(m, R, n) + i] - yb[m];
}

// sum over the split chains of sum_i z_i z_(i+t) for t = t0 (skipped when 0) and t0 + 1
template <bool LDS>
__device__ __forceinline__ void lag_pair(const double* z, const double* row, const double* yb, int R, int n, int total, int t0, double& a0, double& a1) {
    a0 = 0.0; a1 = 0.0;
    for (int e = threadIdx.x; e < total; e += SUM_WG) {
        const int m = e / n, i = e - m * n;
        if (i + t0 + 1 < n || (t0 > 0 && i + t0 < n)) {
            const double zi = centred<LDS>(z, row, yb, m, i, R, n);
            if (t0 > 0 && i + t0 < n) a0 += zi * centred<LDS>(z, row, yb, m, i + t0, R, n);
            if (i + t0 + 1 < n) a1 += zi * centred<LDS>(z, row, yb, m, i + t0 + 1, R, n);
        }
    }
}

__global__ __launch_bounds__(SUM_WG) void k_sum_ess(int C, int R, int max_lag, const double* __restrict__ chunk, const double* __restrict__ ybar,
                                                    const double* __restrict__ col, long long k0, int mode, int N, int D,
                                                    double* __restrict__ ess, double* __restrict__ mcse) {
    __shared__ double z[SUM_LDS];
    __shared__ double red[SUM_WG / 64];
    const int S = C * R, tid = threadIdx.x;
    const double* row = chunk + (size_t)blockIdx.x * S;
    const double* cl = col + (size_t)blockIdx.x * 4;
    const long long o = out_index(mode, k0 + blockIdx.x, N, D);
    if (cl[3] != 0.0) {                                        // (uniform over the workgroup)
        if (tid == 0) { ess[o] = __builtin_nan(""); mcse[o] = __builtin_nan(""); }
        return;
    }
    const int n = R / 2, M = 2 * C, total = M * n;             // (total <= C R <= 2^22)
    const double* yb = ybar + (size_t)blockIdx.x * M;
    const double W = cl[0], varp = cl[1], sdv = cl[2], Mn = (double)total;
    const bool lds = total <= SUM_LDS;
    if (lds) {
        for (int e = tid; e < total; e += SUM_WG) {
            const int m = e / n, i = e - m * n;
            z[e] = row[split_start(m, R, n) + i] - yb[m];
        }
        __syncthreads();
    }
    const int L = (max_lag <= 0 || max_lag > n - 1) ? n - 1 : max_lag;
    const int pairs = (L + 1) / 2;                             // the k with 2 k + 1 <= L
    double sum = 0.0, prev = 0.0;
    for (int k = 0; k < pairs; ++k) {
        double a0, a1;
        if (lds) lag_pair<true>(z, row, yb, R, n, total, 2 * k, a0, a1);
        else lag_pair<false>(z, row, yb, R, n, total, 2 * k, a0, a1);
        a0 = wg_sum(a0, red);
        a1 = wg_sum(a1, red);
        const double rho0 = k == 0 ? 1.0 : 1.0 - (W - a0 / Mn) / varp;
        const double rho1 = 1.0 - (W - a1 / Mn) / varp;
        const double P = rho0 + rho1;
        if (P < 0.0) break;                                    // K* = k (every thread holds the same P)
        prev = k == 0 ? P : fmin(P, prev);
        sum += prev;
    }
    if (tid == 0) {
        const double tau = fmax(-1.0 + 2.0 * sum, 1.0 / log10(Mn));
        const double e = Mn / tau;
        ess[o] = e;
        mcse[o] = sdv / sqrt(e);
    }
}

__global__ __launch_bounds__(SUM_WG) void k_sum_order(int S, const double* __restrict__ chunk, const double* __restrict__ col, long long k0,
                                                      int mode, int N, int D, long long K, int n_q, SumProbs probs,
                                                      double* __restrict__ quant /* [n_q][K] */) {
    static_assert(SUM_WG == 256, "one thread per histogram bin");
    __shared__ double v[SUM_LDS];
    __shared__ int hist[256];
    __shared__ unsigned long long s_above;
    __shared__ int s_le;
    const int tid = threadIdx.x;
    const double* row = chunk + (size_t)blockIdx.x * S;
    const long long o = out_index(mode, k0 + blockIdx.x, N, D);
    if (col[(size_t)blockIdx.x * 4 + 3] == 1.0) {              // a non-finite draw (uniform over the workgroup)
        if (tid < n_q) quant[(size_t)tid * K + o] = __builtin_nan("");
        return;
    }
    const bool sorted = S <= SUM_LDS;
    if (sorted) {
        int n2 = 1;
        while (n2 < S) n2 <<= 1;
        for (int i = tid; i < n2; i += SUM_WG) v[i] = i < S ? row[i] : __builtin_inf();
        __syncthreads();
        for (int k = 2; k <= n2; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < n2; i += SUM_WG) {
                    const int p = i ^ j;
                    if (p > i) {
                        const double a = v[i], b = v[p];
                        // (the order of the keys, as the radix path: -0.0 sorts before +0.0 whatever C R is; the padding is the largest key)
                        if ((to_key(a) > to_key(b)) == ((i & k) == 0)) { v[i] = b; v[p] = a; }
                    }
                }
                __syncthreads();
            }
    }
    for (int q = 0; q < n_q; ++q) {
        const double hq = (double)(S - 1) * probs.p[q];
        int lo = (int)floor(hq);
        lo = lo < 0 ? 0 : lo > S - 1 ? S - 1 : lo;             // (0 <= p <= 1 keeps it there; this keeps every index in bounds regardless)
        const double g = hq - (double)lo;
        const int hi = lo + 1 < S ? lo + 1 : S - 1;
        double vlo, vhi;
        if (sorted) {
            vlo = v[lo];
            vhi = v[hi];
        } else {
            const unsigned long long klo = radix_select(row, S, lo, hist);
            vlo = from_key(klo);
            vhi = vlo;
            if (hi != lo) {
                // the next order statistic: v[lo] again when more than lo + 1 values are <= it, else the smallest value above it
                if (tid == 0) { s_le = 0; s_above = ~0ull; }
                __syncthreads();
                int le = 0;
                unsigned long long above = ~0ull;
                for (int e = tid; e < S; e += SUM_WG) {
                    const unsigned long long key = to_key(row[e]);
                    if (key <= klo) ++le;
                    else above = key < above ? key : above;
                }
                atomicAdd(&s_le, le);
                atomicMin(&s_above, above);
                __syncthreads();
                if (s_le <= lo + 1) vhi = from_key(s_above);
                __syncthreads();                               // (read before the next quantile resets them)
            }
        }
        // (g = 0: the order statistic itself, also where v[hi] - v[lo] overflows)
        if (tid == 0) quant[(size_t)q * K + o] = g == 0.0 ? vlo : vlo + g * (vhi - vlo);
    }
}

__global__ __launch_bounds__(SUM_WG) void k_ode_stats(int S, int S_pad, const double* __restrict__ trj /* [T D][S_pad] */,
                                                      const int* __restrict__ status /* [S_pad] */, double* __restrict__ mean /* [T D] */,
                                                      double* __restrict__ sd /* [T D] */, int* __restrict__ n_failed) {
    __shared__ double red[SUM_WG / 64];
    const double* row = trj + (size_t)blockIdx.x * S_pad;
    double sum = 0.0, cnt = 0.0;
    for (int s = threadIdx.x; s < S; s += SUM_WG) {
        const bool ok = status[s] == 0;
        sum += ok ? row[s] : 0.0;
        cnt += ok ? 1.0 : 0.0;
    }
    sum = wg_sum(sum, red);
    cnt = wg_sum(cnt, red);                                    // (exact: an integer <= 2^20)
    const double nan = __builtin_nan("");
    const double mu = cnt > 0.0 ? sum / cnt : nan;
    double ss = 0.0;
    for (int s = threadIdx.x; s < S; s += SUM_WG) {
        const double dv = row[s] - mu;
        ss += status[s] == 0 ? dv * dv : 0.0;
    }
    ss = wg_sum(ss, red);
    if (threadIdx.x == 0) {
        mean[blockIdx.x] = mu;
        sd[blockIdx.x] = cnt > 1.0 ? sqrt(ss / (cnt - 1.0)) : nan;
        if (blockIdx.x == 0) *n_failed = S - (int)cnt;
    }
}

// grid (ceil(cols / 64), ceil(rows / 64)), block (64, 4)
__global__ __launch_bounds__(G_TILE * 4) void k_transpose(int rows, int cols, const double* __restrict__ in /* [rows][ld_in] */, size_t ld_in,
                                                          double* __restrict__ out /* [cols][ld_out] */, size_t ld_out) {
    __shared__ double tile[G_TILE][G_TILE + 1];               // (+1: the column reads below fall on 32 different bank pairs)
    const int r0 = blockIdx.y * G_TILE, c0 = blockIdx.x * G_TILE, tx = threadIdx.x, ty = threadIdx.y;
    for (int r = ty; r < G_TILE; r += 4)
        if (r0 + r < rows && c0 + tx < cols) tile[r][tx] = in[(size_t)(r0 + r) * ld_in + c0 + tx];
    __syncthreads();
    for (int c = ty; c < G_TILE; c += 4)
        if (c0 + c < cols && r0 + tx < rows) out[(size_t)(c0 + c) * ld_out + r0 + tx] = tile[tx][c];
}

struct SumOut { double *mean, *sd, *quant, *rhat, *ess, *mcse; };

// one block of K columns of C x R draws: from the device (dsrc: column j of row r at dsrc[r ld + j]) or from the host (hsrc [C R][K]).
// Adds the block's columns with a non-finite draw to *nonfinite.  Scratch: the chunk, the staging of the host route's strided upload,
// and the statistics' arrays.
int summarize_block(magi_handle* h, const char* who, const double* dsrc, const double* hsrc, long long ld, int C, int R, long long K, int mode,
                    int N, int D, const SumLB& lb, const double2* tsup, const double4* prior, int n_q, const SumProbs& probs, int max_lag, const SumOut& o, int* nonfinite) {
    const size_t S = (size_t)C * R;
    const size_t cc = chunk_cols(h, S, (size_t)K);
    MagiScratch s(h, who);
    MagiColStats st;
    double *chunk, *stage;
    s.take(chunk, cc * S);
    s.take(stage, hsrc ? cc * S : 0);
    magi_colstats_take(s, st, C, R, K, (int)cc, n_q, probs, max_lag, o.ess || o.mcse, o.quant != nullptr);
    if (int rc = s.alloc()) return rc;
    for (size_t c0 = 0; c0 < (size_t)K && s.ok(); c0 += cc) {
        const int nc = (int)std::min(cc, (size_t)K - c0);
        const double* src = dsrc ? dsrc + c0 : stage;
        const long long sld = dsrc ? ld : nc;
        if (hsrc)
            s.note(hipMemcpy2DAsync(stage, (size_t)nc * sizeof(double), hsrc + c0, (size_t)K * sizeof(double), (size_t)nc * sizeof(double), S,
                                    hipMemcpyHostToDevice, h->stream));
        if (s.ok()) s.note(magi_sum_gather(h, (int)S, nc, src, sld, mode, (int)c0, lb, tsup, prior, chunk));
        if (s.ok()) s.note(magi_colstats_chunk(h, who, st, chunk, nc, (long long)c0, mode, N, D));
    }
    magi_colstats_down(s, st, o.mean, o.sd, o.quant, o.rhat, o.ess, o.mcse);
    if (int rc = s.finish()) return rc;
    if (nonfinite) *nonfinite += st.n_bad;
    return MAGI_OK;
}

}  // namespace

int magi_ode_stats(magi_handle* h, int S, int S_pad, int R, const double* trj, const int* status, double* mean, double* sd, int* n_failed) {
    return magi_launch(h, "k_ode_stats: ", k_ode_stats, dim3((unsigned)R), dim3(SUM_WG), h->stream, S, S_pad, trj, status, mean, sd, n_failed);
}

int magi_transpose(magi_handle* h, int rows, int cols, const double* in, size_t ld_in, double* out, size_t ld_out) {
    return magi_launch(h, "k_transpose: ", k_transpose, dim3((unsigned)((cols + G_TILE - 1) / G_TILE), (unsigned)((rows + G_TILE - 1) / G_TILE)), dim3(G_TILE, 4),
                       h->stream, rows, cols, in, ld_in, out, ld_out);
}

int magi_sum_gather(magi_handle* h, int S, int nc, const double* src, long long ld, int mode, int lb0, const SumLB& lb, const double2* tsup,
                    const double4* prior, double* chunk) {
    return magi_launch(h, "k_sum_gather: ", k_sum_gather, dim3((unsigned)((S + G_TILE - 1) / G_TILE), (unsigned)((nc + G_TILE - 1) / G_TILE)), dim3(G_TILE, 4),
                       h->stream, S, nc, src, ld, mode, lb0, lb, tsup, prior, chunk);
}

int magi_ode_transpose(magi_handle* h, int S, int S_pad, int R, const double* trj, double* out) {
    return magi_transpose(h, R, S, trj, (size_t)S_pad, out, (size_t)R);
}

void magi_colstats_take(MagiScratch& s, MagiColStats& st, int C, int R, long long K, int max_cols, int n_q, const SumProbs& probs, int max_lag,
                        bool want_ess, bool want_quant) {
    st = MagiColStats{};
    st.C = C; st.R = R; st.n_q = n_q; st.max_lag = max_lag; st.max_cols = max_cols; st.K = K;
    st.want_ess = want_ess; st.want_q = want_quant && n_q > 0; st.probs = probs;
    const size_t cc = (size_t)max_cols, k = (size_t)K;
    s.take(st.yb, R >= 4 ? cc * 2 * (size_t)C : 0);           // (R < 4: no diagnostics, k_sum_moments leaves before it touches ybar)
    s.take(st.col, cc * 4);
    s.take(st.mean, k); s.take(st.sd, k); s.take(st.rhat, k); s.take(st.ess, k); s.take(st.mcse, k);
    s.take(st.quant, st.want_q ? (size_t)n_q * k : 0);
    s.take(st.count, 1, true);
}

int magi_colstats_chunk(magi_handle* h, const char* who, const MagiColStats& st, const double* chunk, int nc, long long k0, int mode, int N, int D) {
    if (nc < 1 || nc > st.max_cols || k0 < 0 || k0 + nc > st.K) return magi_fail(h, MAGI_E_BADARG, std::string(who) + ": statistics chunk out of range");
    const int C = st.C, R = st.R;
    int rc = magi_launch(h, "k_sum_moments: ", k_sum_moments, dim3((unsigned)nc), dim3(SUM_WG), h->stream, C, R, chunk, st.yb, st.col, k0, mode, N, D, st.mean,
                         st.sd, st.rhat, st.count);
    if (rc == MAGI_OK && st.want_ess)
        rc = magi_launch(h, "k_sum_ess: ", k_sum_ess, dim3((unsigned)nc), dim3(SUM_WG), h->stream, C, R, st.max_lag, chunk, (const double*)st.yb,
                         (const double*)st.col, k0, mode, N, D, st.ess, st.mcse);
    if (rc == MAGI_OK && st.want_q)
        rc = magi_launch(h, "k_sum_order: ", k_sum_order, dim3((unsigned)nc), dim3(SUM_WG), h->stream, C * R, chunk, (const double*)st.col, k0, mode, N, D, st.K,
                         st.n_q, st.probs, st.quant);
    return rc;
}

void magi_colstats_down(MagiScratch& s, MagiColStats& st, double* mean, double* sd, double* quant, double* rhat, double* ess, double* mcse) {
    const size_t kb = (size_t)st.K * sizeof(double);
    s.down_opt(mean, st.mean, kb);
    s.down_opt(sd, st.sd, kb);
    s.down_opt(rhat, st.rhat, kb);
    if (st.want_ess) {
        s.down_opt(ess, st.ess, kb);
        s.down_opt(mcse, st.mcse, kb);
    }
    if (st.want_q) s.down_opt(quant, st.quant, (size_t)st.n_q * kb);
    s.down(&st.n_bad, st.count, sizeof(int));
}

int magi_finished_chains(magi_handle* h, const char* who, int chain0, int n_sel, MagiChainRange* out) {
    const std::string me = std::string(who) + ": ";
    if (!h->sampler_ready) return magi_fail(h, MAGI_E_STATE, "sampler not initialised");
    if (chain0 < 0 || n_sel < 1 || (long long)chain0 + n_sel > h->n_chains)
        return magi_fail(h, MAGI_E_BADARG, me + "chains [chain0, chain0 + n_sel) must lie inside the sampler's " + std::to_string(h->n_chains));
    out->member = -1;
    if (h->group_n) {
        const int per = h->group_per > 0 ? h->group_per : h->n_chains;
        out->member = chain0 / per;
        if ((chain0 + n_sel - 1) / per != out->member)
            return magi_fail(h, MAGI_E_BADARG, me + "the chain range spans more than one member of the group (their posteriors differ)");
    }
    (void)hipSetDevice(h->device);
    std::vector<ChainCtl> ctl((size_t)n_sel);
    MAGI_HIP_CHECK(h, hipMemcpy(ctl.data(), h->ch.ctl + chain0, sizeof(ChainCtl) * n_sel, hipMemcpyDeviceToHost));
    for (int c = 0; c < n_sel; ++c)
        if (ctl[c].k < h->cfg.total)
            return magi_fail(h, MAGI_E_STATE, me + "chain " + std::to_string(chain0 + c) + " has taken " + std::to_string((long long)ctl[c].k) + " of " +
                                                  std::to_string((long long)h->cfg.total) + " transitions");
    out->R = h->num_results;
    if (int rc = check_draws(h, who, n_sel, out->R)) return rc;
    out->pb = h->pb;
    if (out->member >= 0) MAGI_HIP_CHECK(h, hipMemcpy(&out->pb, h->d_members + out->member, sizeof(DevProblem), hipMemcpyDeviceToHost));
    out->base = h->ch.samples + (size_t)chain0 * out->R * out->pb.dimp;
    return MAGI_OK;
}

int magi_summarize(magi_handle* h, int C, int R, int K, const double* draws, int n_q, const double* probs, int max_lag, double* mean, double* sd,
                   double* quant, double* rhat, double* ess, double* mcse_mean, int* n_nonfinite) {
    if (!h) return MAGI_E_BADARG;
    static const char* who = "magi_summarize";
    if (!draws) return magi_fail(h, MAGI_E_BADARG, "magi_summarize: draws is NULL");
    int rc = check_draws(h, who, C, R);
    if (rc) return rc;
    if (K < 1 || K > (1 << 24)) return magi_fail(h, MAGI_E_BADARG, "magi_summarize: 1 <= K <= 2^24 columns");
    SumProbs pr;
    if ((rc = check_probs(h, who, n_q, probs, pr))) return rc;
    (void)hipSetDevice(h->device);
    SumLB lb{};
    int count = 0;
    rc = summarize_block(h, who, nullptr, draws, K, C, R, K, MODE_PLAIN, 1, 1, lb, nullptr, nullptr, n_q, pr, max_lag, SumOut{mean, sd, quant, rhat, ess, mcse_mean}, &count);
    if (rc == MAGI_OK && n_nonfinite) *n_nonfinite = count;
    return rc;
}

int magi_sampler_summarize(magi_handle* h, int chain0, int n_sel, int n_q, const double* probs, int max_lag,
                           double* X_mean, double* X_sd, double* X_quant, double* X_rhat, double* X_ess, double* X_mcse_mean,
                           double* sig_mean, double* sig_sd, double* sig_quant, double* sig_rhat, double* sig_ess, double* sig_mcse_mean,
                           double* th_mean, double* th_sd, double* th_quant, double* th_rhat, double* th_ess, double* th_mcse_mean,
                           int* n_nonfinite) {
    if (!h) return MAGI_E_BADARG;
    static const char* who = "magi_sampler_summarize";
    MagiChainRange cr;
    int rc = magi_finished_chains(h, who, chain0, n_sel, &cr);
    if (rc) return rc;
    SumProbs pr;
    if ((rc = check_probs(h, who, n_q, probs, pr))) return rc;
    const DevProblem& pb = h->pb;                              // the shapes; the bounds, supports and priors are cr.pb's: the member's own on a group
    const int R = cr.R;
    SumLB lb{};
    for (int d = 0; d < pb.D; ++d) lb.v[d] = cr.pb.LB[d];
    const double2* tsup = cr.pb.tsup;
    const double4* prior = cr.pb.prior;
    const double* base = cr.base;
    int count = 0;
    if (X_mean || X_sd || X_quant || X_rhat || X_ess || X_mcse_mean || n_nonfinite)
        rc = summarize_block(h, who, base, nullptr, pb.dimp, n_sel, R, pb.ND, MODE_X, pb.N, pb.D, lb, nullptr, nullptr, n_q, pr, max_lag,
                             SumOut{X_mean, X_sd, X_quant, X_rhat, X_ess, X_mcse_mean}, &count);
    if (rc == MAGI_OK && (sig_mean || sig_sd || sig_quant || sig_rhat || sig_ess || sig_mcse_mean || n_nonfinite))
        rc = summarize_block(h, who, base + pb.ND, nullptr, pb.dimp, n_sel, R, pb.D, MODE_SIGMA, pb.N, pb.D, lb, nullptr, prior, n_q, pr, max_lag,
                             SumOut{sig_mean, sig_sd, sig_quant, sig_rhat, sig_ess, sig_mcse_mean}, &count);
    if (rc == MAGI_OK && (th_mean || th_sd || th_quant || th_rhat || th_ess || th_mcse_mean || n_nonfinite))
        rc = summarize_block(h, who, base + pb.ND + pb.D, nullptr, pb.dimp, n_sel, R, pb.P, MODE_THETA, pb.N, pb.D, lb, tsup, nullptr, n_q, pr, max_lag,
                             SumOut{th_mean, th_sd, th_quant, th_rhat, th_ess, th_mcse_mean}, &count);
    if (rc == MAGI_OK && n_nonfinite) *n_nonfinite = count;
    return rc;
}
