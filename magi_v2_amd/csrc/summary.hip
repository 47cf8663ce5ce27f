// Posterior summaries and convergence diagnostics (magi_summarize, magi_sampler_summarize): per scalar column of C chains x R draws the
// pooled mean, sd (ddof 1) and quantiles (exact order statistics, linear interpolation), split R-hat, ESS (Geyer's initial monotone
// sequence over the split chains' autocovariances) and the Monte-Carlo standard error of the mean -- definitions in include/magi_hip.h and DESIGN.md 4.4.
// A sample row is [D][N] | sig_pre[D] | th_pre[P] | pad: the draws of one column lie dimp doubles apart.  So
//   k_sum_gather    tiled gather + transpose through an LDS tile (as k_ode_transpose): rows x columns of the source -> chunk[column][C R],
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
#include "colstat.h"

#include <cmath>
#include <vector>

namespace {

using namespace colstat;              // SUM_WG, G_TILE, SUM_LDS, the workgroup reductions, to_key / radix_select, check_draws (shared with elpd.hip)
constexpr int MAX_Q = 16;

enum { MODE_PLAIN = 0, MODE_X = 1, MODE_SIGMA = 2, MODE_THETA = 3 };

struct SumProbs { double p[MAX_Q]; };

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

// where column j of a block goes in the caller's arrays: the X block is walked in the samples' order [D][N] and reported in the host
// layout [N][D]
__device__ __forceinline__ long long out_index(int mode, long long j, int N, int D) {
    return mode == MODE_X ? (j % N) * (long long)D + j / N : j;
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

struct SumOut { double *mean, *sd, *quant, *rhat, *ess, *mcse; };

// one block of K columns of C x R draws: from the device (dsrc: column j of row r at dsrc[r ld + j]) or from the host (hsrc [C R][K]).
// Adds the block's columns with a non-finite draw to *nonfinite.
int summarize_block(magi_handle* h, const char* who, const double* dsrc, const double* hsrc, long long ld, int C, int R, long long K, int mode,
                    int N, int D, const SumLB& lb, const double2* tsup, const double4* prior, int n_q, const SumProbs& probs, int max_lag, const SumOut& o, int* nonfinite) {
    const size_t S = (size_t)C * R, M = 2 * (size_t)C;
    const size_t cc = chunk_cols(h, S, (size_t)K);
    const bool diag = R >= 4, want_ess = o.ess || o.mcse, want_q = n_q > 0 && o.quant;
    // one device buffer: chunk (cc S) | staging of the host route (cc S) | ybar (cc M) | col (cc 4) | mean, sd, rhat, ess, mcse (K each) |
    // quant (n_q K) | the counter (1 int)
    const size_t n_stage = hsrc ? cc * S : 0, n_yb = diag ? cc * M : 0, nq = want_q ? (size_t)n_q * K : 0;
    const size_t doubles = cc * S + n_stage + n_yb + cc * 4 + 5 * (size_t)K + nq;
    double* buf = nullptr;
    MAGI_HIP_CHECK(h, hipMalloc((void**)&buf, doubles * sizeof(double) + sizeof(int)));
    double *chunk = buf, *stage = chunk + cc * S, *yb = stage + n_stage, *col = yb + n_yb, *dmean = col + cc * 4, *dsd = dmean + K, *drhat = dsd + K,
           *dess = drhat + K, *dmcse = dess + K, *dq = dmcse + K;
    int* dcount = reinterpret_cast<int*>(dq + nq);
    int rc = MAGI_OK, count = 0;
    hipError_t e = hipMemsetAsync(dcount, 0, sizeof(int), h->stream);
    for (size_t c0 = 0; c0 < (size_t)K && rc == MAGI_OK && e == hipSuccess; c0 += cc) {
        const int nc = (int)std::min(cc, (size_t)K - c0);
        const double* src = dsrc ? dsrc + c0 : stage;
        const long long sld = dsrc ? ld : nc;
        if (hsrc) {
            e = hipMemcpy2DAsync(stage, (size_t)nc * sizeof(double), hsrc + c0, (size_t)K * sizeof(double), (size_t)nc * sizeof(double), S,
                                 hipMemcpyHostToDevice, h->stream);
            if (e != hipSuccess) break;
        }
        rc = magi_launch(h, "k_sum_gather: ", k_sum_gather, dim3((unsigned)((S + G_TILE - 1) / G_TILE), (unsigned)((nc + G_TILE - 1) / G_TILE)),
                         dim3(G_TILE, 4), h->stream, (int)S, nc, src, sld, mode, (int)c0, lb, tsup, prior, chunk);
        if (rc == MAGI_OK)
            rc = magi_launch(h, "k_sum_moments: ", k_sum_moments, dim3((unsigned)nc), dim3(SUM_WG), h->stream, C, R, (const double*)chunk, yb, col,
                             (long long)c0, mode, N, D, dmean, dsd, drhat, dcount);
        if (rc == MAGI_OK && want_ess)
            rc = magi_launch(h, "k_sum_ess: ", k_sum_ess, dim3((unsigned)nc), dim3(SUM_WG), h->stream, C, R, max_lag, (const double*)chunk,
                             (const double*)yb, (const double*)col, (long long)c0, mode, N, D, dess, dmcse);
        if (rc == MAGI_OK && want_q)
            rc = magi_launch(h, "k_sum_order: ", k_sum_order, dim3((unsigned)nc), dim3(SUM_WG), h->stream, (int)S, (const double*)chunk,
                             (const double*)col, (long long)c0, mode, N, D, K, n_q, probs, dq);
    }
    const bool ok = rc == MAGI_OK;
    const size_t kb = (size_t)K * sizeof(double);
    if (ok && e == hipSuccess && o.mean) e = hipMemcpyAsync(o.mean, dmean, kb, hipMemcpyDeviceToHost, h->stream);
    if (ok && e == hipSuccess && o.sd) e = hipMemcpyAsync(o.sd, dsd, kb, hipMemcpyDeviceToHost, h->stream);
    if (ok && e == hipSuccess && o.rhat) e = hipMemcpyAsync(o.rhat, drhat, kb, hipMemcpyDeviceToHost, h->stream);
    if (ok && e == hipSuccess && o.ess) e = hipMemcpyAsync(o.ess, dess, kb, hipMemcpyDeviceToHost, h->stream);
    if (ok && e == hipSuccess && o.mcse) e = hipMemcpyAsync(o.mcse, dmcse, kb, hipMemcpyDeviceToHost, h->stream);
    if (ok && e == hipSuccess && want_q) e = hipMemcpyAsync(o.quant, dq, nq * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (ok && e == hipSuccess) e = hipMemcpyAsync(&count, dcount, sizeof(int), hipMemcpyDeviceToHost, h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream);          // (also on an error path: nothing may be in flight when the buffer goes)
    (void)hipFree(buf);
    if (rc != MAGI_OK) return rc;
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return magi_fail(h, MAGI_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    if (nonfinite) *nonfinite += count;
    return MAGI_OK;
}

// the checks the two entry points share; fills pr
int check_probs(magi_handle* h, const char* who, int n_q, const double* probs, SumProbs& pr) {
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

}  // namespace

// The device-source route for columns already in chunk layout (magi_internal.h; gp.hip): the launches of summarize_block without its gather.
struct MagiColStats {
    const char* who;
    int C, R, n_q, max_lag, max_cols;
    long long K;
    bool want_ess, want_q;
    SumProbs probs;
    double *buf, *yb, *col, *mean, *sd, *rhat, *ess, *mcse, *quant;
    int* count;
};

int magi_colstats_begin(magi_handle* h, const char* who, int C, int R, long long K, int max_cols, int n_q, const double* probs, int max_lag,
                        bool want_ess, bool want_quant, MagiColStats** out) {
    *out = nullptr;
    SumProbs pr;
    int rc = check_draws(h, who, C, R);
    if (rc == MAGI_OK) rc = check_probs(h, who, n_q, probs, pr);
    if (rc) return rc;
    MagiColStats* st = new MagiColStats{};
    st->who = who; st->C = C; st->R = R; st->n_q = n_q; st->max_lag = max_lag; st->max_cols = max_cols; st->K = K;
    st->want_ess = want_ess; st->want_q = want_quant && n_q > 0; st->probs = pr;
    const size_t cc = (size_t)max_cols, n_yb = R >= 4 ? cc * 2 * (size_t)C : 0, nq = st->want_q ? (size_t)n_q * K : 0;
    // one device buffer: ybar (cc 2 C) | col (cc 4) | mean, sd, rhat, ess, mcse (K each) | quant (n_q K) | the counter (1 int)
    hipError_t e = hipMalloc((void**)&st->buf, (n_yb + cc * 4 + 5 * (size_t)K + nq) * sizeof(double) + sizeof(int));
    if (e != hipSuccess) {
        delete st;
        return magi_fail(h, MAGI_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    }
    st->yb = st->buf; st->col = st->yb + n_yb; st->mean = st->col + cc * 4; st->sd = st->mean + K; st->rhat = st->sd + K; st->ess = st->rhat + K;
    st->mcse = st->ess + K; st->quant = st->mcse + K;
    st->count = reinterpret_cast<int*>(st->quant + nq);
    *out = st;
    MAGI_HIP_CHECK(h, hipMemsetAsync(st->count, 0, sizeof(int), h->stream));
    return MAGI_OK;
}

int magi_colstats_chunk(magi_handle* h, MagiColStats* st, const double* chunk, int nc, long long k0) {
    if (nc < 1 || nc > st->max_cols || k0 < 0 || k0 + nc > st->K) return magi_fail(h, MAGI_E_BADARG, std::string(st->who) + ": statistics chunk out of range");
    const int C = st->C, R = st->R;
    int rc = magi_launch(h, "k_sum_moments: ", k_sum_moments, dim3((unsigned)nc), dim3(SUM_WG), h->stream, C, R, chunk, st->yb, st->col, k0, (int)MODE_PLAIN, 1, 1,
                         st->mean, st->sd, st->rhat, st->count);
    if (rc == MAGI_OK && st->want_ess)
        rc = magi_launch(h, "k_sum_ess: ", k_sum_ess, dim3((unsigned)nc), dim3(SUM_WG), h->stream, C, R, st->max_lag, chunk, (const double*)st->yb,
                         (const double*)st->col, k0, (int)MODE_PLAIN, 1, 1, st->ess, st->mcse);
    if (rc == MAGI_OK && st->want_q)
        rc = magi_launch(h, "k_sum_order: ", k_sum_order, dim3((unsigned)nc), dim3(SUM_WG), h->stream, C * R, chunk, (const double*)st->col, k0,
                         (int)MODE_PLAIN, 1, 1, st->K, st->n_q, st->probs, st->quant);
    return rc;
}

int magi_colstats_end(magi_handle* h, MagiColStats* st, double* mean, double* sd, double* quant, double* rhat, double* ess, double* mcse, int* nonfinite) {
    if (!st) return MAGI_OK;
    const size_t kb = (size_t)st->K * sizeof(double);
    int count = 0;
    hipError_t e = hipSuccess;
    if (mean) e = hipMemcpyAsync(mean, st->mean, kb, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && sd) e = hipMemcpyAsync(sd, st->sd, kb, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && rhat) e = hipMemcpyAsync(rhat, st->rhat, kb, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && ess && st->want_ess) e = hipMemcpyAsync(ess, st->ess, kb, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && mcse && st->want_ess) e = hipMemcpyAsync(mcse, st->mcse, kb, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && quant && st->want_q) e = hipMemcpyAsync(quant, st->quant, (size_t)st->n_q * kb, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && nonfinite) e = hipMemcpyAsync(&count, st->count, sizeof(int), hipMemcpyDeviceToHost, h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream);          // (also on an error path: nothing may be in flight when the buffer goes)
    const std::string who = st->who;
    (void)hipFree(st->buf);
    delete st;
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return magi_fail(h, MAGI_E_HIP, who + ": " + hipGetErrorString(e));
    if (nonfinite) *nonfinite += count;
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
    if (!h->sampler_ready) return magi_fail(h, MAGI_E_STATE, "sampler not initialised");
    if (chain0 < 0 || n_sel < 1 || (long long)chain0 + n_sel > h->n_chains)
        return magi_fail(h, MAGI_E_BADARG, "magi_sampler_summarize: chains [chain0, chain0 + n_sel) must lie inside the sampler's " + std::to_string(h->n_chains));
    SumProbs pr;
    int rc = check_probs(h, who, n_q, probs, pr);
    if (rc) return rc;
    int member = -1;
    if (h->group_n) {
        const int per = h->group_per > 0 ? h->group_per : h->n_chains;
        member = chain0 / per;
        if ((chain0 + n_sel - 1) / per != member)
            return magi_fail(h, MAGI_E_BADARG, "magi_sampler_summarize: the chain range spans more than one member of the group (their posteriors differ)");
    }
    (void)hipSetDevice(h->device);
    std::vector<ChainCtl> ctl((size_t)n_sel);
    MAGI_HIP_CHECK(h, hipMemcpy(ctl.data(), h->ch.ctl + chain0, sizeof(ChainCtl) * n_sel, hipMemcpyDeviceToHost));
    for (int c = 0; c < n_sel; ++c)
        if (ctl[c].k < h->cfg.total)
            return magi_fail(h, MAGI_E_STATE, "magi_sampler_summarize: chain " + std::to_string(chain0 + c) + " has taken " + std::to_string((long long)ctl[c].k) +
                                                  " of " + std::to_string((long long)h->cfg.total) + " transitions");
    const int R = h->num_results;
    if ((rc = check_draws(h, who, n_sel, R))) return rc;
    const DevProblem& pb = h->pb;
    SumLB lb{};
    const double2* tsup = pb.tsup;                             // the parameters' supports: the handle's, or the member's own on a group
    const double4* prior = pb.prior;                           // likewise the prior table
    if (member >= 0) {                                         // the member's problem as the sampler read it (magi_sampler_init)
        DevProblem mp;
        MAGI_HIP_CHECK(h, hipMemcpy(&mp, h->d_members + member, sizeof(DevProblem), hipMemcpyDeviceToHost));
        for (int d = 0; d < pb.D; ++d) lb.v[d] = mp.LB[d];
        tsup = mp.tsup;
        prior = mp.prior;
    } else {
        for (int d = 0; d < pb.D; ++d) lb.v[d] = pb.LB[d];
    }
    const double* base = h->ch.samples + (size_t)chain0 * R * pb.dimp;
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
