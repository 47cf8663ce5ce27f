// Pointwise log-likelihood, WAIC and PSIS-LOO (magi_elpd, magi_sampler_elpd): per observed entry e = d N + i the log predictive density
// lpd, p_waic, elpd_waic, and the Pareto-smoothed importance-sampling leave-one-out estimate elpd_loo with p_loo and the Pareto shape
// khat -- definitions in include/magi_hip.h and DESIGN.md 4.5.  The scheme of summary.hip (colstat.h) for a new quantity:
//   k_ll_gather   tiled gather + transpose through an LDS tile: rows (draws) x observed entries of the samples -> chunk[obs][C R], the
//                 log-likelihood of the entry under the observation model (ObsModel::resid, the sigma^2 of the draw's row as k_sum_gather
//                 MODE_SIGMA forms it) evaluated on the way; the host route (a given log-likelihood array) only transposes.  Chunks of
//                 at most 2^23 doubles.
//   k_ll_waic     one workgroup per observation: non-finite flag, max, log-sum-exp, two-pass variance.
//   k_ll_psis     one workgroup per observation: the log ratios r = -l - max(-l); radix select of the smallest tail key on the
//                 order-preserving key of r (ties go by draw index: a second select over the tied indices); the M tail (key, index) pairs
//                 collected into LDS through an integer slot counter and bitonic-sorted by (key, index), so the slot order does not matter;
//                 the Zhang-Stephens fit, one wave per candidate theta_j; the smoothed log weights written over the sorted keys; two
//                 log-sum-exps over all C R draws (the draws below the tail from the chunk, the tail from LDS by rank).
// Every floating-point sum runs in one fixed order and the only atomics are integer ones: results are bit-identical from run to run and
// do not depend on the chunking.  Does not depend on the drift (jit._DRIFT_FREE).
#include "colstat.h"

#include <climits>
#include <cmath>
#include <vector>

namespace {

using namespace colstat;

constexpr int TAIL_LDS = 2048;                 // (key, index) pairs of LDS k_ll_psis sorts: 24 KiB of its 27 KiB, five workgroups per CU
constexpr int MAX_CAND = 30 + 45;              // candidates m = 30 + floor(sqrt(M)), M <= TAIL_LDS
constexpr long long LOO_MAX_S = 466033;        // the largest C R whose tail M = ceil(3 sqrt(C R)) fits: 9 C R <= TAIL_LDS^2

__global__ __launch_bounds__(G_TILE * 4) void k_ll_gather(int S, int nc, const double* __restrict__ src /* rows ld apart */, long long ld,
                                                          const int* __restrict__ oidx /* the observed entries e of the block's columns; null: src holds the columns themselves */,
                                                          DevProblem pb, SumLB lb, double* __restrict__ chunk /* [nc][S] */) {
    __shared__ double tile[G_TILE][G_TILE + 1];               // (+1: the column reads below fall on 32 different bank pairs)
    __shared__ double s2[G_TILE][MAGI_MAX_D];                 // sigma^2_d of the tile's rows
    const int r0 = blockIdx.x * G_TILE, c0 = blockIdx.y * G_TILE, tx = threadIdx.x, ty = threadIdx.y;
    if (oidx) {
        for (int q = ty * G_TILE + tx; q < G_TILE * pb.D; q += G_TILE * 4) {
            const int r = q / pb.D, d = q - r * pb.D;
            if (r0 + r < S) {
                double v = softplus_ref(src[(size_t)(r0 + r) * (size_t)ld + pb.ND + d]) + lb.v[d];
                if (pb.prior) { const double4 pe = pb.prior[d]; if (Prior::fixed(pe)) v = pe.y; }
                s2[r][d] = v;
            }
        }
        __syncthreads();
    }
    const bool col = c0 + tx < nc;
    int e = c0 + tx, d = 0;
    double gy = 0.0, w = 1.0;
    if (oidx && col) {
        e = oidx[c0 + tx];
        d = e / pb.N;
        gy = pb.yobs[e];
        w = pb.obsw ? pb.obsw[e] : 1.0;
    }
    for (int r = ty; r < G_TILE; r += 4)
        if (r0 + r < S && col) {
            double v = src[(size_t)(r0 + r) * (size_t)ld + e];
            if (oidx) {
                double dss;
                const double ss = ObsModel::resid(pb, d, (size_t)e, v, gy, dss), sg = s2[r][d];
                v = -0.5 * (m_log(2.0 * 3.141592653589793 * sg / w) + ss / sg);
            }
            tile[r][tx] = v;
        }
    __syncthreads();
    for (int c = ty; c < G_TILE; c += 4)
        if (c0 + c < nc && r0 + tx < S) chunk[(size_t)(c0 + c) * S + r0 + tx] = tile[tx][c];
}

__device__ __forceinline__ double wg_max(double v, double* red) { return -wg_min(-v, red); }

__global__ __launch_bounds__(SUM_WG) void k_ll_waic(int S, const double* __restrict__ chunk, long long k0, double* __restrict__ lpd,
                                                    double* __restrict__ p_waic, double* __restrict__ elpd_waic, int* __restrict__ flag /* 1: a non-finite draw */,
                                                    int* __restrict__ n_nonfinite) {
    __shared__ double red[SUM_WG / 64];
    const int tid = threadIdx.x;
    const double* row = chunk + (size_t)blockIdx.x * S;
    const long long o = k0 + blockIdx.x;
    const double nan = __builtin_nan("");
    double s = 0.0, mx = -__builtin_inf();
    int bad = 0;
    for (int e = tid; e < S; e += SUM_WG) {
        const double v = row[e];
        bad |= !isfinite(v);
        s += v;
        mx = fmax(mx, v);
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0) {
            lpd[o] = nan; p_waic[o] = nan; elpd_waic[o] = nan;
            flag[o] = 1;
            atomicAdd(n_nonfinite, 1);
        }
        return;
    }
    s = wg_sum(s, red);
    mx = wg_max(mx, red);
    const double mu = s / (double)S;
    double se = 0.0, ss = 0.0;
    for (int e = tid; e < S; e += SUM_WG) {
        const double v = row[e], dv = v - mu;
        se += m_exp(v - mx);
        ss += dv * dv;
    }
    se = wg_sum(se, red);
    ss = wg_sum(ss, red);
    if (tid == 0) {
        const double l = mx + m_log(se) - m_log((double)S), pw = S < 2 ? nan : ss / (double)(S - 1);
        lpd[o] = l; p_waic[o] = pw; elpd_waic[o] = l - pw;
        flag[o] = 0;
    }
}

__device__ __forceinline__ unsigned long long d2u(double v) { return (unsigned long long)__double_as_longlong(v); }
__device__ __forceinline__ double u2d(unsigned long long b) { return __longlong_as_double((long long)b); }

// log ratio of draw e: -l - max(-l), with -0.0 made +0.0 so that equal ratios have equal keys
__device__ __forceinline__ double log_ratio(const double* __restrict__ row, int e, double mx) {
    const double r = -row[e] - mx;
    return r == 0.0 ? 0.0 : r;
}

// M: the tail length min(S / 5, ceil(3 sqrt(S))) (<= TAIL_LDS), m: the candidates 30 + floor(sqrt(M)) -- both exact integers formed on the host
__global__ __launch_bounds__(SUM_WG) void k_ll_psis(int S, int M, int m, const double* __restrict__ chunk, long long k0, const int* __restrict__ flag,
                                                    const double* __restrict__ lpd, double* __restrict__ elpd_loo, double* __restrict__ p_loo,
                                                    double* __restrict__ khat) {
    static_assert(SUM_WG == 256, "one thread per histogram bin");
    __shared__ unsigned long long tk[TAIL_LDS];               // the tail's keys, then its exceedances, then its log weights (as bits)
    __shared__ int ti[TAIL_LDS];                              // the tail's draw indices
    __shared__ int hist[256];
    __shared__ double red[SUM_WG / 64];
    __shared__ double cth[MAX_CAND], cl[MAX_CAND], cw[MAX_CAND];
    __shared__ unsigned long long s_below;
    __shared__ int s_gt, s_eq, s_cnt;
    const int tid = threadIdx.x;
    const double* row = chunk + (size_t)blockIdx.x * S;
    const long long o = k0 + blockIdx.x;
    if (flag[o]) {                                            // a non-finite draw (uniform over the workgroup)
        if (tid == 0) { elpd_loo[o] = __builtin_nan(""); p_loo[o] = __builtin_nan(""); khat[o] = __builtin_nan(""); }
        return;
    }
    double mx = -__builtin_inf();
    for (int e = tid; e < S; e += SUM_WG) mx = fmax(mx, -row[e]);
    mx = wg_max(mx, red);
    // the smallest key of the tail; the largest ratio is 0, so a tail that starts at 0 is tied throughout
    unsigned long long kt = ~0ull;                            // (no finite ratio has this key: without smoothing no draw is in the tail)
    int thr = -1;
    bool smooth = M >= 5;
    if (smooth) {
        kt = radix_select_keys([row, mx](int e) { return to_key(log_ratio(row, e, mx)); }, S, S - M, 64, hist);
        if (kt == to_key(0.0)) { smooth = false; kt = ~0ull; }
    }
    double kh = __builtin_inf(), ec = 0.0;
    if (smooth) {
        if (tid == 0) { s_gt = 0; s_eq = 0; s_cnt = 0; s_below = 0; }
        __syncthreads();
        int gt = 0, eq = 0;
        unsigned long long below = 0;
        for (int e = tid; e < S; e += SUM_WG) {
            const unsigned long long key = to_key(log_ratio(row, e, mx));
            if (key > kt) ++gt;
            else if (key == kt) ++eq;
            else below = key > below ? key : below;
        }
        atomicAdd(&s_gt, gt);
        atomicAdd(&s_eq, eq);
        atomicMax(&s_below, below);
        __syncthreads();
        const int need = M - s_gt, tied = s_eq;               // of the draws tied at kt the `need` (>= 1) with the largest indices are in the tail
        double cut;
        if (need < tied) {                                    // the ties straddle the cutoff: the draw below the tail is one of them
            cut = from_key(kt);
            thr = (int)radix_select_keys([row, mx, kt](int e) { return to_key(log_ratio(row, e, mx)) == kt ? (unsigned long long)e : 0xFFFFFFull; },
                                         S, tied - need - 1, 24, hist);
        } else {
            cut = from_key(s_below);                          // (S - M >= 1 draws lie below the tail)
        }
        for (int e = tid; e < S; e += SUM_WG) {
            const unsigned long long key = to_key(log_ratio(row, e, mx));
            if (key > kt || (key == kt && e > thr)) {
                const int slot = atomicAdd(&s_cnt, 1);
                if (slot < TAIL_LDS) { tk[slot] = key; ti[slot] = e; }      // (M of them: the bound only keeps a wrong count inside the arrays)
            }
        }
        int n2 = 1;
        while (n2 < M) n2 <<= 1;
        for (int i = M + tid; i < n2; i += SUM_WG) { tk[i] = ~0ull; ti[i] = INT_MAX; }      // the padding sorts last
        __syncthreads();
        for (int k = 2; k <= n2; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < n2; i += SUM_WG) {
                    const int p = i ^ j;
                    if (p > i) {
                        const unsigned long long a = tk[i], b = tk[p];
                        const int ia = ti[i], ib = ti[p];
                        if ((a > b || (a == b && ia > ib)) == ((i & k) == 0)) { tk[i] = b; tk[p] = a; ti[i] = ib; ti[p] = ia; }
                    }
                }
                __syncthreads();
            }
        // exceedances over the cutoff, ascending
        ec = m_exp(cut);
        for (int i = tid; i < M; i += SUM_WG) tk[i] = d2u(m_exp(from_key(tk[i])) - ec);
        __syncthreads();
        const double xM = u2d(tk[M - 1]), xq = u2d(tk[(M + 2) / 4 - 1]), dM = (double)M;
        const int wv = tid >> 6, lane = tid & 63;
        for (int j = wv; j < m; j += SUM_WG / 64) {           // one wave per candidate
            const double th = 1.0 / xM + (1.0 - sqrt((double)m / ((double)(j + 1) - 0.5))) / (3.0 * xq);
            double a = 0.0;
            for (int i = lane; i < M; i += 64) a += m_log1p(-(th * u2d(tk[i])));
            const double k = wave_bsum(a) / dM;
            if (lane == 0) { cth[j] = th; cl[j] = dM * (m_log(-th / k) - k - 1.0); }
        }
        __syncthreads();
        if (tid < m) {
            double a = 0.0;
            for (int i = 0; i < m; ++i) a += m_exp(cl[i] - cl[tid]);
            cw[tid] = cth[tid] * (1.0 / a);
        }
        __syncthreads();
        double th = 0.0;
        for (int j = 0; j < m; ++j) th += cw[j];               // (every thread forms the same sum)
        double a = 0.0;
        for (int i = tid; i < M; i += SUM_WG) a += m_log1p(-(th * u2d(tk[i])));
        const double k = wg_sum(a, red) / dM, sigma = -k / th;
        kh = (k * dM + 5.0) / (dM + 10.0);
        // the tail's log weights, capped at 0: smoothed by the fitted distribution's quantiles, or the ratios themselves
        __syncthreads();                                       // (every thread has read the exceedances)
        for (int i = tid; i < M; i += SUM_WG) {
            double lw;
            if (isfinite(kh)) {
                const double lp = m_log1p(-(((double)(i + 1) - 0.5) / dM));
                const double q = kh != 0.0 ? sigma / kh * expm1(-kh * lp) : -sigma * lp;
                lw = m_log(ec + q);
            } else {
                lw = log_ratio(row, ti[i], mx);
            }
            tk[i] = d2u(fmin(lw, 0.0));
        }
        __syncthreads();
    }
    const int ntail = smooth ? M : 0;
    // logsumexp(l + lw) - logsumexp(lw): the draws below the tail carry their ratio (<= 0), the tail its weights by rank
    double A = -__builtin_inf(), B = -__builtin_inf();
    for (int e = tid; e < S; e += SUM_WG) {
        const double r = log_ratio(row, e, mx);
        const unsigned long long key = to_key(r);
        if (!(key > kt || (key == kt && e > thr))) { A = fmax(A, row[e] + r); B = fmax(B, r); }
    }
    for (int i = tid; i < ntail; i += SUM_WG) {
        const double lw = u2d(tk[i]);
        A = fmax(A, row[ti[i]] + lw);
        B = fmax(B, lw);
    }
    A = wg_max(A, red);
    B = wg_max(B, red);
    double sa = 0.0, sb = 0.0;
    for (int e = tid; e < S; e += SUM_WG) {
        const double r = log_ratio(row, e, mx);
        const unsigned long long key = to_key(r);
        if (!(key > kt || (key == kt && e > thr))) { sa += m_exp(row[e] + r - A); sb += m_exp(r - B); }
    }
    for (int i = tid; i < ntail; i += SUM_WG) {
        const double lw = u2d(tk[i]);
        sa += m_exp(row[ti[i]] + lw - A);
        sb += m_exp(lw - B);
    }
    sa = wg_sum(sa, red);
    sb = wg_sum(sb, red);
    if (tid == 0) {
        const double el = (A + m_log(sa)) - (B + m_log(sb));
        elpd_loo[o] = el; p_loo[o] = lpd[o] - el; khat[o] = kh;
    }
}

struct ElpdOut { double *lpd, *p_waic, *elpd_waic, *elpd_loo, *p_loo, *khat; };

int isqrt_floor(long long v) {
    long long r = (long long)std::sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return (int)r;
}

// K columns of C x R draws: the log-likelihood of the observed entries oidx[K] of the device samples dsrc (rows ld apart) under pb, or
// the host array hsrc [C R][K] as it is.  loglik_out (device route): host [C R][K].
int elpd_block(magi_handle* h, const char* who, const double* dsrc, const double* hsrc, long long ld, int C, int R, long long K,
               const std::vector<int>& oidx, const DevProblem& pb, const ElpdOut& o, double* loglik_out, int* nonfinite) {
    const size_t S = (size_t)C * R;
    const bool want_loo = o.elpd_loo || o.p_loo || o.khat;
    if (want_loo && (long long)S > LOO_MAX_S)
        return magi_fail(h, MAGI_E_BADARG, std::string(who) + ": elpd_loo, p_loo and khat need C R <= " + std::to_string(LOO_MAX_S) +
                                               " draws per column (a tail of at most " + std::to_string(TAIL_LDS) + " draws); lpd and the WAIC outputs are served without them");
    int M = (int)(S / 5);
    const int t = isqrt_floor(9 * (long long)S), ceil3 = (long long)t * t == 9 * (long long)S ? t : t + 1;      // ceil(3 sqrt(S))
    M = std::min(M, ceil3);
    const int m = 30 + isqrt_floor(M);
    const size_t cc = chunk_cols(h, S, (size_t)K);
    SumLB lb{};
    for (int d = 0; d < pb.D && d < MAGI_MAX_D; ++d) lb.v[d] = pb.LB[d];
    const size_t k = (size_t)K, n_idx = oidx.size();
    MagiScratch sc(h, who);
    double *chunk, *stage /* the host route's strided upload */, *dlpd, *dpw, *dew, *del, *dpl, *dkh;
    int *dflag, *dcount, *didx /* the observed entries */;
    sc.take(chunk, cc * S); sc.take(stage, hsrc ? cc * S : 0);
    sc.take(dlpd, k); sc.take(dpw, k); sc.take(dew, k); sc.take(del, k); sc.take(dpl, k); sc.take(dkh, k);
    sc.take(dflag, k); sc.take(dcount, 1, true); sc.take(didx, n_idx);
    if (int rc = sc.alloc()) return rc;
    std::vector<double> back(loglik_out ? cc * S : 0);
    int count = 0;
    if (n_idx) sc.up(didx, oidx.data(), n_idx * sizeof(int));
    for (size_t c0 = 0; c0 < (size_t)K && sc.ok(); c0 += cc) {
        const int nc = (int)std::min(cc, (size_t)K - c0);
        if (hsrc)
            sc.note(hipMemcpy2DAsync(stage, (size_t)nc * sizeof(double), hsrc + c0, (size_t)K * sizeof(double), (size_t)nc * sizeof(double), S,
                                     hipMemcpyHostToDevice, h->stream));
        if (sc.ok())
            sc.note(magi_launch(h, "k_ll_gather: ", k_ll_gather, dim3((unsigned)((S + G_TILE - 1) / G_TILE), (unsigned)((nc + G_TILE - 1) / G_TILE)),
                                dim3(G_TILE, 4), h->stream, (int)S, nc, hsrc ? (const double*)stage : dsrc, hsrc ? (long long)nc : ld,
                                hsrc ? (const int*)nullptr : (const int*)(didx + c0), pb, lb, chunk));
        if (sc.ok())
            sc.note(magi_launch(h, "k_ll_waic: ", k_ll_waic, dim3((unsigned)nc), dim3(SUM_WG), h->stream, (int)S, (const double*)chunk, (long long)c0,
                                dlpd, dpw, dew, dflag, dcount));
        if (sc.ok() && want_loo)
            sc.note(magi_launch(h, "k_ll_psis: ", k_ll_psis, dim3((unsigned)nc), dim3(SUM_WG), h->stream, (int)S, M, m, (const double*)chunk,
                                (long long)c0, (const int*)dflag, (const double*)dlpd, del, dpl, dkh));
        if (sc.ok() && loglik_out) {                           // chunk [nc][S] -> loglik_out [S][K]
            sc.down(back.data(), chunk, (size_t)nc * S * sizeof(double));
            if (sc.ok()) sc.note(hipStreamSynchronize(h->stream));
            if (!sc.ok()) break;
            for (int c = 0; c < nc; ++c)
                for (size_t s = 0; s < S; ++s) loglik_out[s * (size_t)K + c0 + c] = back[(size_t)c * S + s];
        }
    }
    const size_t kb = k * sizeof(double);
    sc.down_opt(o.lpd, dlpd, kb);
    sc.down_opt(o.p_waic, dpw, kb);
    sc.down_opt(o.elpd_waic, dew, kb);
    sc.down_opt(o.elpd_loo, del, kb);
    sc.down_opt(o.p_loo, dpl, kb);
    sc.down_opt(o.khat, dkh, kb);
    sc.down(&count, dcount, sizeof(int));
    if (int rc = sc.finish()) return rc;
    if (nonfinite) *nonfinite = count;
    return MAGI_OK;
}

}  // namespace

int magi_elpd(magi_handle* h, int C, int R, int K, const double* loglik, double* lpd, double* p_waic, double* elpd_waic, double* elpd_loo,
              double* p_loo, double* khat, int* n_nonfinite) {
    if (!h) return MAGI_E_BADARG;
    static const char* who = "magi_elpd";
    if (!loglik) return magi_fail(h, MAGI_E_BADARG, "magi_elpd: loglik is NULL");
    int rc = check_draws(h, who, C, R);
    if (rc) return rc;
    if (K < 1 || K > (1 << 24)) return magi_fail(h, MAGI_E_BADARG, "magi_elpd: 1 <= K <= 2^24 columns");
    (void)hipSetDevice(h->device);
    DevProblem none{};
    return elpd_block(h, who, nullptr, loglik, K, C, R, K, std::vector<int>(), none, ElpdOut{lpd, p_waic, elpd_waic, elpd_loo, p_loo, khat}, nullptr, n_nonfinite);
}

int magi_sampler_elpd(magi_handle* h, int chain0, int n_sel, double* lpd, double* p_waic, double* elpd_waic, double* elpd_loo, double* p_loo,
                      double* khat, int* obs_index, int* n_obs_out, double* loglik_out, int* n_nonfinite) {
    if (!h) return MAGI_E_BADARG;
    static const char* who = "magi_sampler_elpd";
    MagiChainRange cr;
    if (int rc = magi_finished_chains(h, who, chain0, n_sel, &cr)) return rc;
    const DevProblem& pb = cr.pb;
    std::vector<double> y((size_t)pb.ND);
    MAGI_HIP_CHECK(h, hipMemcpy(y.data(), pb.yobs, y.size() * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<int> oidx;
    for (int e = 0; e < pb.ND; ++e)
        if (!std::isnan(y[e])) oidx.push_back(e);
    const int K = (int)oidx.size();
    if (n_obs_out) *n_obs_out = K;
    if (obs_index) std::copy(oidx.begin(), oidx.end(), obs_index);
    if (n_nonfinite) *n_nonfinite = 0;
    if (K == 0 || !(lpd || p_waic || elpd_waic || elpd_loo || p_loo || khat || loglik_out || n_nonfinite)) return MAGI_OK;
    return elpd_block(h, who, cr.base, nullptr, pb.dimp, n_sel, cr.R, K, oidx, pb, ElpdOut{lpd, p_waic, elpd_waic, elpd_loo, p_loo, khat}, loglik_out, n_nonfinite);
}
