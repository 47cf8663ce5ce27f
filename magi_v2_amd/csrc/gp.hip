// Posterior trajectories at any time: GP conditioning of the draws on the grid (magi_matern_cross, magi_gp_predict,
// magi_sampler_gp_predict; definitions in include/magi_hip.h and DESIGN.md 4.7).  Per component d, with C^-1_d the resident dense stack
// AS STORED (never symmetrised or transposed) and Ks_d, pKs_d the Matern cross blocks of the new times against the grid times:
//   W_d = Ks_d C^-1_d,  Wd_d = pKs_d C^-1_d                                     [T][N]   (k_gemm_f64 of build.hip, all components per launch)
//   cond_var[m][d]  = max(0, phi1_d    - sum_k W_d[m][k]  Ks_d[m][k])
//   dcond_var[m][d] = max(0, diag_pp_d - sum_k Wd_d[m][k] pKs_d[m][k])                    (k_gp_rows: one workgroup per row)
//   x_new[s][m][d]  = sum_k W_d[m][k]  X_s[d][k] + mu_d (1 - sum_k W_d[m][k])
//   dx_new[s][m][d] = sum_k Wd_d[m][k] X_s[d][k] - mu_d sum_k Wd_d[m][k]
// The sums over the draws are ONE GEMM whose B operand is the sample buffer read in place (B(n = s, k) = samples[s dimp + d N + k], or the
// caller's host layout [S][N][D] uploaded as it is: only the strides differ); mu enters through the two row constants, formed by
// k_gp_rows from the row sums of the same W / Wd the GEMM reads and added by k_gp_shift -- no pass over the samples subtracts it.  The
// GEMM writes chunk[column = (m, d)][S], the layout the statistics kernels of summary.hip consume (magi_colstats_*), so the summaries
// need no gather; the draws themselves, when the caller wants them, go through k_gp_transpose to the host layout [S][T][D].
// The rows of t_new go in chunks so that no buffer exceeds 2^23 doubles (64 MiB, the rule of summary.hip) unless a single row needs
// more; W and Wd of a chunk are formed once and serve every draw.  Nothing depends on the chunking: an output's k loop runs in the same
// order wherever its row falls in a tile, and every row sum runs in one fixed order (lane-strided partials, colstat::wg_sum), so
// the results are bit-identical from run to run and from chunking to chunking.  Does not depend on the drift (jit._DRIFT_FREE).
#include "colstat.h"

#include <cmath>
#include <vector>

namespace {

using namespace colstat;
constexpr int TR = 64;                // k_gp_transpose: 64 x 64 doubles per workgroup of 64 x 4 threads

struct GpComp { double phi1[MAGI_MAX_D], diag_pp[MAGI_MAX_D], mu[MAGI_MAX_D]; };

// grid (tc, D, 1 or 2): z = 0 the value (W against Ks, prior variance phi1), z = 1 the derivative (Wd against pKs, prior variance diag_pp).
// w, ks: [2][D][tc][N] (value planes, then derivative planes); var: [2][T][D]; shift: [2][tc][D]
__global__ __launch_bounds__(SUM_WG) void k_gp_rows(int tc, int N, int D, int T, int m0, const double* __restrict__ w, const double* __restrict__ ks, GpComp cp,
                                                    double* __restrict__ var, double* __restrict__ shift) {
    __shared__ double red[SUM_WG / 64];
    const int m = blockIdx.x, d = blockIdx.y, z = blockIdx.z;
    const size_t row = (((size_t)z * D + d) * tc + m) * (size_t)N;
    const double *wr = w + row, *kr = ks + row;
    double dot = 0.0, rs = 0.0;
    for (int k = threadIdx.x; k < N; k += SUM_WG) {
        const double wv = wr[k];
        dot += wv * kr[k];
        rs += wv;
    }
    dot = wg_sum(dot, red);
    rs = wg_sum(rs, red);
    if (threadIdx.x == 0) {
        const double prior = z ? cp.diag_pp[d] : cp.phi1[d];
        var[((size_t)z * T + m0 + m) * D + d] = fmax(0.0, prior - dot);
        shift[((size_t)z * tc + m) * D + d] = z ? -(cp.mu[d] * rs) : cp.mu[d] * (1.0 - rs);
    }
}

// chunk[column][S] += shift[column]; grid (columns, ceil(S / 256))
__global__ __launch_bounds__(SUM_WG) void k_gp_shift(int S, double* __restrict__ chunk, const double* __restrict__ shift) {
    const int s = blockIdx.y * SUM_WG + threadIdx.x;
    if (s < S) chunk[(size_t)blockIdx.x * S + s] += shift[blockIdx.x];
}

// chunk[nc][S] -> out[S][nc] through an LDS tile; grid (ceil(S / 64), ceil(nc / 64)), block (64, 4)
__global__ __launch_bounds__(TR * 4) void k_gp_transpose(int S, int nc, const double* __restrict__ chunk, double* __restrict__ out) {
    __shared__ double tile[TR][TR + 1];                       // (+1: the column reads below fall on 32 different bank pairs)
    const int s0 = blockIdx.x * TR, c0 = blockIdx.y * TR, tx = threadIdx.x, ty = threadIdx.y;
    for (int c = ty; c < TR; c += 4)
        if (c0 + c < nc && s0 + tx < S) tile[c][tx] = chunk[(size_t)(c0 + c) * S + s0 + tx];
    __syncthreads();
    for (int r = ty; r < TR; r += 4)
        if (s0 + r < S && c0 + tx < nc) out[(size_t)(s0 + r) * nc + c0 + tx] = tile[tx][r];
}

struct GpBuf {                        // releases its buffer after the stream has drained (also on every error path)
    magi_handle* h;
    double* p = nullptr;
    ~GpBuf() {
        (void)hipStreamSynchronize(h->stream);
        if (p) (void)hipFree(p);
    }
};

struct GpDraws {                      // the B operand of the application GEMM: B(n = s, k) of component d at base[d bd + s sn + k sk]
    const double* base;
    long sn, sk, bd;
    int C, R;                         // S = C R draws
};

struct GpOut {
    double *x_new, *dx_new, *cond_var, *dcond_var;
    double *x[6], *dx[6];             // mean, sd, quant, rhat, ess, mcse
    int* n_nonfinite;
};

bool any(double* const (&a)[6]) { return a[0] || a[1] || a[2] || a[3] || a[4] || a[5]; }

int check_hyper(magi_handle* h, const char* who, int D, const double* phi1, const double* phi2, double nu) {
    if (!(nu > 1.0) || !std::isfinite(nu)) return magi_fail(h, MAGI_E_BADARG, std::string(who) + ": nu must exceed 1 (once-differentiable Matern)");
    for (int d = 0; d < D; ++d)
        if (!(phi1[d] > 0.0) || !(phi2[d] > 0.0) || !std::isfinite(phi1[d]) || !std::isfinite(phi2[d]))
            return magi_fail(h, MAGI_E_BADARG, std::string(who) + ": phi1 and phi2 must be positive");
    return MAGI_OK;
}

int check_times(magi_handle* h, const char* who, const char* name, const double* t, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(t[i])) return magi_fail(h, MAGI_E_BADARG, std::string(who) + ": " + name + "[" + std::to_string(i) + "] is not finite");
    return MAGI_OK;
}

int check_T(magi_handle* h, const char* who, int T) {
    if (T < 1 || T > (1 << 16)) return magi_fail(h, MAGI_E_BADARG, std::string(who) + ": 1 <= T <= 2^16 new times");
    return MAGI_OK;
}

// rows of t_new per chunk: no buffer above 2^23 doubles unless one row needs more (the test switch gp_chunk_rows forces small chunks)
int chunk_rows(const magi_handle* h, int T, int N, int D, size_t S) {
    const size_t per_row = (size_t)D * std::max((size_t)N, S);
    size_t tc = std::max<size_t>(1, CHUNK_DOUBLES / per_row);
    if (tc > 128) tc -= tc % 128;                              // whole 128-row GEMM tiles: 262 rows would pay for 384 in both products
    tc = std::min<size_t>(tc, (size_t)T);
    if (h->opt.gp_chunk_rows > 0) tc = std::min<size_t>(tc, (size_t)h->opt.gp_chunk_rows);
    return (int)tc;
}

// per-stage device time while the option gp_profile is set (HIP events, a synchronisation per stage: diagnostics only)
struct GpStage {
    magi_handle* h;
    bool on;
    void begin() const { if (on) (void)hipEventRecord(h->ev_t0, h->stream); }
    void end(int stage) const {
        if (!on) return;
        float ms = 0.f;
        (void)hipEventRecord(h->ev_t1, h->stream);
        if (hipEventSynchronize(h->ev_t1) == hipSuccess && hipEventElapsedTime(&ms, h->ev_t0, h->ev_t1) == hipSuccess) h->gp_ms[stage] += (double)ms;
    }
};

// the whole computation: dCinv the dense C^-1 stack [D][N][N] on the device, I and t_new on the host, the draws on the device
int gp_core(magi_handle* h, const char* who, const double* dCinv, const double* I, int N, int D, const double* phi1, const double* phi2, double nu,
            const double* mu, int T, const double* t_new, const GpDraws& dr, int n_q, const double* probs, int max_lag, const GpOut& o) {
    const size_t S = (size_t)dr.C * dr.R;
    const bool want_x_stats = any(o.x) || o.n_nonfinite, want_dx_stats = any(o.dx);
    const bool deriv = o.dx_new || o.dcond_var || want_dx_stats;
    const bool apply = o.x_new || o.dx_new || want_x_stats || want_dx_stats;
    const int nz = deriv ? 2 : 1;
    const int tc = chunk_rows(h, T, N, D, apply ? S : 1);
    const size_t plane = (size_t)D * tc * N, cplane = (size_t)D * tc * S;
    const bool stage = o.x_new || o.dx_new;
    GpComp cp{};
    for (int d = 0; d < D; ++d) { cp.phi1[d] = phi1[d]; cp.diag_pp[d] = magi_matern_diag_pp(phi1[d], phi2[d], nu); cp.mu[d] = mu[d]; }
    for (double& t : h->gp_ms) t = 0.0;
    const GpStage prof{h, h->opt.gp_profile != 0};

    // one device buffer: I (N) | t_new (T) | Ks, pKs (2 planes) | W, Wd (2 planes) | shift (2 tc D) | var (2 T D) | x, dx chunks (2 cplanes) |
    // staging of the draws on their way to the host (1 cplane)
    GpBuf buf{h};
    const size_t doubles = (size_t)N + T + 4 * plane + 2 * (size_t)tc * D + 2 * (size_t)T * D + (apply ? 2 * cplane : 0) + (stage ? cplane : 0);
    MAGI_HIP_CHECK(h, hipMalloc((void**)&buf.p, doubles * sizeof(double)));
    double *dI = buf.p, *dT = dI + N, *ks = dT + T, *w = ks + 2 * plane, *shift = w + 2 * plane, *var = shift + 2 * (size_t)tc * D,
           *xc = var + 2 * (size_t)T * D, *st = xc + (apply ? 2 * cplane : 0);
    MAGI_HIP_CHECK(h, hipMemcpyAsync(dI, I, sizeof(double) * N, hipMemcpyHostToDevice, h->stream));
    MAGI_HIP_CHECK(h, hipMemcpyAsync(dT, t_new, sizeof(double) * T, hipMemcpyHostToDevice, h->stream));

    MagiColStats *sx = nullptr, *sdx = nullptr;
    int rc = MAGI_OK, count = 0;
    if (want_x_stats) rc = magi_colstats_begin(h, who, dr.C, dr.R, (long long)T * D, tc * D, n_q, probs, max_lag, o.x[4] || o.x[5], o.x[2] != nullptr, &sx);
    if (rc == MAGI_OK && want_dx_stats)
        rc = magi_colstats_begin(h, who, dr.C, dr.R, (long long)T * D, tc * D, n_q, probs, max_lag, o.dx[4] || o.dx[5], o.dx[2] != nullptr, &sdx);
    hipError_t e = hipSuccess;
    for (int m0 = 0; m0 < T && rc == MAGI_OK && e == hipSuccess; m0 += tc) {
        const int nt = std::min(tc, T - m0), nc = nt * D;
        // (the planes of a short last chunk are packed at ITS pitch nt: every stride below is in nt)
        const size_t pl = (size_t)D * nt * N, cpl = (size_t)nc * S;
        prof.begin();
        for (int d = 0; d < D && rc == MAGI_OK; ++d)
            rc = magi_matern_cross_launch(h, h->stream, dT + m0, nt, dI, N, phi1[d], phi2[d], nu, ks + (size_t)d * nt * N,
                                          deriv ? ks + pl + (size_t)d * nt * N : nullptr);
        prof.end(0);
        if (rc) break;
        prof.begin();
        MagiGemm g{};           // W_d = Ks_d C^-1_d: rows of Ks times columns of C^-1 as stored, B(n, k) = C^-1[k][n]
        g.A = ks; g.sAm = N; g.sAk = 1; g.batchA = (long)nt * N; g.batchA2 = (long)pl;
        g.B = dCinv; g.sBn = 1; g.sBk = N; g.batchB = (long)N * N; g.batchB2 = 0;
        g.C = w; g.ldc = N; g.batchC = (long)nt * N; g.batchC2 = (long)pl;
        g.M = nt; g.N = N; g.K = N; g.inner = D; g.outer = nz;
        rc = magi_gemm_strided(h, h->stream, g);
        if (rc == MAGI_OK)
            rc = magi_launch(h, "k_gp_rows: ", k_gp_rows, dim3((unsigned)nt, (unsigned)D, (unsigned)nz), dim3(SUM_WG), h->stream, nt, N, D, T, m0, (const double*)w,
                             (const double*)ks, cp, var, shift);
        prof.end(1);
        if (rc || !apply) continue;
        prof.begin();
        MagiGemm a{};           // chunk[(m, d)][s] = sum_k W_d[m][k] B_d(s, k): the draws read in place
        a.A = w; a.sAm = N; a.sAk = 1; a.batchA = (long)nt * N; a.batchA2 = (long)pl;
        a.B = dr.base; a.sBn = dr.sn; a.sBk = dr.sk; a.batchB = dr.bd; a.batchB2 = 0;
        a.C = xc; a.ldc = (long)D * (long)S; a.batchC = (long)S; a.batchC2 = (long)cpl;
        a.M = nt; a.N = (int)S; a.K = N; a.inner = D; a.outer = nz;
        rc = magi_gemm_strided(h, h->stream, a);
        prof.end(2);
        prof.begin();
        // (shift is [2][nt][D] at this chunk's pitch, the chunk planes [2][nc][S]: one launch adds both)
        if (rc == MAGI_OK)
            rc = magi_launch(h, "k_gp_shift: ", k_gp_shift, dim3((unsigned)(nz * nc), (unsigned)((S + SUM_WG - 1) / SUM_WG)), dim3(SUM_WG), h->stream, (int)S, xc,
                             (const double*)shift);
        prof.end(3);
        if (rc) break;
        prof.begin();
        if (sx) rc = magi_colstats_chunk(h, sx, xc, nc, (long long)m0 * D);
        if (rc == MAGI_OK && sdx) rc = magi_colstats_chunk(h, sdx, xc + cpl, nc, (long long)m0 * D);
        prof.end(4);
        double* const dst[2] = {o.x_new, o.dx_new};
        for (int z = 0; z < 2 && rc == MAGI_OK && e == hipSuccess; ++z) {
            if (!dst[z]) continue;
            rc = magi_launch(h, "k_gp_transpose: ", k_gp_transpose, dim3((unsigned)((S + TR - 1) / TR), (unsigned)((nc + TR - 1) / TR)), dim3(TR, 4), h->stream,
                             (int)S, nc, (const double*)(xc + z * cpl), st);
            if (rc == MAGI_OK)
                e = hipMemcpy2DAsync(dst[z] + (size_t)m0 * D, (size_t)T * D * sizeof(double), st, (size_t)nc * sizeof(double), (size_t)nc * sizeof(double), S,
                                     hipMemcpyDeviceToHost, h->stream);
        }
    }
    const size_t vb = (size_t)T * D * sizeof(double);
    if (rc == MAGI_OK && e == hipSuccess && o.cond_var) e = hipMemcpyAsync(o.cond_var, var, vb, hipMemcpyDeviceToHost, h->stream);
    if (rc == MAGI_OK && e == hipSuccess && o.dcond_var) e = hipMemcpyAsync(o.dcond_var, var + (size_t)T * D, vb, hipMemcpyDeviceToHost, h->stream);
    const bool ok = rc == MAGI_OK && e == hipSuccess;
    // (the ends also release the statistics' buffers on an error path: then nothing is downloaded)
    const int r1 = magi_colstats_end(h, sx, ok ? o.x[0] : nullptr, ok ? o.x[1] : nullptr, ok ? o.x[2] : nullptr, ok ? o.x[3] : nullptr, ok ? o.x[4] : nullptr,
                                     ok ? o.x[5] : nullptr, ok ? &count : nullptr);
    const int r2 = magi_colstats_end(h, sdx, ok ? o.dx[0] : nullptr, ok ? o.dx[1] : nullptr, ok ? o.dx[2] : nullptr, ok ? o.dx[3] : nullptr,
                                     ok ? o.dx[4] : nullptr, ok ? o.dx[5] : nullptr, ok ? &count : nullptr);
    const hipError_t es = hipStreamSynchronize(h->stream);
    if (rc != MAGI_OK) return rc;
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return magi_fail(h, MAGI_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    if (r1 != MAGI_OK) return r1;
    if (r2 != MAGI_OK) return r2;
    if (o.n_nonfinite) *o.n_nonfinite = count;
    return MAGI_OK;
}

// the checks the two predicting entry points share
int check_predict(magi_handle* h, const char* who, const double* I, int N, int D, const double* phi1, const double* phi2, double nu, const double* mu, int T,
                  const double* t_new, long long S, bool want_draws) {
    if (!I || !phi1 || !phi2 || !t_new) return magi_fail(h, MAGI_E_BADARG, std::string(who) + ": null pointer (I, phi1, phi2 and t_new are required)");
    int rc = check_T(h, who, T);
    if (rc) return rc;
    if (S < 1 || S > (1 << 20)) return magi_fail(h, MAGI_E_BADARG, std::string(who) + ": 1 <= S <= 2^20 draws");
    if (want_draws && S * T * D > (1LL << 28)) return magi_fail(h, MAGI_E_BADARG, std::string(who) + ": x_new / dx_new would exceed 2^28 doubles");
    if ((rc = check_hyper(h, who, D, phi1, phi2, nu))) return rc;
    if ((rc = check_times(h, who, "t_new", t_new, T))) return rc;
    if ((rc = check_times(h, who, "I", I, N))) return rc;
    return check_times(h, who, "mu", mu, D);
}

}  // namespace

int magi_matern_cross(magi_handle* h, const double* t_new, int T, const double* I, int N, double phi1, double phi2, double nu, double* Ks, double* pKs) {
    if (!h) return MAGI_E_BADARG;
    static const char* who = "magi_matern_cross";
    if (!t_new || !I) return magi_fail(h, MAGI_E_BADARG, "magi_matern_cross: null pointer (t_new and I are required)");
    int rc = check_T(h, who, T);
    if (rc) return rc;
    if (N < 1 || N > (1 << 20)) return magi_fail(h, MAGI_E_BADARG, "magi_matern_cross: 1 <= N <= 2^20 grid times");
    if ((long long)T * N > (1LL << 28)) return magi_fail(h, MAGI_E_BADARG, "magi_matern_cross: Ks / pKs would exceed 2^28 doubles");
    if ((rc = check_hyper(h, who, 1, &phi1, &phi2, nu))) return rc;
    if ((rc = check_times(h, who, "t_new", t_new, T))) return rc;
    if ((rc = check_times(h, who, "I", I, N))) return rc;
    (void)hipSetDevice(h->device);
    const size_t tn = (size_t)T * N;
    GpBuf buf{h};
    MAGI_HIP_CHECK(h, hipMalloc((void**)&buf.p, ((size_t)T + N + 2 * tn) * sizeof(double)));
    double *dT = buf.p, *dI = dT + T, *dK = dI + N, *dP = dK + tn;
    MAGI_HIP_CHECK(h, hipMemcpyAsync(dT, t_new, sizeof(double) * T, hipMemcpyHostToDevice, h->stream));
    MAGI_HIP_CHECK(h, hipMemcpyAsync(dI, I, sizeof(double) * N, hipMemcpyHostToDevice, h->stream));
    if ((rc = magi_matern_cross_launch(h, h->stream, dT, T, dI, N, phi1, phi2, nu, Ks ? dK : nullptr, pKs ? dP : nullptr))) return rc;
    if (Ks) MAGI_HIP_CHECK(h, hipMemcpyAsync(Ks, dK, tn * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (pKs) MAGI_HIP_CHECK(h, hipMemcpyAsync(pKs, dP, tn * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    MAGI_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    return MAGI_OK;
}

int magi_gp_predict(magi_handle* h, const double* I, int N, int D, const double* phi1, const double* phi2, double nu, const double* mu, int T,
                    const double* t_new, int S, const double* X, double* x_new, double* dx_new, double* cond_var, double* dcond_var) {
    if (!h) return MAGI_E_BADARG;
    static const char* who = "magi_gp_predict";
    if (N < 2 || D < 1 || D > MAGI_MAX_D) return magi_fail(h, MAGI_E_BADARG, "magi_gp_predict: need N >= 2 and 1 <= D <= " + std::to_string(MAGI_MAX_D));
    if (!mu || !X) return magi_fail(h, MAGI_E_BADARG, "magi_gp_predict: null pointer (mu and X are required)");
    int rc = check_predict(h, who, I, N, D, phi1, phi2, nu, mu, T, t_new, S, x_new || dx_new);
    if (rc) return rc;
    if (!h->dDense[0] || h->dense_N != N || h->dense_D != D)
        return magi_fail(h, MAGI_E_STATE, "magi_gp_predict: no resident matrices of this N, D: build or set them first");
    (void)hipSetDevice(h->device);
    // the draws go up in the caller's layout [S][N][D]: B(n = s, k) of component d at X[s N D + k D + d]
    GpBuf dX{h};
    const size_t nx = (size_t)S * N * D;
    MAGI_HIP_CHECK(h, hipMalloc((void**)&dX.p, nx * sizeof(double)));
    MAGI_HIP_CHECK(h, hipMemcpyAsync(dX.p, X, nx * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const GpDraws dr{dX.p, (long)N * D, (long)D, 1, 1, S};
    GpOut o{};
    o.x_new = x_new; o.dx_new = dx_new; o.cond_var = cond_var; o.dcond_var = dcond_var;
    return gp_core(h, who, h->dDense[0], I, N, D, phi1, phi2, nu, mu, T, t_new, dr, 0, nullptr, 0, o);
}

int magi_sampler_gp_predict(magi_handle* h, int chain0, int n_sel, const double* I, const double* phi1, const double* phi2, double nu, int T,
                            const double* t_new, int n_q, const double* probs, int max_lag, double* x_new, double* dx_new, double* cond_var,
                            double* dcond_var, double* x_mean, double* x_sd, double* x_quant, double* x_rhat, double* x_ess, double* x_mcse_mean,
                            double* dx_mean, double* dx_sd, double* dx_quant, double* dx_rhat, double* dx_ess, double* dx_mcse_mean, int* n_nonfinite) {
    if (!h) return MAGI_E_BADARG;
    static const char* who = "magi_sampler_gp_predict";
    if (!h->sampler_ready) return magi_fail(h, MAGI_E_STATE, "sampler not initialised");
    if (chain0 < 0 || n_sel < 1 || (long long)chain0 + n_sel > h->n_chains)
        return magi_fail(h, MAGI_E_BADARG, "magi_sampler_gp_predict: chains [chain0, chain0 + n_sel) must lie inside the sampler's " + std::to_string(h->n_chains));
    const magi_handle* owner = h;                                  // whose matrices: the handle's, or the member's own on a group
    int member = -1;
    if (h->group_n) {
        const int per = h->group_per > 0 ? h->group_per : h->n_chains;
        member = chain0 / per;
        if ((chain0 + n_sel - 1) / per != member)
            return magi_fail(h, MAGI_E_BADARG, "magi_sampler_gp_predict: the chain range spans more than one member of the group (their posteriors differ)");
        owner = h->members[(size_t)member];
    }
    const DevProblem& pb = h->pb;
    const int R = h->num_results;
    double mu[MAGI_MAX_D] = {};
    for (int d = 0; d < pb.D; ++d) mu[d] = pb.mu[d];
    int rc = check_draws(h, who, n_sel, R);
    if (rc) return rc;
    if (n_q < 0 || n_q > 16) return magi_fail(h, MAGI_E_BADARG, "magi_sampler_gp_predict: 0 <= n_q <= 16 probabilities");
    if (n_q > 0 && !probs) return magi_fail(h, MAGI_E_BADARG, "magi_sampler_gp_predict: probs is NULL");
    for (int q = 0; q < n_q; ++q)
        if (!std::isfinite(probs[q]) || probs[q] < 0.0 || probs[q] > 1.0)
            return magi_fail(h, MAGI_E_BADARG, "magi_sampler_gp_predict: probs[" + std::to_string(q) + "] is not a finite number in [0, 1]");
    (void)hipSetDevice(h->device);
    if (member >= 0) {                                             // the member's problem as the sampler read it (magi_sampler_init)
        DevProblem mp;
        MAGI_HIP_CHECK(h, hipMemcpy(&mp, h->d_members + member, sizeof(DevProblem), hipMemcpyDeviceToHost));
        for (int d = 0; d < pb.D; ++d) mu[d] = mp.mu[d];
    }
    if ((rc = check_predict(h, who, I, pb.N, pb.D, phi1, phi2, nu, mu, T, t_new, (long long)n_sel * R, x_new || dx_new))) return rc;
    if (!owner->dDense[0] || owner->dense_N != pb.N || owner->dense_D != pb.D)
        return magi_fail(h, MAGI_E_STATE, "magi_sampler_gp_predict: no resident dense matrices of the problem's N, D");
    std::vector<ChainCtl> ctl((size_t)n_sel);
    MAGI_HIP_CHECK(h, hipMemcpy(ctl.data(), h->ch.ctl + chain0, sizeof(ChainCtl) * n_sel, hipMemcpyDeviceToHost));
    for (int c = 0; c < n_sel; ++c)
        if (ctl[c].k < h->cfg.total)
            return magi_fail(h, MAGI_E_STATE, "magi_sampler_gp_predict: chain " + std::to_string(chain0 + c) + " has taken " + std::to_string((long long)ctl[c].k) +
                                                  " of " + std::to_string((long long)h->cfg.total) + " transitions");
    // a sample row is [D][N] | sig_pre | th_pre | pad, dimp apart: B(n = s, k) of component d at samples[s dimp + d N + k]
    const GpDraws dr{h->ch.samples + (size_t)chain0 * R * pb.dimp, (long)pb.dimp, 1, (long)pb.N, n_sel, R};
    GpOut o{};
    o.x_new = x_new; o.dx_new = dx_new; o.cond_var = cond_var; o.dcond_var = dcond_var; o.n_nonfinite = n_nonfinite;
    double* const xs[6] = {x_mean, x_sd, x_quant, x_rhat, x_ess, x_mcse_mean};
    double* const dxs[6] = {dx_mean, dx_sd, dx_quant, dx_rhat, dx_ess, dx_mcse_mean};
    for (int i = 0; i < 6; ++i) { o.x[i] = xs[i]; o.dx[i] = dxs[i]; }
    return gp_core(h, who, owner->dDense[0], I, pb.N, pb.D, phi1, phi2, nu, mu, T, t_new, dr, n_q, probs, max_lag, o);
}

int magi_gp_profile(magi_handle* h, double* ms) {
    if (!h || !ms) return MAGI_E_BADARG;
    for (int i = 0; i < 5; ++i) ms[i] = h->gp_ms[i];
    return MAGI_OK;
}
