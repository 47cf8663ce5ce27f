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
// need no gather; the draws themselves, when the caller wants them, go through k_transpose of summary.hip (magi_transpose) to the host layout [S][T][D].
// The rows of t_new go in chunks so that no buffer exceeds 2^23 doubles (64 MiB, the rule of summary.hip) unless a single row needs
// more; W and Wd of a chunk are formed once and serve every draw.  Nothing depends on the chunking: an output's k loop runs in the same
// order wherever its row falls in a tile, and every row sum runs in one fixed order (lane-strided partials, colstat::wg_sum), so
// the results are bit-identical from run to run and from chunking to chunking.  Does not depend on the drift (jit._DRIFT_FREE).
#include "colstat.h"

#include <cmath>
#include <vector>

namespace {

using namespace colstat;

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

struct GpDraws {                      // the B operand of the application GEMM: B(n = s, k) of component d at base[d bd + s sn + k sk]
    const double* base;               // on the device, or null: gp_core uploads `host` (n_host doubles) into its scratch and reads that
    const double* host;
    size_t n_host;
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

// the whole computation: dCinv the dense C^-1 stack [D][N][N] on the device, I and t_new on the host, the draws on either
int gp_core(magi_handle* h, const char* who, const double* dCinv, const double* I, int N, int D, const double* phi1, const double* phi2, double nu,
            const double* mu, int T, const double* t_new, GpDraws dr, int n_q, const SumProbs& probs, int max_lag, const GpOut& o) {
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

    // scratch: I | t_new | Ks, pKs | W, Wd | shift [2][tc][D] | var [2][T][D] | the x and dx chunks | the staging of the draws on their way to the
    // host | the draws a host caller brought | the statistics' arrays
    MagiScratch s(h, who);
    MagiColStats sx, sdx;
    double *dI, *dT, *ks, *w, *shift, *var, *xc, *st, *dX;
    s.take(dI, (size_t)N); s.take(dT, (size_t)T); s.take(ks, 2 * plane); s.take(w, 2 * plane); s.take(shift, 2 * (size_t)tc * D); s.take(var, 2 * (size_t)T * D);
    s.take(xc, apply ? 2 * cplane : 0); s.take(st, stage ? cplane : 0); s.take(dX, dr.base ? 0 : dr.n_host);
    if (want_x_stats) magi_colstats_take(s, sx, dr.C, dr.R, (long long)T * D, tc * D, n_q, probs, max_lag, o.x[4] || o.x[5], o.x[2] != nullptr);
    if (want_dx_stats) magi_colstats_take(s, sdx, dr.C, dr.R, (long long)T * D, tc * D, n_q, probs, max_lag, o.dx[4] || o.dx[5], o.dx[2] != nullptr);
    if (int rc = s.alloc()) return rc;
    if (!dr.base) {
        s.up(dX, dr.host, dr.n_host * sizeof(double));
        dr.base = dX;
    }
    s.up(dI, I, sizeof(double) * N);
    s.up(dT, t_new, sizeof(double) * T);

    for (int m0 = 0; m0 < T && s.ok(); m0 += tc) {
        const int nt = std::min(tc, T - m0), nc = nt * D;
        // (the planes of a short last chunk are packed at ITS pitch nt: every stride below is in nt)
        const size_t pl = (size_t)D * nt * N, cpl = (size_t)nc * S;
        prof.begin();
        for (int d = 0; d < D && s.ok(); ++d)
            s.note(magi_matern_cross_launch(h, h->stream, dT + m0, nt, dI, N, phi1[d], phi2[d], nu, ks + (size_t)d * nt * N,
                                            deriv ? ks + pl + (size_t)d * nt * N : nullptr));
        prof.end(0);
        if (!s.ok()) break;
        prof.begin();
        MagiGemm g{};           // W_d = Ks_d C^-1_d: rows of Ks times columns of C^-1 as stored, B(n, k) = C^-1[k][n]
        g.A = ks; g.sAm = N; g.sAk = 1; g.batchA = (long)nt * N; g.batchA2 = (long)pl;
        g.B = dCinv; g.sBn = 1; g.sBk = N; g.batchB = (long)N * N; g.batchB2 = 0;
        g.C = w; g.ldc = N; g.batchC = (long)nt * N; g.batchC2 = (long)pl;
        g.M = nt; g.N = N; g.K = N; g.inner = D; g.outer = nz;
        s.note(magi_gemm_strided(h, h->stream, g));
        if (s.ok())
            s.note(magi_launch(h, "k_gp_rows: ", k_gp_rows, dim3((unsigned)nt, (unsigned)D, (unsigned)nz), dim3(SUM_WG), h->stream, nt, N, D, T, m0, (const double*)w,
                               (const double*)ks, cp, var, shift));
        prof.end(1);
        if (!s.ok() || !apply) continue;
        prof.begin();
        MagiGemm a{};           // chunk[(m, d)][s] = sum_k W_d[m][k] B_d(s, k): the draws read in place
        a.A = w; a.sAm = N; a.sAk = 1; a.batchA = (long)nt * N; a.batchA2 = (long)pl;
        a.B = dr.base; a.sBn = dr.sn; a.sBk = dr.sk; a.batchB = dr.bd; a.batchB2 = 0;
        a.C = xc; a.ldc = (long)D * (long)S; a.batchC = (long)S; a.batchC2 = (long)cpl;
        a.M = nt; a.N = (int)S; a.K = N; a.inner = D; a.outer = nz;
        s.note(magi_gemm_strided(h, h->stream, a));
        prof.end(2);
        prof.begin();
        // (shift is [2][nt][D] at this chunk's pitch, the chunk planes [2][nc][S]: one launch adds both)
        if (s.ok())
            s.note(magi_launch(h, "k_gp_shift: ", k_gp_shift, dim3((unsigned)(nz * nc), (unsigned)((S + SUM_WG - 1) / SUM_WG)), dim3(SUM_WG), h->stream, (int)S, xc,
                               (const double*)shift));
        prof.end(3);
        if (!s.ok()) break;
        prof.begin();
        if (want_x_stats) s.note(magi_colstats_chunk(h, who, sx, xc, nc, (long long)m0 * D, MODE_PLAIN, 1, 1));
        if (s.ok() && want_dx_stats) s.note(magi_colstats_chunk(h, who, sdx, xc + cpl, nc, (long long)m0 * D, MODE_PLAIN, 1, 1));
        prof.end(4);
        double* const dst[2] = {o.x_new, o.dx_new};
        for (int z = 0; z < 2 && s.ok(); ++z) {
            if (!dst[z]) continue;
            s.note(magi_transpose(h, nc, (int)S, xc + z * cpl, S, st, (size_t)nc));          // chunk[nc][S] -> st[S][nc]
            if (s.ok())
                s.note(hipMemcpy2DAsync(dst[z] + (size_t)m0 * D, (size_t)T * D * sizeof(double), st, (size_t)nc * sizeof(double), (size_t)nc * sizeof(double), S,
                                        hipMemcpyDeviceToHost, h->stream));
        }
    }
    const size_t vb = (size_t)T * D * sizeof(double);
    s.down_opt(o.cond_var, var, vb);
    s.down_opt(o.dcond_var, var + (size_t)T * D, vb);
    if (want_x_stats) magi_colstats_down(s, sx, o.x[0], o.x[1], o.x[2], o.x[3], o.x[4], o.x[5]);
    if (want_dx_stats) magi_colstats_down(s, sdx, o.dx[0], o.dx[1], o.dx[2], o.dx[3], o.dx[4], o.dx[5]);
    if (int rc = s.finish()) return rc;
    if (o.n_nonfinite) *o.n_nonfinite = (want_x_stats ? sx.n_bad : 0) + (want_dx_stats ? sdx.n_bad : 0);
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
    MagiScratch s(h, who);
    double *dT, *dI, *dK, *dP;
    s.take(dT, (size_t)T); s.take(dI, (size_t)N); s.take(dK, tn); s.take(dP, tn);
    if ((rc = s.alloc())) return rc;
    s.up(dT, t_new, sizeof(double) * T);
    s.up(dI, I, sizeof(double) * N);
    if (s.ok()) s.note(magi_matern_cross_launch(h, h->stream, dT, T, dI, N, phi1, phi2, nu, Ks ? dK : nullptr, pKs ? dP : nullptr));
    s.down_opt(Ks, dK, tn * sizeof(double));
    s.down_opt(pKs, dP, tn * sizeof(double));
    return s.finish();
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
    const GpDraws dr{nullptr, X, (size_t)S * N * D, (long)N * D, (long)D, 1, 1, S};
    GpOut o{};
    o.x_new = x_new; o.dx_new = dx_new; o.cond_var = cond_var; o.dcond_var = dcond_var;
    return gp_core(h, who, h->dDense[0], I, N, D, phi1, phi2, nu, mu, T, t_new, dr, 0, SumProbs{}, 0, o);
}

int magi_sampler_gp_predict(magi_handle* h, int chain0, int n_sel, const double* I, const double* phi1, const double* phi2, double nu, int T,
                            const double* t_new, int n_q, const double* probs, int max_lag, double* x_new, double* dx_new, double* cond_var,
                            double* dcond_var, double* x_mean, double* x_sd, double* x_quant, double* x_rhat, double* x_ess, double* x_mcse_mean,
                            double* dx_mean, double* dx_sd, double* dx_quant, double* dx_rhat, double* dx_ess, double* dx_mcse_mean, int* n_nonfinite) {
    if (!h) return MAGI_E_BADARG;
    static const char* who = "magi_sampler_gp_predict";
    MagiChainRange cr;
    int rc = magi_finished_chains(h, who, chain0, n_sel, &cr);
    if (rc) return rc;
    SumProbs pr;
    if ((rc = check_probs(h, who, n_q, probs, pr))) return rc;
    const magi_handle* owner = cr.member >= 0 ? h->members[(size_t)cr.member] : h;      // whose matrices: the handle's, or the member's own on a group
    const DevProblem& pb = h->pb;                                  // the shapes; mu is cr.pb's: the member's own as the sampler read it
    const int R = cr.R;
    double mu[MAGI_MAX_D] = {};
    for (int d = 0; d < pb.D; ++d) mu[d] = cr.pb.mu[d];
    if ((rc = check_predict(h, who, I, pb.N, pb.D, phi1, phi2, nu, mu, T, t_new, (long long)n_sel * R, x_new || dx_new))) return rc;
    if (!owner->dDense[0] || owner->dense_N != pb.N || owner->dense_D != pb.D)
        return magi_fail(h, MAGI_E_STATE, "magi_sampler_gp_predict: no resident dense matrices of the problem's N, D");
    // a sample row is [D][N] | sig_pre | th_pre | pad, dimp apart: B(n = s, k) of component d at samples[s dimp + d N + k]
    const GpDraws dr{cr.base, nullptr, 0, (long)pb.dimp, 1, (long)pb.N, n_sel, R};
    GpOut o{};
    o.x_new = x_new; o.dx_new = dx_new; o.cond_var = cond_var; o.dcond_var = dcond_var; o.n_nonfinite = n_nonfinite;
    double* const xs[6] = {x_mean, x_sd, x_quant, x_rhat, x_ess, x_mcse_mean};
    double* const dxs[6] = {dx_mean, dx_sd, dx_quant, dx_rhat, dx_ess, dx_mcse_mean};
    for (int i = 0; i < 6; ++i) { o.x[i] = xs[i]; o.dx[i] = dxs[i]; }
    return gp_core(h, who, owner->dDense[0], I, pb.N, pb.D, phi1, phi2, nu, mu, T, t_new, dr, n_q, pr, max_lag, o);
}

int magi_gp_profile(magi_handle* h, double* ms) {
    if (!h || !ms) return MAGI_E_BADARG;
    for (int i = 0; i < 5; ++i) ms[i] = h->gp_ms[i];
    return MAGI_OK;
}
