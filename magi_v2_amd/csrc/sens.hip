// Forward sensitivities and Fisher information (magi_ode_sensitivities): the variational equations of THIS library's drift integrated
// beside the state, on the RK4 steps of k_ode_rk4 (ode.hip) restated -- the derivative of the discrete map magi_ode_solve computes.
//   k_ode_sens<DRIFT>  one lane per (draw, column): lanes are draws (64-thread workgroups, S_pad = roundup(S, 64), the lanes past S
//                      integrate a copy of draw S - 1), blockIdx.y is the column, so q = cols[blockIdx.y] is wave-uniform.  A lane
//                      carries x[D], s[D], th[P]; per stage and per component d one drift_jt_at call with the unit vector along d gives
//                      row d of J_x and of df/dtheta, and l[d] = sum_k row[k] z[k] + (q < P ? t[q] : 0) with t[q] picked by a
//                      compare-select chain: every register-array index is a compile-time constant after unrolling, the Jacobian is
//                      never stored.  The state is recomputed per column: that is the price of keeping the 2 D Q wide augmented state
//                      out of one lane.  Column 0 of the launch also writes trj and status, exactly as k_ode_rk4 does.
//                      sens[((j D + d) Q + c) S_pad + s]: the 64 lanes' stores coalesce as those of trj do.
//   k_sens_fim         one lane per draw, one pair a <= b per blockIdx.y: F_ab = sum_k ((w_k / sigma^2) g'^2) s_a s_b over the
//                      observation list in ascending k, written to [a][b] and [b][a]; no atomics.
//   k_sens_fim_flag    one lane per draw: a draw with status != 0 or a non-finite entry gets NaN in all of F and flag 1, so that
//                      k_ode_stats (summary.hip) averages the others in its fixed order and counts the flagged ones.
// Mean and sd of the sensitivities (k_ode_stats with R = T D Q) and the host layouts (k_transpose) are summary.hip's.
// Depends on the drift: a build for a traced drift compiles this unit again (it is not in jit._DRIFT_FREE).
#include "colstat.h"
#include "ode_common.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr int SENS_WG = MAGI_ODE_PAD;          // one wave per workgroup, as k_ode_rk4

// l[d] = sum_k (df_d/dx_k)(tm, y) z[k] + (q < P ? (df_d/dtheta_q)(tm, y) : 0)
template <class DR>
__device__ __forceinline__ void sens_rhs(const double (&y)[DR::D], const double (&th)[DR::P], double tm, const double (&z)[DR::D], int q,
                                         double (&l)[DR::D]) {
    constexpr int D = DR::D, P = DR::P;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        double g[D], row[D], tacc[P];
#pragma unroll
        for (int k = 0; k < D; ++k) g[k] = k == d ? 1.0 : 0.0;
#pragma unroll
        for (int p = 0; p < P; ++p) tacc[p] = 0.0;
        drift_jt_at<DR>(y, th, tm, g, row, tacc);
        double tq = 0.0;
#pragma unroll
        for (int p = 0; p < P; ++p) tq = q == p ? tacc[p] : tq;
        double acc = row[0] * z[0];
#pragma unroll
        for (int k = 1; k < D; ++k) acc += row[k] * z[k];
        l[d] = acc + tq;
    }
}

template <int DRIFT>
__global__ __launch_bounds__(SENS_WG) void k_ode_sens(int S, int S_pad, int T, int substeps, int Q, const int* __restrict__ cols /* [Q] */,
                                                      int relative, const double* __restrict__ x0s /* [S][D] */,
                                                      const double* __restrict__ ths /* [S][P] */, const double* __restrict__ ts /* [T] */,
                                                      double* __restrict__ trj /* [T][D][S_pad] */, double* __restrict__ sens /* [T][D][Q][S_pad] */,
                                                      int* __restrict__ status /* [S_pad] */) {
    using DR = DriftT<DRIFT>;
    constexpr int D = DR::D, P = DR::P;
    const int s = blockIdx.x * SENS_WG + threadIdx.x;         // < S_pad: the grid is S_pad / 64 workgroups wide
    const int c = blockIdx.y;                                 // < Q
    const int q = cols[c];
    const bool first = c == 0;                                // this column's lanes also store the state
    const int src = s < S ? s : S - 1;
    double x[D], z[D], th[P];
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = x0s[(size_t)src * D + d];
#pragma unroll
    for (int p = 0; p < P; ++p) th[p] = ths[(size_t)src * P + p];
    double scale = 1.0;                                       // relative: the draw's own theta_q or x0 component
#pragma unroll
    for (int p = 0; p < P; ++p) scale = (relative && q == p) ? th[p] : scale;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        scale = (relative && q == P + d) ? x[d] : scale;
        z[d] = q == P + d ? 1.0 : 0.0;
    }
    int st = 0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        if (first) trj[(size_t)d * S_pad + s] = x[d];
        sens[((size_t)d * Q + c) * S_pad + s] = z[d] * scale;
    }
    for (int j = 0; j + 1 < T; ++j) {
        const double t0 = ts[j];
        const double h = (ts[j + 1] - t0) / (double)substeps;
        const double hh = 0.5 * h, h6 = h / 6.0;
        for (int k = 0; k < substeps; ++k) {
            const double sk = DR::TDEP ? t0 + (double)k * h : 0.0;
            const double sm = DR::TDEP ? sk + hh : 0.0, se = DR::TDEP ? sk + h : 0.0;
            double k1[D], k2[D], k3[D], k4[D], y[D];
            double l1[D], l2[D], l3[D], l4[D], w[D];
            drift_f_at<DR>(x, th, sk, k1);
            sens_rhs<DR>(x, th, sk, z, q, l1);
#pragma unroll
            for (int d = 0; d < D; ++d) { y[d] = x[d] + hh * k1[d]; w[d] = z[d] + hh * l1[d]; }
            drift_f_at<DR>(y, th, sm, k2);
            sens_rhs<DR>(y, th, sm, w, q, l2);
#pragma unroll
            for (int d = 0; d < D; ++d) { y[d] = x[d] + hh * k2[d]; w[d] = z[d] + hh * l2[d]; }
            drift_f_at<DR>(y, th, sm, k3);
            sens_rhs<DR>(y, th, sm, w, q, l3);
#pragma unroll
            for (int d = 0; d < D; ++d) { y[d] = x[d] + h * k3[d]; w[d] = z[d] + h * l3[d]; }
            drift_f_at<DR>(y, th, se, k4);
            sens_rhs<DR>(y, th, se, w, q, l4);
#pragma unroll
            for (int d = 0; d < D; ++d) {
                x[d] = x[d] + h6 * (k1[d] + 2.0 * k2[d] + 2.0 * k3[d] + k4[d]);
                z[d] = z[d] + h6 * (l1[d] + 2.0 * l2[d] + 2.0 * l3[d] + l4[d]);
            }
        }
        bool fin = true;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (first) trj[((size_t)(j + 1) * D + d) * S_pad + s] = x[d];
            sens[(((size_t)(j + 1) * D + d) * Q + c) * S_pad + s] = z[d] * scale;
            fin = fin && isfinite(x[d]);
        }
        st = (st == 0 && !fin) ? j + 1 : st;                  // as k_ode_rk4: the state alone decides
    }
    if (first) status[s] = st;
}

// grid (S_pad / 64, Q (Q + 1) / 2); links: 2 bits per component
__global__ __launch_bounds__(SENS_WG) void k_sens_fim(int S, int S_pad, int D, int Q, int n_obs, const int* __restrict__ obs_j, const int* __restrict__ obs_d,
                                                      const double* __restrict__ obs_w, const double* __restrict__ sig /* [S][D] */, unsigned links,
                                                      const double* __restrict__ trj /* [T][D][S_pad] */,
                                                      const double* __restrict__ sens /* [T][D][Q][S_pad] */, double* __restrict__ F /* [Q][Q][S_pad] */) {
    const int s = blockIdx.x * SENS_WG + threadIdx.x;
    const int src = s < S ? s : S - 1;
    int a = 0, rest = blockIdx.y;                             // pair index -> (a, b), a <= b, rows of the upper triangle in turn
    while (rest >= Q - a) { rest -= Q - a; ++a; }
    const int b = a + rest;
    double acc = 0.0;
    for (int k = 0; k < n_obs; ++k) {
        const int j = obs_j[k], d = obs_d[k];
        const size_t r = (size_t)j * D + d;
        const double xv = trj[r * S_pad + s];
        const int lk = (links >> (2 * d)) & 3u;
        const double gp = lk == MAGI_LINK_LOG ? 1.0 / xv : lk == MAGI_LINK_SQRT ? 0.5 / sqrt(xv) : 1.0;
        const double cf = (obs_w[k] / sig[(size_t)src * D + d]) * (gp * gp);
        const double sa = sens[(r * Q + a) * S_pad + s], sb = sens[(r * Q + b) * S_pad + s];
        acc += (cf * sa) * sb;
    }
    F[((size_t)a * Q + b) * S_pad + s] = acc;
    F[((size_t)b * Q + a) * S_pad + s] = acc;
}

__global__ __launch_bounds__(SENS_WG) void k_sens_fim_flag(int S_pad, int QQ, const int* __restrict__ status, double* __restrict__ F /* [Q Q][S_pad] */,
                                                           int* __restrict__ flag /* [S_pad] */) {
    const int s = blockIdx.x * SENS_WG + threadIdx.x;         // < S_pad
    bool bad = status[s] != 0;
    for (int e = 0; e < QQ; ++e) bad = bad || !isfinite(F[(size_t)e * S_pad + s]);
    if (bad) {
        const double nan = __builtin_nan("");
        for (int e = 0; e < QQ; ++e) F[(size_t)e * S_pad + s] = nan;
    }
    flag[s] = bad ? 1 : 0;
}

// x0, theta and sigma^2 of the thinned draws of a finished sampler, from its resident sample rows: draw s = (chain s / per, result
// (s % per) thin); x0 = the row's X at grid point i0, theta on its natural scale under the supports and sigma^2 = softplus(sig_pre) + LB
// or the MAGI_PRIOR_FIXED constant, each exactly as k_sum_gather (summary.hip) forms it
__global__ __launch_bounds__(SENS_WG) void k_sens_gather(int S, int R, int per, int thin, int N, int D, int P, int i0, const double* __restrict__ base,
                                                         long long ld, colstat::SumLB lb, const double2* __restrict__ tsup, const double4* __restrict__ prior,
                                                         double* __restrict__ x0 /* [S][D] */, double* __restrict__ th /* [S][P] */,
                                                         double* __restrict__ sig /* [S][D] */) {
    const int s = blockIdx.x * SENS_WG + threadIdx.x;
    if (s >= S) return;
    const double* row = base + ((size_t)(s / per) * R + (size_t)(s % per) * thin) * (size_t)ld;
    const int ND = N * D;
    for (int d = 0; d < D; ++d) {
        x0[(size_t)s * D + d] = row[(size_t)d * N + i0];
        double v = softplus_ref(row[ND + d]) + lb.v[d];
        if (prior) { const double4 pe = prior[d]; if (Prior::fixed(pe)) v = pe.y; }
        sig[(size_t)s * D + d] = v;
    }
    for (int p = 0; p < P; ++p) {
        const double v = row[ND + D + p];
        th[(size_t)s * P + p] = ThetaSup::theta(tsup != nullptr, ThetaSup::load(tsup, p), v, softplus_ref(v));
    }
}

struct SensArgs {
    const char* who;
    int P, S, T, substeps, n_col, relative, n_obs;
    const double *x0, *theta, *t_out;                        // host draws; x0 and theta are not read when `from` is set
    const int *cols, *obs_j, *obs_comp;
    const double *obs_weight, *sigma_sq;
    const int* link;                                         // [D] or null: `links` as given
    unsigned links;
    double *traj, *sens, *sens_mean, *sens_sd, *fim, *fim_mean;
    int *status, *n_failed, *n_fim_excluded;
    // the sampler route: the draws come from the resident samples (k_sens_gather) and may be downloaded as they were used
    const MagiChainRange* from;
    int per, thin, i0;
    double *x0_out, *theta_out, *sigma_sq_out;
};

template <int DRIFT>
int sens_host(magi_handle* h, const SensArgs& a) {
    using DR = DriftT<DRIFT>;
    constexpr int D = DR::D;
    const char* who = a.who;
    const std::string me = std::string(who) + ": ";
    const int S = a.S, T = a.T, P = a.P, Q = a.n_col, n_obs = a.n_obs;
    size_t S_pad;
    if (int rc = check_ode_shape<DR>(h, who, P, S, T, Q < 1 ? 1 : Q, &S_pad)) return rc;
    if (Q < 1 || Q > P + D) return magi_fail(h, MAGI_E_BADARG, me + "1 <= n_col <= P + D = " + std::to_string(P + D));
    if (!a.cols) return magi_fail(h, MAGI_E_BADARG, me + "cols is NULL");
    for (int c = 0; c < Q; ++c) {
        if (a.cols[c] < 0 || a.cols[c] >= P + D) return magi_fail(h, MAGI_E_BADARG, me + "cols[" + std::to_string(c) + "] is outside [0, P + D)");
        for (int e = 0; e < c; ++e)
            if (a.cols[e] == a.cols[c]) return magi_fail(h, MAGI_E_BADARG, me + "cols[" + std::to_string(c) + "] repeats cols[" + std::to_string(e) + "]");
    }
    unsigned links = a.links;
    if (n_obs < 0 || n_obs > (1 << 24)) return magi_fail(h, MAGI_E_BADARG, me + "0 <= n_obs <= 2^24 observations");
    if (n_obs > 0) {
        if (!a.obs_j || !a.obs_comp) return magi_fail(h, MAGI_E_BADARG, me + "obs_j or obs_comp is NULL");
        if (!a.sigma_sq && !a.from) return magi_fail(h, MAGI_E_BADARG, me + "sigma_sq is NULL (n_obs > 0 needs the draws' variances)");
        for (int k = 0; k < n_obs; ++k) {
            if (a.obs_j[k] < 0 || a.obs_j[k] >= T) return magi_fail(h, MAGI_E_BADARG, me + "obs_j[" + std::to_string(k) + "] is outside [0, T)");
            if (a.obs_comp[k] < 0 || a.obs_comp[k] >= D) return magi_fail(h, MAGI_E_BADARG, me + "obs_comp[" + std::to_string(k) + "] is outside [0, D)");
            if (a.obs_weight && (!std::isfinite(a.obs_weight[k]) || !(a.obs_weight[k] > 0.0)))
                return magi_fail(h, MAGI_E_BADARG, me + "obs_weight[" + std::to_string(k) + "] is not a finite number > 0");
        }
        for (size_t i = 0; a.sigma_sq && i < (size_t)S * D; ++i)
            if (!std::isfinite(a.sigma_sq[i]) || !(a.sigma_sq[i] > 0.0))
                return magi_fail(h, MAGI_E_BADARG, me + "sigma_sq[" + std::to_string(i) + "] is not a finite number > 0");
        for (int d = 0; a.link && d < D; ++d) {
            if (a.link[d] < MAGI_LINK_IDENTITY || a.link[d] > MAGI_LINK_SQRT)
                return magi_fail(h, MAGI_E_BADARG, me + "link[" + std::to_string(d) + "] = " + std::to_string(a.link[d]) + " is none of MAGI_LINK_*");
            links |= (unsigned)a.link[d] << (2 * d);
        }
    }
    const bool fisher = n_obs > 0 && (a.fim || a.fim_mean || a.n_fim_excluded);
    const bool want_sig = fisher || (a.from && a.sigma_sq_out);
    const size_t Rx = (size_t)T * D, R = Rx * Q, QQ = (size_t)Q * Q, nx = (size_t)S * D, nth = (size_t)S * P, no = fisher ? (size_t)n_obs : 0;
    const size_t n_traj = a.traj ? (size_t)S * Rx : 0, n_sens = a.sens ? (size_t)S * R : 0, n_fim = fisher && a.fim ? (size_t)S * QQ : 0;
    const bool stats = a.sens_mean || a.sens_sd || a.n_failed;
    std::vector<double> ones;
    if (fisher && !a.obs_weight) ones.assign(no, 1.0);
    MagiScratch s(h, who);
    double *dtrj, *dsens, *dtraj_out, *dsens_out, *dx, *dth, *dt, *dmean, *dsd, *dF, *dF_out, *dFmean, *dFsd, *dw, *dsig;
    int *dcols, *dstatus, *dnf, *dj, *dd, *dflag, *dnex;
    s.take(dtrj, S_pad * Rx); s.take(dsens, S_pad * R); s.take(dtraj_out, n_traj); s.take(dsens_out, n_sens); s.take(dx, nx); s.take(dth, nth);
    s.take(dt, (size_t)T); s.take(dmean, stats ? R : 0); s.take(dsd, stats ? R : 0); s.take(dF, fisher ? S_pad * QQ : 0); s.take(dF_out, n_fim);
    s.take(dFmean, fisher ? QQ : 0); s.take(dFsd, fisher ? QQ : 0); s.take(dw, no); s.take(dsig, want_sig || a.from ? nx : 0);
    s.take(dcols, (size_t)Q); s.take(dstatus, S_pad); s.take(dnf, 1); s.take(dj, no); s.take(dd, no); s.take(dflag, fisher ? S_pad : 0); s.take(dnex, 1);
    if (int rc = s.alloc()) return rc;
    const unsigned gx = (unsigned)(S_pad / SENS_WG);
    if (a.from) {
        const DevProblem& pb = a.from->pb;
        colstat::SumLB lb{};
        for (int d = 0; d < D && d < MAGI_MAX_D; ++d) lb.v[d] = pb.LB[d];
        if (s.ok()) s.note(magi_launch(h, "k_sens_gather: ", k_sens_gather, dim3(gx), dim3(SENS_WG), h->stream, S, a.from->R, a.per, a.thin, pb.N, D, P, a.i0,
                                       a.from->base, (long long)pb.dimp, lb, pb.tsup, pb.prior, dx, dth, dsig));
    } else {
        s.up(dx, a.x0, nx * sizeof(double));
        s.up(dth, a.theta, nth * sizeof(double));
        if (fisher) s.up(dsig, a.sigma_sq, nx * sizeof(double));
    }
    s.up(dt, a.t_out, (size_t)T * sizeof(double));
    s.up(dcols, a.cols, (size_t)Q * sizeof(int));
    if (fisher) {
        s.up(dj, a.obs_j, no * sizeof(int));
        s.up(dd, a.obs_comp, no * sizeof(int));
        s.up(dw, a.obs_weight ? a.obs_weight : ones.data(), no * sizeof(double));
    }
    if (s.ok()) s.note(magi_launch(h, "k_ode_sens: ", k_ode_sens<DRIFT>, dim3(gx, (unsigned)Q), dim3(SENS_WG), h->stream, S, (int)S_pad, T, a.substeps, Q,
                                   (const int*)dcols, a.relative ? 1 : 0, (const double*)dx, (const double*)dth, (const double*)dt, dtrj, dsens, dstatus));
    if (s.ok() && stats) s.note(magi_ode_stats(h, S, (int)S_pad, (int)R, dsens, dstatus, dmean, dsd, dnf));
    if (s.ok() && a.traj) s.note(magi_ode_transpose(h, S, (int)S_pad, (int)Rx, dtrj, dtraj_out));
    if (s.ok() && a.sens) s.note(magi_ode_transpose(h, S, (int)S_pad, (int)R, dsens, dsens_out));
    if (fisher) {
        if (s.ok()) s.note(magi_launch(h, "k_sens_fim: ", k_sens_fim, dim3(gx, (unsigned)(Q * (Q + 1) / 2)), dim3(SENS_WG), h->stream, S, (int)S_pad, D, Q, n_obs,
                                       (const int*)dj, (const int*)dd, (const double*)dw, (const double*)dsig, links, (const double*)dtrj,
                                       (const double*)dsens, dF));
        if (s.ok()) s.note(magi_launch(h, "k_sens_fim_flag: ", k_sens_fim_flag, dim3(gx), dim3(SENS_WG), h->stream, (int)S_pad, (int)QQ, (const int*)dstatus, dF, dflag));
        if (s.ok()) s.note(magi_ode_stats(h, S, (int)S_pad, (int)QQ, dF, dflag, dFmean, dFsd, dnex));
        if (s.ok() && a.fim) s.note(magi_ode_transpose(h, S, (int)S_pad, (int)QQ, dF, dF_out));
        s.down_opt(a.fim, dF_out, n_fim * sizeof(double));
        s.down_opt(a.fim_mean, dFmean, QQ * sizeof(double));
        s.down_opt(a.n_fim_excluded, dnex, sizeof(int));
    }
    if (a.from) {
        s.down_opt(a.x0_out, dx, nx * sizeof(double));
        s.down_opt(a.theta_out, dth, nth * sizeof(double));
        s.down_opt(a.sigma_sq_out, dsig, nx * sizeof(double));
    }
    s.down_opt(a.traj, dtraj_out, n_traj * sizeof(double));
    s.down_opt(a.sens, dsens_out, n_sens * sizeof(double));
    s.down_opt(a.sens_mean, dmean, R * sizeof(double));
    s.down_opt(a.sens_sd, dsd, R * sizeof(double));
    s.down_opt(a.status, dstatus, (size_t)S * sizeof(int));
    s.down_opt(a.n_failed, dnf, sizeof(int));
    return s.finish();
}

int check_substeps(magi_handle* h, const char* who, int substeps) {
    return substeps < 1 || substeps > 1024 ? magi_fail(h, MAGI_E_BADARG, std::string(who) + ": 1 <= substeps <= 1024") : MAGI_OK;
}

}  // namespace

int magi_ode_sensitivities(magi_handle* h, int drift_id, int P, int S, const double* x0, const double* theta, int T, const double* t_out, int substeps,
                           int n_col, const int* cols, int relative, int n_obs, const int* obs_j, const int* obs_comp, const double* obs_weight,
                           const double* sigma_sq, const int* link, double* traj, double* sens, double* sens_mean, double* sens_sd, double* fim,
                           double* fim_mean, int* status, int* n_failed, int* n_fim_excluded) {
    if (!h) return MAGI_E_BADARG;
    static const char* who = "magi_ode_sensitivities";
    int rc = check_ode_common(h, who, drift_id, S, x0, theta, T, t_out, [&] { return check_substeps(h, who, substeps); });
    if (rc) return rc;
    (void)hipSetDevice(h->device);
    SensArgs a{};
    a.who = who; a.P = P; a.S = S; a.T = T; a.substeps = substeps; a.n_col = n_col; a.relative = relative; a.n_obs = n_obs;
    a.x0 = x0; a.theta = theta; a.t_out = t_out; a.cols = cols; a.obs_j = obs_j; a.obs_comp = obs_comp; a.obs_weight = obs_weight;
    a.sigma_sq = sigma_sq; a.link = link;
    a.traj = traj; a.sens = sens; a.sens_mean = sens_mean; a.sens_sd = sens_sd; a.fim = fim; a.fim_mean = fim_mean;
    a.status = status; a.n_failed = n_failed; a.n_fim_excluded = n_fim_excluded;
#define MAGI_CALL(DR) rc = sens_host<DR>(h, a)
    MAGI_DRIFT_DISPATCH(drift_id, MAGI_CALL);
#undef MAGI_CALL
    return rc;
}

int magi_sampler_sensitivities(magi_handle* h, int chain0, int n_sel, int thin, int start_index, int T, const double* t_out, int substeps,
                               const int* grid_out, int n_col, const int* cols, int relative, double* traj, double* sens, double* sens_mean,
                               double* sens_sd, double* fim, double* fim_mean, int* status, int* n_failed, int* n_fim_excluded, int* n_obs_used,
                               int* obs_index, double* x0_out, double* theta_out, double* sigma_sq_out) {
    if (!h) return MAGI_E_BADARG;
    static const char* who = "magi_sampler_sensitivities";
    const std::string me = "magi_sampler_sensitivities: ";
    MagiChainRange cr;
    int rc = magi_finished_chains(h, who, chain0, n_sel, &cr);
    if (rc) return rc;
    const DevProblem& pb = cr.pb;
    if (thin < 1) return magi_fail(h, MAGI_E_BADARG, me + "thin >= 1");
    if (start_index < 0 || start_index >= pb.N) return magi_fail(h, MAGI_E_BADARG, me + "start_index is outside [0, N)");
    const int per = (cr.R + thin - 1) / thin;
    const long long S = (long long)n_sel * per;
    // (the draws are the samples': t_out stands in for the two host arrays the common check wants to see)
    rc = check_ode_common(h, who, pb.drift, S > (1 << 20) ? (1 << 20) + 1 : (int)S, t_out, t_out, T, t_out, [&] { return check_substeps(h, who, substeps); });
    if (rc) return rc;
    std::vector<int> oj, oc, oidx;
    std::vector<double> ow;
    if (grid_out) {
        std::vector<double> y((size_t)pb.ND), w;
        MAGI_HIP_CHECK(h, hipMemcpy(y.data(), pb.yobs, y.size() * sizeof(double), hipMemcpyDeviceToHost));
        if (pb.obsw) {
            w.resize((size_t)pb.ND);
            MAGI_HIP_CHECK(h, hipMemcpy(w.data(), pb.obsw, w.size() * sizeof(double), hipMemcpyDeviceToHost));
        }
        for (int i = 0; i < pb.N; ++i)
            if (grid_out[i] < -1 || grid_out[i] >= T) return magi_fail(h, MAGI_E_BADARG, me + "grid_out[" + std::to_string(i) + "] is outside [-1, T)");
        for (int e = 0; e < pb.ND; ++e)
            if (!std::isnan(y[e]) && grid_out[e % pb.N] >= 0) {
                oidx.push_back(e);
                oj.push_back(grid_out[e % pb.N]);
                oc.push_back(e / pb.N);
                ow.push_back(pb.obsw ? w[e] : 1.0);
            }
    }
    if (n_obs_used) *n_obs_used = (int)oidx.size();
    if (obs_index) std::copy(oidx.begin(), oidx.end(), obs_index);
    SensArgs a{};
    a.who = who; a.P = pb.P; a.S = (int)S; a.T = T; a.substeps = substeps; a.n_col = n_col; a.relative = relative; a.n_obs = (int)oidx.size();
    a.t_out = t_out; a.cols = cols; a.obs_j = oj.data(); a.obs_comp = oc.data(); a.obs_weight = ow.data(); a.links = (unsigned)pb.obs_links;
    a.traj = traj; a.sens = sens; a.sens_mean = sens_mean; a.sens_sd = sens_sd; a.fim = fim; a.fim_mean = fim_mean;
    a.status = status; a.n_failed = n_failed; a.n_fim_excluded = n_fim_excluded;
    a.from = &cr; a.per = per; a.thin = thin; a.i0 = start_index; a.x0_out = x0_out; a.theta_out = theta_out; a.sigma_sq_out = sigma_sq_out;
#define MAGI_CALL(DR) rc = sens_host<DR>(h, a)
    MAGI_DRIFT_DISPATCH(pb.drift, MAGI_CALL);
#undef MAGI_CALL
    return rc;
}
