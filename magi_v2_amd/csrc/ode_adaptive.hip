// Error-controlled posterior trajectories (magi_ode_solve_adaptive): the draws, the layout trj[T][D][S_pad] and the outputs of csrc/ode.hip,
// integrated with a stated tolerance instead of a guessed number of sub-steps.
//   k_ode_adaptive<DRIFT, METHOD>  one lane per draw, 64-thread workgroups, as k_ode_rk4.  Dormand-Prince 5(4), or the Rosenbrock 2(3) pair of
//                     ode23s for stiff draws: its J comes from DriftT<>::jt with unit vectors, its T from DriftT<>::ft (drift_ft_at), and
//                     W = I - h d J is factored in registers.  The controller is stated in include/magi_hip.h and restated op for op in
//                     tests/ode_adaptive_reference.py.  Lanes take different numbers of steps; the wave runs until its last lane is done.
//   mean / sd / n_failed and the host layout: k_ode_stats and k_transpose of csrc/summary.hip (magi_ode_stats, magi_ode_transpose).
// Depends on the drift: not in jit._DRIFT_FREE.
#include "ode_common.h"

#include <cmath>

namespace {

constexpr int ODE_WG = MAGI_ODE_PAD;          // one wave per workgroup

// Every index into a register array below is a compile-time constant after unrolling (the pivot search and the row exchanges are compares
// and selects): nothing goes to scratch.

// 16 ulp(t): the smallest trial step
__device__ __forceinline__ double ode_hmin(double t) {
    const double a = fabs(t);
    return 16.0 * (__longlong_as_double(__double_as_longlong(a) + 1) - a);
}

// LU of W with partial pivoting (the first row of largest |entry| in the column), in place: U on and above the diagonal, the multipliers
// below it, at the rows they had when they were formed (lu_solve replays the exchanges in the same order).  False: a pivot is 0 or not finite.
template <int D>
__device__ __forceinline__ bool lu_factor(double (&W)[D][D], int (&piv)[D]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        int p = k;
        double best = fabs(W[k][k]);
#pragma unroll
        for (int i = k + 1; i < D; ++i) {
            const double a = fabs(W[i][k]);
            const bool g = a > best;
            best = g ? a : best;
            p = g ? i : p;
        }
        piv[k] = p;
#pragma unroll
        for (int i = k + 1; i < D; ++i) {
            const bool sw = p == i;
#pragma unroll
            for (int c = k; c < D; ++c) {
                const double a = W[k][c], b = W[i][c];
                W[k][c] = sw ? b : a;
                W[i][c] = sw ? a : b;
            }
        }
        const double pv = W[k][k];
        ok = ok && pv != 0.0 && isfinite(pv);
#pragma unroll
        for (int i = k + 1; i < D; ++i) {
            const double l = W[i][k] / pv;
            W[i][k] = l;
#pragma unroll
            for (int c = k + 1; c < D; ++c) W[i][c] = W[i][c] - l * W[k][c];
        }
    }
    return ok;
}

// b <- W^-1 b through the factors of lu_factor
template <int D>
__device__ __forceinline__ void lu_solve(const double (&W)[D][D], const int (&piv)[D], double (&b)[D]) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
#pragma unroll
        for (int i = k + 1; i < D; ++i) {
            const bool sw = piv[k] == i;
            const double a = b[k], c = b[i];
            b[k] = sw ? c : a;
            b[i] = sw ? a : c;
        }
#pragma unroll
        for (int i = k + 1; i < D; ++i) b[i] = b[i] - W[i][k] * b[k];
    }
#pragma unroll
    for (int k = D - 1; k >= 0; --k) {
        double s = b[k];
#pragma unroll
        for (int c = k + 1; c < D; ++c) s = s - W[k][c] * b[c];
        b[k] = s / W[k][k];
    }
}

// One trial step of Dormand-Prince 5(4) from (t, x) with k1 = f(t, x): the 5th-order state xn, its drift k7 = f(tn, xn) (FSAL) and
// err = ht sum (b_i - b*_i) k_i.
template <class DR>
__device__ __forceinline__ void dopri5_trial(const double (&x)[DR::D], const double (&th)[DR::P], const double (&k1)[DR::D], double t, double ht,
                                             double tn, double (&xn)[DR::D], double (&k7)[DR::D], double (&err)[DR::D]) {
    constexpr int D = DR::D;
    double k2[D], k3[D], k4[D], k5[D], k6[D], y[D];
#pragma unroll
    for (int d = 0; d < D; ++d) y[d] = x[d] + ht * ((1.0 / 5.0) * k1[d]);
    drift_f_at<DR>(y, th, t + (1.0 / 5.0) * ht, k2);
#pragma unroll
    for (int d = 0; d < D; ++d) y[d] = x[d] + ht * ((3.0 / 40.0) * k1[d] + (9.0 / 40.0) * k2[d]);
    drift_f_at<DR>(y, th, t + (3.0 / 10.0) * ht, k3);
#pragma unroll
    for (int d = 0; d < D; ++d) y[d] = x[d] + ht * ((44.0 / 45.0) * k1[d] + (-56.0 / 15.0) * k2[d] + (32.0 / 9.0) * k3[d]);
    drift_f_at<DR>(y, th, t + (4.0 / 5.0) * ht, k4);
#pragma unroll
    for (int d = 0; d < D; ++d)
        y[d] = x[d] + ht * ((19372.0 / 6561.0) * k1[d] + (-25360.0 / 2187.0) * k2[d] + (64448.0 / 6561.0) * k3[d] + (-212.0 / 729.0) * k4[d]);
    drift_f_at<DR>(y, th, t + (8.0 / 9.0) * ht, k5);
#pragma unroll
    for (int d = 0; d < D; ++d)
        y[d] = x[d] + ht * ((9017.0 / 3168.0) * k1[d] + (-355.0 / 33.0) * k2[d] + (46732.0 / 5247.0) * k3[d] + (49.0 / 176.0) * k4[d] +
                            (-5103.0 / 18656.0) * k5[d]);
    drift_f_at<DR>(y, th, tn, k6);
#pragma unroll
    for (int d = 0; d < D; ++d)
        xn[d] = x[d] + ht * ((35.0 / 384.0) * k1[d] + (500.0 / 1113.0) * k3[d] + (125.0 / 192.0) * k4[d] + (-2187.0 / 6784.0) * k5[d] +
                             (11.0 / 84.0) * k6[d]);
    drift_f_at<DR>(xn, th, tn, k7);
    // b - b*: 71/57600, 0, -71/16695, 71/1920, -17253/339200, 22/525, -1/40
#pragma unroll
    for (int d = 0; d < D; ++d)
        err[d] = ht * ((71.0 / 57600.0) * k1[d] + (-71.0 / 16695.0) * k3[d] + (71.0 / 1920.0) * k4[d] + (-17253.0 / 339200.0) * k5[d] +
                       (22.0 / 525.0) * k6[d] + (-1.0 / 40.0) * k7[d]);
}

// One trial step of the Shampine-Reichelt Rosenbrock 2(3) pair from (t, x) with F0 = f(t, x): xn, F2 = f(tn, xn) (FSAL) and err.  J row i
// is jt with g = e_i (the theta accumulator is dead code); J and T are formed again on a retried step, which keeps W the only matrix held
// in registers.  False: W is singular.
template <class DR>
__device__ __forceinline__ bool ros23_trial(const double (&x)[DR::D], const double (&th)[DR::P], const double (&F0)[DR::D], double t, double ht,
                                            double tn, double (&xn)[DR::D], double (&F2)[DR::D], double (&err)[DR::D]) {
    constexpr int D = DR::D, P = DR::P;
    const double dd = 1.0 / (2.0 + 1.4142135623730951), e32 = 6.0 + 1.4142135623730951;
    const double hd = ht * dd;
    double W[D][D];
    int piv[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double g[D], c[D], tacc[P];
#pragma unroll
        for (int k = 0; k < D; ++k) g[k] = k == i ? 1.0 : 0.0;
#pragma unroll
        for (int p = 0; p < P; ++p) tacc[p] = 0.0;
        drift_jt_at<DR>(x, th, t, g, c, tacc);
#pragma unroll
        for (int k = 0; k < D; ++k) W[i][k] = (k == i ? 1.0 : 0.0) - hd * c[k];
    }
    double Tv[D];
    drift_ft_at<DR>(x, th, t, Tv);
    const bool ok = lu_factor<D>(W, piv);
    double k1[D], k2[D], k3[D], F1[D], y[D];
#pragma unroll
    for (int d = 0; d < D; ++d) k1[d] = F0[d] + hd * Tv[d];
    lu_solve<D>(W, piv, k1);
#pragma unroll
    for (int d = 0; d < D; ++d) y[d] = x[d] + (0.5 * ht) * k1[d];
    drift_f_at<DR>(y, th, t + 0.5 * ht, F1);
#pragma unroll
    for (int d = 0; d < D; ++d) k2[d] = F1[d] - k1[d];
    lu_solve<D>(W, piv, k2);
#pragma unroll
    for (int d = 0; d < D; ++d) {
        k2[d] = k2[d] + k1[d];
        xn[d] = x[d] + ht * k2[d];
    }
    drift_f_at<DR>(xn, th, tn, F2);
#pragma unroll
    for (int d = 0; d < D; ++d) k3[d] = ((F2[d] - e32 * (k2[d] - F1[d])) - 2.0 * (k1[d] - F0[d])) + hd * Tv[d];
    lu_solve<D>(W, piv, k3);
#pragma unroll
    for (int d = 0; d < D; ++d) err[d] = (ht / 6.0) * ((k1[d] - 2.0 * k2[d]) + k3[d]);
    return ok;
}

// One lane per draw as k_ode_rk4; lanes take different numbers of steps, the wave runs until its last lane is done.  METHOD: MAGI_ODE_DOPRI5
// or MAGI_ODE_ROS23.
template <int DRIFT, int METHOD>
__global__ __launch_bounds__(ODE_WG) void k_ode_adaptive(int S, int S_pad, int T, double rtol, double atol, double h0, int max_steps,
                                                         const double* __restrict__ x0s /* [S][D] */, const double* __restrict__ ths /* [S][P] */,
                                                         const double* __restrict__ ts /* [T] */, double* __restrict__ trj /* [T][D][S_pad] */,
                                                         int* __restrict__ status /* [S_pad] */, int* __restrict__ reason /* [S_pad] */,
                                                         int* __restrict__ n_acc /* [S_pad] */, int* __restrict__ n_rej /* [S_pad] */) {
    using DR = DriftT<DRIFT>;
    constexpr int D = DR::D, P = DR::P;
    constexpr double EXPO = METHOD == MAGI_ODE_DOPRI5 ? -1.0 / 5.0 : -1.0 / 3.0;
    const int s = blockIdx.x * ODE_WG + threadIdx.x;          // < S_pad
    const int src = s < S ? s : S - 1;
    double x[D], th[P], F0[D];
    bool fin = true;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        x[d] = x0s[(size_t)src * D + d];
        fin = fin && isfinite(x[d]);
        trj[(size_t)d * S_pad + s] = x[d];
    }
#pragma unroll
    for (int p = 0; p < P; ++p) th[p] = ths[(size_t)src * P + p];
    double t = ts[0];
    double h = h0 > 0.0 ? h0 : ts[1] - t;
    int j = 0, na = 0, nr = 0, st = fin ? 0 : 1, rs = fin ? 0 : 1;
    bool rejected = false;
    drift_f_at<DR>(x, th, t, F0);
    while (rs == 0 && j + 1 < T) {
        const double tend = ts[j + 1];
        const double rem = tend - t;
        const bool clip = rem - h < ode_hmin(tend);           // (h >= rem, or what h would leave of the interval is less than a step)
        const double ht = clip ? rem : h;
        if (na + nr >= max_steps) { rs = 2; st = j + 1; break; }
        if (ht < ode_hmin(t)) { rs = 3; st = j + 1; break; }
        const double tn = clip ? tend : t + ht;
        double xn[D], Fn[D], err[D];
        bool ok = true;
        if constexpr (METHOD == MAGI_ODE_DOPRI5) dopri5_trial<DR>(x, th, F0, t, ht, tn, xn, Fn, err);
        else ok = ros23_trial<DR>(x, th, F0, t, ht, tn, xn, Fn, err);
        double errn = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double r = fabs(err[d]) / (atol + rtol * fmax(fabs(x[d]), fabs(xn[d])));
            ok = ok && isfinite(r) && isfinite(xn[d]);
            errn = fmax(errn, r);
        }
        if (!ok) {                                            // a non-finite trial or a singular W
            ++nr;
            h = ht * 0.2;
            rejected = true;
            continue;
        }
        double fac = errn == 0.0 ? 5.0 : fmin(5.0, fmax(0.2, 0.9 * pow(errn, EXPO)));
        if (errn <= 1.0) {
            ++na;
            fac = rejected ? fmin(fac, 1.0) : fac;
            const double hn = ht * fac;
            h = clip ? fmax(h, hn) : hn;
            rejected = false;
            t = tn;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                x[d] = xn[d];
                F0[d] = Fn[d];
            }
            if (clip) {
                ++j;
#pragma unroll
                for (int d = 0; d < D; ++d) trj[((size_t)j * D + d) * S_pad + s] = x[d];
            }
        } else {
            ++nr;
            h = ht * fmin(fac, 1.0);
            rejected = true;
        }
    }
    if (rs != 0) {                                            // the outputs this draw did not reach
        const double nan = __builtin_nan("");
        for (int jj = j + 1; jj < T; ++jj)
#pragma unroll
            for (int d = 0; d < D; ++d) trj[((size_t)jj * D + d) * S_pad + s] = nan;
    }
    status[s] = st;
    reason[s] = rs;
    n_acc[s] = na;
    n_rej[s] = nr;
}

// magi_ode_solve_adaptive for one drift: the host path of magi_ode_solve (ode_common.h) with reason, n_accepted, n_rejected behind status
template <int DRIFT>
int solve_adaptive(magi_handle* h, int P, int S, const double* x0, const double* theta, int T, const double* t_out, int method, double rtol,
                   double atol, double h0, int max_steps, double* traj, double* mean, double* sd, int* status, int* reason, int* n_accepted,
                   int* n_rejected, int* n_failed) {
    return ode_solve_host<DriftT<DRIFT>>(
        h, "magi_ode_solve_adaptive", P, S, x0, theta, T, t_out, traj, mean, sd, status, n_failed, true, reason, n_accepted, n_rejected, [&](const OdeDev& d) {
            const dim3 grid((unsigned)(d.S_pad / ODE_WG)), wg(ODE_WG);
            if (method == MAGI_ODE_DOPRI5)
                return magi_launch(h, "k_ode_adaptive (dopri5): ", k_ode_adaptive<DRIFT, MAGI_ODE_DOPRI5>, grid, wg, h->stream, S, d.S_pad, T, rtol, atol, h0,
                                   max_steps, d.x0, d.theta, d.t, d.trj, d.status, d.reason, d.n_accepted, d.n_rejected);
            return magi_launch(h, "k_ode_adaptive (ros23): ", k_ode_adaptive<DRIFT, MAGI_ODE_ROS23>, grid, wg, h->stream, S, d.S_pad, T, rtol, atol, h0, max_steps,
                               d.x0, d.theta, d.t, d.trj, d.status, d.reason, d.n_accepted, d.n_rejected);
        });
}

}  // namespace

int magi_ode_solve_adaptive(magi_handle* h, int drift_id, int P, int S, const double* x0, const double* theta, int T, const double* t_out, int method,
                            double rtol, double atol, double h0, int max_steps, double* traj, double* mean, double* sd, int* status, int* reason,
                            int* n_accepted, int* n_rejected, int* n_failed) {
    if (!h) return MAGI_E_BADARG;
    int rc = check_ode_common(h, "magi_ode_solve_adaptive", drift_id, S, x0, theta, T, t_out, [&] {
        const std::string me = "magi_ode_solve_adaptive: ";
        if (method != MAGI_ODE_DOPRI5 && method != MAGI_ODE_ROS23)
            return magi_fail(h, MAGI_E_BADARG, me + "unknown method (MAGI_ODE_DOPRI5 or MAGI_ODE_ROS23)");
        if (!std::isfinite(rtol) || !std::isfinite(atol)) return magi_fail(h, MAGI_E_BADARG, me + "rtol and atol must both be finite");
        if (rtol < 1e-13 || rtol > 1e-1) return magi_fail(h, MAGI_E_BADARG, me + "1e-13 <= rtol <= 1e-1");
        if (atol < 0.0) return magi_fail(h, MAGI_E_BADARG, me + "atol >= 0");
        if (!std::isfinite(h0) || h0 < 0.0) return magi_fail(h, MAGI_E_BADARG, me + "h0 >= 0 and finite (0: the first output interval)");
        if (max_steps < 1 || max_steps > (1 << 24)) return magi_fail(h, MAGI_E_BADARG, me + "1 <= max_steps <= 2^24");
        return (int)MAGI_OK;
    });
    if (rc) return rc;
    (void)hipSetDevice(h->device);
#define MAGI_CALL(DR) \
    rc = solve_adaptive<DR>(h, P, S, x0, theta, T, t_out, method, rtol, atol, h0, max_steps, traj, mean, sd, status, reason, n_accepted, n_rejected, n_failed)
    MAGI_DRIFT_DISPATCH(drift_id, MAGI_CALL);
#undef MAGI_CALL
    return rc;
}
