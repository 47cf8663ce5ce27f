// Posterior trajectories (magi_ode_solve): integrates THIS library's drift -- DriftT<>::f through drift_f_at, the arithmetic the sampler
// ran -- for S draws at once, and summarises them on the device.
//   k_ode_rk4<DRIFT>  one lane per draw, 64-thread workgroups (a draw is a serial chain of drift evaluations: the number of workgroups is
//                     the only parallelism, and 64 threads spread them over four times the CUs 256 would).  x0 and theta live in registers;
//                     classical RK4, `substeps` steps per output interval, the scheme of magi_v2_amd.drift_examples.rk4.  Output j goes to
//                     trj[j][d][s] (S_pad = roundup(S, 64) columns: the 64 lanes' stores coalesce, the lanes past S integrate a copy of draw
//                     S - 1 into the padding, so that no lane has a loop bound or a branch of its own).
// Mean, sd and n_failed (k_ode_stats) and the host layout [S][T D] (k_transpose) do not depend on the drift and live in summary.hip;
// the host path around the kernel is ode_solve_host of ode_common.h, which the error-controlled integrators of ode_adaptive.hip share.
// Depends on the drift: a build for a traced drift compiles this unit again (it is not in jit._DRIFT_FREE).
#include "ode_common.h"

#include <cmath>

namespace {

constexpr int ODE_WG = MAGI_ODE_PAD;          // k_ode_rk4: one wave per workgroup; S_pad = roundup(S, ODE_WG)

template <int DRIFT>
__global__ __launch_bounds__(ODE_WG) void k_ode_rk4(int S, int S_pad, int T, int substeps, const double* __restrict__ x0s /* [S][D] */,
                                                    const double* __restrict__ ths /* [S][P] */, const double* __restrict__ ts /* [T] */,
                                                    double* __restrict__ trj /* [T][D][S_pad] */, int* __restrict__ status /* [S_pad] */) {
    using DR = DriftT<DRIFT>;
    constexpr int D = DR::D, P = DR::P;
    const int s = blockIdx.x * ODE_WG + threadIdx.x;          // < S_pad: the grid is S_pad / 64 workgroups
    const int src = s < S ? s : S - 1;
    double x[D], th[P];
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = x0s[(size_t)src * D + d];
#pragma unroll
    for (int p = 0; p < P; ++p) th[p] = ths[(size_t)src * P + p];
    int st = 0;
#pragma unroll
    for (int d = 0; d < D; ++d) trj[(size_t)d * S_pad + s] = x[d];
    for (int j = 0; j + 1 < T; ++j) {
        const double t0 = ts[j];
        const double h = (ts[j + 1] - t0) / (double)substeps;
        const double hh = 0.5 * h, h6 = h / 6.0;
        for (int k = 0; k < substeps; ++k) {
            // (a drift that does not use t: drift_f_at drops the time, nothing of it is computed)
            const double sk = DR::TDEP ? t0 + (double)k * h : 0.0;
            const double sm = DR::TDEP ? sk + hh : 0.0, se = DR::TDEP ? sk + h : 0.0;
            double k1[D], k2[D], k3[D], k4[D], y[D];
            drift_f_at<DR>(x, th, sk, k1);
#pragma unroll
            for (int d = 0; d < D; ++d) y[d] = x[d] + hh * k1[d];
            drift_f_at<DR>(y, th, sm, k2);
#pragma unroll
            for (int d = 0; d < D; ++d) y[d] = x[d] + hh * k2[d];
            drift_f_at<DR>(y, th, sm, k3);
#pragma unroll
            for (int d = 0; d < D; ++d) y[d] = x[d] + h * k3[d];
            drift_f_at<DR>(y, th, se, k4);
#pragma unroll
            for (int d = 0; d < D; ++d) x[d] = x[d] + h6 * (k1[d] + 2.0 * k2[d] + 2.0 * k3[d] + k4[d]);
        }
        bool fin = true;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            trj[((size_t)(j + 1) * D + d) * S_pad + s] = x[d];
            fin = fin && isfinite(x[d]);
        }
        // interval j is the first with a non-finite output: status j + 1, the index of that output (a non-finite x0 makes output 1
        // non-finite: status 1); the lane goes on regardless
        st = (st == 0 && !fin) ? j + 1 : st;
    }
    status[s] = st;
}

template <int DRIFT>
int solve(magi_handle* h, int P, int S, const double* x0, const double* theta, int T, const double* t_out, int substeps, double* traj,
          double* mean, double* sd, int* status, int* n_failed) {
    return ode_solve_host<DriftT<DRIFT>>(h, "magi_ode_solve", P, S, x0, theta, T, t_out, traj, mean, sd, status, n_failed, false, nullptr, nullptr, nullptr,
                                         [&](const OdeDev& d) {
                                             return magi_launch(h, "k_ode_rk4: ", k_ode_rk4<DRIFT>, dim3((unsigned)(d.S_pad / ODE_WG)), dim3(ODE_WG), h->stream, S,
                                                                d.S_pad, T, substeps, d.x0, d.theta, d.t, d.trj, d.status);
                                         });
}

}  // namespace

int magi_ode_solve(magi_handle* h, int drift_id, int P, int S, const double* x0, const double* theta, int T, const double* t_out, int substeps,
                   double* traj, double* mean, double* sd, int* status, int* n_failed) {
    if (!h) return MAGI_E_BADARG;
    int rc = check_ode_common(h, "magi_ode_solve", drift_id, S, x0, theta, T, t_out, [&] {
        return substeps < 1 || substeps > 1024 ? magi_fail(h, MAGI_E_BADARG, "magi_ode_solve: 1 <= substeps <= 1024") : MAGI_OK;
    });
    if (rc) return rc;
    (void)hipSetDevice(h->device);
#define MAGI_CALL(DR) rc = solve<DR>(h, P, S, x0, theta, T, t_out, substeps, traj, mean, sd, status, n_failed)
    MAGI_DRIFT_DISPATCH(drift_id, MAGI_CALL);
#undef MAGI_CALL
    return rc;
}
