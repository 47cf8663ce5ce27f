// The host path the two trajectory entry points share (ode.hip: magi_ode_solve, ode_adaptive.hip: magi_ode_solve_adaptive): the checks
// on S, T, t_out and the drift id, and -- per drift -- the scratch, the uploads, the integrator's launch, k_ode_stats, the transpose to
// the host layout, the downloads and the epilogue.  Both integrators write trj[T D][S_pad] with S_pad = roundup(S, MAGI_ODE_PAD) and
// status[S_pad]; the error-controlled ones also reason, n_accepted, n_rejected [S_pad].
#pragma once
#include "scratch.h"

#include <cmath>

struct OdeDev {                       // what an integrator's launch receives
    int S_pad;
    const double *x0, *theta, *t;     // [S][D], [S][P], [T]
    double* trj;                      // [T][D][S_pad]
    int *status, *reason, *n_accepted, *n_rejected;      // [S_pad] each; the last three only where the integrator has them
};

// `specific` holds the entry point's own argument checks: they run between those on T and those on t_out
template <class Specific>
int check_ode_common(magi_handle* h, const char* who, int drift_id, int S, const double* x0, const double* theta, int T, const double* t_out,
                     Specific specific) {
    const std::string me = std::string(who) + ": ";
    if (!x0 || !theta || !t_out) return magi_fail(h, MAGI_E_BADARG, me + "null pointer (x0, theta and t_out are required)");
    if (S < 1 || S > (1 << 20)) return magi_fail(h, MAGI_E_BADARG, me + "1 <= S <= 2^20 draws");
    if (T < 2 || T > (1 << 16)) return magi_fail(h, MAGI_E_BADARG, me + "2 <= T <= 2^16 output times");
    if (int rc = specific()) return rc;
    for (int j = 0; j < T; ++j) {
        if (!std::isfinite(t_out[j])) return magi_fail(h, MAGI_E_BADARG, me + "t_out[" + std::to_string(j) + "] is not finite");
        if (j > 0 && !(t_out[j] > t_out[j - 1])) return magi_fail(h, MAGI_E_BADARG, me + "t_out is not strictly increasing at index " + std::to_string(j));
    }
    return magi_check_drift_id(h, drift_id);
}

// what depends on the drift: P, and the size of the largest device buffer, S_pad * T * D * width cells (width 1: the trajectories; the
// sensitivities of sens.hip have one per column); *S_pad = roundup(S, MAGI_ODE_PAD)
template <class DR>
int check_ode_shape(magi_handle* h, const char* who, int P, int S, int T, int width, size_t* S_pad) {
    const std::string me = std::string(who) + ": ";
    if (P != DR::P) return magi_fail(h, MAGI_E_BADARG, me + "drift expects P=" + std::to_string(DR::P));
    *S_pad = ((size_t)S + MAGI_ODE_PAD - 1) / MAGI_ODE_PAD * MAGI_ODE_PAD;
    if (*S_pad * (size_t)T * DR::D * (size_t)width > ((size_t)1 << 28))
        return magi_fail(h, MAGI_E_BADARG, me + "roundup(S, 64) * T * D" + (width > 1 ? " * n_col" : "") + " exceeds 2^28 (a 2 GiB device buffer)");
    return MAGI_OK;
}

// launch(const OdeDev&) starts the integrator of drift DR on h->stream and returns magi_launch's code; extras: the integrator fills
// reason, n_accepted, n_rejected, downloaded to the three host arrays that are not null
template <class DR, class Launch>
int ode_solve_host(magi_handle* h, const char* who, int P, int S, const double* x0, const double* theta, int T, const double* t_out, double* traj,
                   double* mean, double* sd, int* status, int* n_failed, bool extras, int* reason, int* n_accepted, int* n_rejected, Launch launch) {
    constexpr int D = DR::D;
    size_t S_pad;
    if (int rc = check_ode_shape<DR>(h, who, P, S, T, 1, &S_pad)) return rc;
    const size_t R = (size_t)T * D, cells = S_pad * R;
    const size_t n_out = traj ? (size_t)S * R : 0, nx = (size_t)S * D, nth = (size_t)S * P, ni = (size_t)S * sizeof(int);
    MagiScratch s(h, who);
    double *dtrj, *dout /* the draws in host layout, only when asked for */, *dx, *dth, *dt, *dmean, *dsd;
    int *dstatus, *dreason, *dacc, *drej, *dnf;
    s.take(dtrj, cells); s.take(dout, n_out); s.take(dx, nx); s.take(dth, nth); s.take(dt, (size_t)T); s.take(dmean, R); s.take(dsd, R);
    s.take(dstatus, S_pad); s.take(dreason, extras ? S_pad : 0); s.take(dacc, extras ? S_pad : 0); s.take(drej, extras ? S_pad : 0); s.take(dnf, 1);
    if (int rc = s.alloc()) return rc;
    s.up(dx, x0, nx * sizeof(double));
    s.up(dth, theta, nth * sizeof(double));
    s.up(dt, t_out, (size_t)T * sizeof(double));
    if (s.ok()) s.note(launch(OdeDev{(int)S_pad, dx, dth, dt, dtrj, dstatus, dreason, dacc, drej}));
    if (s.ok() && (mean || sd || n_failed)) s.note(magi_ode_stats(h, S, (int)S_pad, (int)R, dtrj, dstatus, dmean, dsd, dnf));
    if (s.ok() && traj) s.note(magi_ode_transpose(h, S, (int)S_pad, (int)R, dtrj, dout));
    s.down_opt(traj, dout, n_out * sizeof(double));
    s.down_opt(mean, dmean, R * sizeof(double));
    s.down_opt(sd, dsd, R * sizeof(double));
    s.down_opt(status, dstatus, ni);
    if (extras) {
        s.down_opt(reason, dreason, ni);
        s.down_opt(n_accepted, dacc, ni);
        s.down_opt(n_rejected, drej, ni);
    }
    s.down_opt(n_failed, dnf, sizeof(int));
    return s.finish();
}
