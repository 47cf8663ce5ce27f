// Drift probe (magi_drift_probe): evaluates THIS library's copy of the drift code by itself, one thread per point, so that the host
// (magi_v2_amd/selftest.py) can hold it against the expressions the code was generated from.  The probe re-derives nothing: every path
// calls the members the production kernels call --
//   path 0: DriftT<>::f, ::jt           (k_point, leap_point.h; k_ti_eval, thetainit.hip)
//   path 1: drift_f, drift_jt_g, drift_tt_g_acc with the drift id as a RUN-TIME value (the three-phase kernels, logpost.hip; for a traced
//           drift they end in user_drift_f / user_drift_jt of the generated header)
//   path 2: DriftT<>::coefs(theta), ::basis(x): f_d = sum_k coefs[d][k] basis[d][k]   (k_stream_sep and its point phase, the mirror)
//   path 3: DriftT<>::f1(d, ..) per component (the VALU / matrix-core streaming kernels; a hand-written body of its own in the compiled-in drifts)
// Depends on the drift: a build for a traced drift compiles this unit again (it is not in jit._DRIFT_FREE).
#include "scratch.h"

namespace {

template <int DRIFT, int PATH>
__global__ __launch_bounds__(256) void k_drift_probe(int drift, int n, const double* __restrict__ xs /* [n][D] */, const double* __restrict__ ths /* [P] */,
                                                     const double* __restrict__ gs /* [n][D] */, double* __restrict__ fo /* [n][D] */,
                                                     double* __restrict__ co /* [n][D] */, double* __restrict__ to /* [n][P] */,
                                                     const double* __restrict__ ts /* [n] time per point, or null: 0 */) {
    using DR = DriftT<DRIFT>;
    constexpr int D = DR::D, P = DR::P;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double tm = ts ? ts[i] : 0.0;
    if constexpr (PATH == 1) {
        double x[MAGI_MAX_D], g[MAGI_MAX_D], th[MAGI_MAX_P], t[MAGI_MAX_P];
#pragma unroll
        for (int k = 0; k < MAGI_MAX_D; ++k) { x[k] = (k < D) ? xs[(size_t)i * D + k] : 0.0; g[k] = (k < D) ? gs[(size_t)i * D + k] : 0.0; }
#pragma unroll
        for (int p = 0; p < MAGI_MAX_P; ++p) { th[p] = (p < P) ? ths[p] : 0.0; t[p] = 0.0; }
#pragma unroll
        for (int d = 0; d < D; ++d) {
            fo[(size_t)i * D + d] = drift_f(drift, d, x, th, tm);
            co[(size_t)i * D + d] = drift_jt_g(drift, d, x, th, g, tm);
        }
        drift_tt_g_acc(drift, x, th, g, t, tm);
#pragma unroll
        for (int p = 0; p < P; ++p) to[(size_t)i * P + p] = t[p];
    } else {
        double x[D], th[P];
#pragma unroll
        for (int k = 0; k < D; ++k) x[k] = xs[(size_t)i * D + k];
#pragma unroll
        for (int p = 0; p < P; ++p) th[p] = ths[p];
        if constexpr (PATH == 0) {
            double g[D], f[D], c[D], t[P];
#pragma unroll
            for (int k = 0; k < D; ++k) g[k] = gs[(size_t)i * D + k];
#pragma unroll
            for (int p = 0; p < P; ++p) t[p] = 0.0;
            drift_f_at<DR>(x, th, tm, f);
            drift_jt_at<DR>(x, th, tm, g, c, t);
#pragma unroll
            for (int k = 0; k < D; ++k) { fo[(size_t)i * D + k] = f[k]; co[(size_t)i * D + k] = c[k]; }
#pragma unroll
            for (int p = 0; p < P; ++p) to[(size_t)i * P + p] = t[p];
        } else if constexpr (PATH == 2) {
            if constexpr (DR::SEP) {
                double ph[D][DR::NBMAX], cf[D][DR::NBMAX];
                drift_basis_at<DR>(x, tm, ph);
                DR::coefs(th, cf);
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    double f = 0.0;
#pragma unroll
                    for (int k = 0; k < DR::NBMAX; ++k) if (k < DR::nbasis(d)) f = fma(cf[d][k], ph[d][k], f);
                    fo[(size_t)i * D + d] = f;
                }
            }
        } else {
#pragma unroll
            for (int d = 0; d < D; ++d) fo[(size_t)i * D + d] = drift_f1_at<DR>(d, x, th, tm);
        }
    }
}

template <int DRIFT>
int probe(magi_handle* h, int drift, int P, int path, int n, const double* x, const double* th, const double* g, double* f, double* c, double* t, const double* tt) {
    using DR = DriftT<DRIFT>;
    constexpr int D = DR::D;
    if (P != DR::P) return magi_fail(h, MAGI_E_BADARG, "drift expects P=" + std::to_string(DR::P));
    if (path == 2 && !DR::SEP) return magi_fail(h, MAGI_E_BADARG, "path 2: this drift has no separable form");
    const bool deriv = path < 2;
    if (deriv && (!g || !c || !t)) return magi_fail(h, MAGI_E_BADARG, "null pointer");
    const size_t nd = (size_t)n * D, np_ = (size_t)n * P;
    MagiScratch s(h, "magi_drift_probe");
    double *dx, *dg, *dout /* f | c (n D each) | t (n P): the outputs, cleared by one memset */, *dth, *dtimes;
    s.take(dx, nd); s.take(dg, nd); s.take(dout, 2 * nd + np_, true); s.take(dth, (size_t)P); s.take(dtimes, tt ? (size_t)n : 0);
    if (int rc = s.alloc()) return rc;
    double *df = dout, *dc = dout + nd, *dt = dout + 2 * nd;
    const double* dtt = tt ? dtimes : nullptr;
    s.up(dx, x, nd * sizeof(double));
    s.up(dth, th, P * sizeof(double));
    if (tt) s.up(dtimes, tt, (size_t)n * sizeof(double));
    if (deriv) s.up(dg, g, nd * sizeof(double));
    if (s.ok()) {
        const dim3 grid((n + 255) / 256), block(256);
        switch (path) {
        case 0: s.note(magi_launch(h, "k_drift_probe: ", k_drift_probe<DRIFT, 0>, grid, block, h->stream, drift, n, dx, dth, dg, df, dc, dt, dtt)); break;
        case 1: s.note(magi_launch(h, "k_drift_probe: ", k_drift_probe<DRIFT, 1>, grid, block, h->stream, drift, n, dx, dth, dg, df, dc, dt, dtt)); break;
        case 2: s.note(magi_launch(h, "k_drift_probe: ", k_drift_probe<DRIFT, 2>, grid, block, h->stream, drift, n, dx, dth, dg, df, dc, dt, dtt)); break;
        default: s.note(magi_launch(h, "k_drift_probe: ", k_drift_probe<DRIFT, 3>, grid, block, h->stream, drift, n, dx, dth, dg, df, dc, dt, dtt)); break;
        }
    }
    s.down(f, df, nd * sizeof(double));
    if (deriv) {
        s.down(c, dc, nd * sizeof(double));
        s.down(t, dt, np_ * sizeof(double));
    }
    return s.finish();
}

}  // namespace

int magi_drift_probe(magi_handle* h, int drift_id, int P, int path, int n, const double* x, const double* th, const double* g,
                     double* f, double* c, double* t) {
    return magi_drift_probe_at(h, drift_id, P, path, n, x, th, g, f, c, t, nullptr);
}

int magi_drift_probe_at(magi_handle* h, int drift_id, int P, int path, int n, const double* x, const double* th, const double* g,
                        double* f, double* c, double* t, const double* tt) {
    if (!h) return MAGI_E_BADARG;
    if (!x || !th || !f) return magi_fail(h, MAGI_E_BADARG, "null pointer");
    if (path < 0 || path > 3) return magi_fail(h, MAGI_E_BADARG, "path: 0 f / jt, 1 runtime-switch entries, 2 separable members, 3 f1");
    if (n < 1 || n > (1 << 20)) return magi_fail(h, MAGI_E_BADARG, "1 <= n <= 2^20 points");
    int rc = magi_check_drift_id(h, drift_id);
    if (rc) return rc;
    (void)hipSetDevice(h->device);
#define MAGI_CALL(DR) rc = probe<DR>(h, drift_id, P, path, n, x, th, g, f, c, t, tt)
    MAGI_DRIFT_DISPATCH(drift_id, MAGI_CALL);
#undef MAGI_CALL
    return rc;
}
