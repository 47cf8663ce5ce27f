// Posterior trajectories (magi_ode_solve): integrates THIS library's drift -- DriftT<>::f through drift_f_at, the arithmetic the sampler
// ran -- for S draws at once, and summarises them on the device.
//   k_ode_rk4<DRIFT>  one lane per draw, 64-thread workgroups (a draw is a serial chain of drift evaluations: the number of workgroups is
//                     the only parallelism, and 64 threads spread them over four times the CUs 256 would).  x0 and theta live in registers;
//                     classical RK4, `substeps` steps per output interval, the scheme of magi_v2_amd.drift_examples.rk4.  Output j goes to
//                     trj[j][d][s] (S_pad = roundup(S, 64) columns: the 64 lanes' stores coalesce, the lanes past S integrate a copy of draw
//                     S - 1 into the padding, so that no lane has a loop bound or a branch of its own).
//   k_ode_stats       mean and sample standard deviation per (j, d) over the draws with status 0: two passes, lane-strided partial sums,
//                     then a butterfly -- one fixed summation order, bit-identical from run to run.
//   k_ode_transpose   trj[T D][S_pad] -> the host layout [S][T D] through an LDS tile; launched only when the caller wants the draws.
// Depends on the drift: a build for a traced drift compiles this unit again (it is not in jit._DRIFT_FREE).
// The error-controlled integrators of csrc/ode_adaptive.hip share the layout and launch k_ode_stats / k_ode_transpose through
// magi_ode_stats / magi_ode_transpose at the end of this file.
#include "magi_internal.h"

#include <cmath>

namespace {

constexpr int ODE_WG = 64;          // k_ode_rk4: one wave per workgroup
constexpr int STATS_WG = 256;
constexpr int TR_TILE = 64;         // k_ode_transpose: 64 x 64 doubles per workgroup of 64 x 4 threads

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

// sum over the workgroup in one fixed order: butterfly inside each wave (every lane ends with the wave's sum), then the four waves' sums
// added as (w0 + w1) + (w2 + w3) by every thread
__device__ __forceinline__ double wg_sum(double v, double* red /* LDS [4] */) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    __syncthreads();                                           // (the previous use of red is over)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(STATS_WG) void k_ode_stats(int S, int S_pad, const double* __restrict__ trj /* [T D][S_pad] */,
                                                        const int* __restrict__ status /* [S_pad] */, double* __restrict__ mean /* [T D] */,
                                                        double* __restrict__ sd /* [T D] */, int* __restrict__ n_failed) {
    __shared__ double red[STATS_WG / 64];
    const double* row = trj + (size_t)blockIdx.x * S_pad;
    double sum = 0.0, cnt = 0.0;
    for (int s = threadIdx.x; s < S; s += STATS_WG) {
        const bool ok = status[s] == 0;
        sum += ok ? row[s] : 0.0;
        cnt += ok ? 1.0 : 0.0;
    }
    sum = wg_sum(sum, red);
    cnt = wg_sum(cnt, red);                                    // (exact: an integer <= 2^20)
    const double nan = __builtin_nan("");
    const double mu = cnt > 0.0 ? sum / cnt : nan;
    double ss = 0.0;
    for (int s = threadIdx.x; s < S; s += STATS_WG) {
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

__global__ __launch_bounds__(TR_TILE * 4) void k_ode_transpose(int S, int S_pad, int R /* T D */, const double* __restrict__ trj /* [R][S_pad] */,
                                                               double* __restrict__ out /* [S][R] */) {
    __shared__ double tile[TR_TILE][TR_TILE + 1];             // (+1: the column reads below fall on 32 different bank pairs)
    const int r0 = blockIdx.y * TR_TILE, c0 = blockIdx.x * TR_TILE, tx = threadIdx.x, ty = threadIdx.y;
    for (int r = ty; r < TR_TILE; r += 4)
        if (r0 + r < R) tile[r][tx] = trj[(size_t)(r0 + r) * S_pad + c0 + tx];        // (c0 + tx < S_pad: S_pad is a multiple of the tile)
    __syncthreads();
    for (int c = ty; c < TR_TILE; c += 4)
        if (c0 + c < S && r0 + tx < R) out[(size_t)(c0 + c) * R + r0 + tx] = tile[tx][c];
}

template <int DRIFT>
int solve(magi_handle* h, int P, int S, const double* x0, const double* theta, int T, const double* t_out, int substeps, double* traj,
          double* mean, double* sd, int* status, int* n_failed) {
    using DR = DriftT<DRIFT>;
    constexpr int D = DR::D;
    if (P != DR::P) return magi_fail(h, MAGI_E_BADARG, "magi_ode_solve: drift expects P=" + std::to_string(DR::P));
    const size_t S_pad = ((size_t)S + ODE_WG - 1) / ODE_WG * ODE_WG, R = (size_t)T * D, cells = S_pad * R;
    if (cells > ((size_t)1 << 28)) return magi_fail(h, MAGI_E_BADARG, "magi_ode_solve: roundup(S, 64) * T * D exceeds 2^28 (a 2 GiB device buffer)");
    const bool stats = mean || sd || n_failed;
    // one device buffer: trj (S_pad T D) | draws in host layout (S T D, only when asked for) | x0 (S D) | theta (S P) | t (T) | mean, sd (T D each)
    // | status (S_pad ints) | n_failed (1 int)
    const size_t n_out = traj ? (size_t)S * R : 0, nx = (size_t)S * D, nth = (size_t)S * P;
    const size_t doubles = cells + n_out + nx + nth + (size_t)T + 2 * R;
    double* buf = nullptr;
    MAGI_HIP_CHECK(h, hipMalloc((void**)&buf, doubles * sizeof(double) + (S_pad + 1) * sizeof(int)));
    double *dtrj = buf, *dout = dtrj + cells, *dx = dout + n_out, *dth = dx + nx, *dt = dth + nth, *dmean = dt + T, *dsd = dmean + R;
    int *dstatus = reinterpret_cast<int*>(dsd + R), *dnf = dstatus + S_pad;
    int rc = MAGI_OK;
    hipError_t e = hipMemcpyAsync(dx, x0, nx * sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dth, theta, nth * sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dt, t_out, (size_t)T * sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess)
        rc = magi_launch(h, "k_ode_rk4: ", k_ode_rk4<DRIFT>, dim3((unsigned)(S_pad / ODE_WG)), dim3(ODE_WG), h->stream, S, (int)S_pad, T, substeps,
                         (const double*)dx, (const double*)dth, (const double*)dt, dtrj, dstatus);
    if (rc == MAGI_OK && e == hipSuccess && stats)
        rc = magi_launch(h, "k_ode_stats: ", k_ode_stats, dim3((unsigned)R), dim3(STATS_WG), h->stream, S, (int)S_pad, (const double*)dtrj,
                         (const int*)dstatus, dmean, dsd, dnf);
    if (rc == MAGI_OK && e == hipSuccess && traj)
        rc = magi_launch(h, "k_ode_transpose: ", k_ode_transpose, dim3((unsigned)(S_pad / TR_TILE), (unsigned)((R + TR_TILE - 1) / TR_TILE)),
                         dim3(TR_TILE, 4), h->stream, S, (int)S_pad, (int)R, (const double*)dtrj, dout);
    const bool ok = rc == MAGI_OK;
    if (ok && e == hipSuccess && traj) e = hipMemcpyAsync(traj, dout, n_out * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (ok && e == hipSuccess && mean) e = hipMemcpyAsync(mean, dmean, R * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (ok && e == hipSuccess && sd) e = hipMemcpyAsync(sd, dsd, R * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (ok && e == hipSuccess && status) e = hipMemcpyAsync(status, dstatus, (size_t)S * sizeof(int), hipMemcpyDeviceToHost, h->stream);
    if (ok && e == hipSuccess && n_failed) e = hipMemcpyAsync(n_failed, dnf, sizeof(int), hipMemcpyDeviceToHost, h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream);          // (also on an error path: nothing may be in flight when the buffer goes)
    (void)hipFree(buf);
    if (rc != MAGI_OK) return rc;
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return magi_fail(h, MAGI_E_HIP, std::string("magi_ode_solve: ") + hipGetErrorString(e));
    return MAGI_OK;
}

}  // namespace

static_assert(ODE_WG == MAGI_ODE_PAD && TR_TILE == MAGI_ODE_PAD, "S_pad = roundup(S, MAGI_ODE_PAD) is what both kernels and the transpose's tiles assume");

int magi_ode_stats(magi_handle* h, int S, int S_pad, int R, const double* trj, const int* status, double* mean, double* sd, int* n_failed) {
    return magi_launch(h, "k_ode_stats: ", k_ode_stats, dim3((unsigned)R), dim3(STATS_WG), h->stream, S, S_pad, trj, status, mean, sd, n_failed);
}

int magi_ode_transpose(magi_handle* h, int S, int S_pad, int R, const double* trj, double* out) {
    return magi_launch(h, "k_ode_transpose: ", k_ode_transpose, dim3((unsigned)(S_pad / TR_TILE), (unsigned)((R + TR_TILE - 1) / TR_TILE)), dim3(TR_TILE, 4),
                       h->stream, S, S_pad, R, trj, out);
}

int magi_ode_solve(magi_handle* h, int drift_id, int P, int S, const double* x0, const double* theta, int T, const double* t_out, int substeps,
                   double* traj, double* mean, double* sd, int* status, int* n_failed) {
    if (!h) return MAGI_E_BADARG;
    if (!x0 || !theta || !t_out) return magi_fail(h, MAGI_E_BADARG, "magi_ode_solve: null pointer (x0, theta and t_out are required)");
    if (S < 1 || S > (1 << 20)) return magi_fail(h, MAGI_E_BADARG, "magi_ode_solve: 1 <= S <= 2^20 draws");
    if (T < 2 || T > (1 << 16)) return magi_fail(h, MAGI_E_BADARG, "magi_ode_solve: 2 <= T <= 2^16 output times");
    if (substeps < 1 || substeps > 1024) return magi_fail(h, MAGI_E_BADARG, "magi_ode_solve: 1 <= substeps <= 1024");
    for (int j = 0; j < T; ++j) {
        if (!std::isfinite(t_out[j])) return magi_fail(h, MAGI_E_BADARG, "magi_ode_solve: t_out[" + std::to_string(j) + "] is not finite");
        if (j > 0 && !(t_out[j] > t_out[j - 1]))
            return magi_fail(h, MAGI_E_BADARG, "magi_ode_solve: t_out is not strictly increasing at index " + std::to_string(j));
    }
#ifdef MAGI_USER_DRIFT_HEADER
    if (drift_id != MAGI_DRIFT_USER) return magi_fail(h, MAGI_E_BADARG, "this library is specialised for a traced f_vec: drift id must be MAGI_DRIFT_USER");
#else
    if (drift_id < MAGI_DRIFT_SEIR3 || drift_id > MAGI_DRIFT_SIRW) return magi_fail(h, MAGI_E_BADARG, "unknown drift id (a traced f_vec needs its own library: magi_v2_amd.jit)");
#endif
    (void)hipSetDevice(h->device);
    int rc = MAGI_OK;
#define MAGI_CALL(DR) rc = solve<DR>(h, P, S, x0, theta, T, t_out, substeps, traj, mean, sd, status, n_failed)
    MAGI_DRIFT_DISPATCH(drift_id, MAGI_CALL);
#undef MAGI_CALL
    return rc;
}
