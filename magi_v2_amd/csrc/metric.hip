// Diagonal metric of the sampler from a window of states (magi_sampler_adapt_metric, capi.hip).
//
// While a window is open the point phase adds, per chain and entry e of the state vector, the state q_k the chain holds after every
// finished transition to shifted sums (leap_point.h: boundary_block, VOP_ACC):  c = q at the window's start,  S1 = sum (q_k - c),
// S2 = sum (q_k - c)^2.  k_metric_adapt turns the n states of a window into the chain's metric:
//     var_e = (S2_e - S1_e^2 / n) / (n - 1)                                   (>= 0: a rounding residue below zero counts as 0)
//     v_e   = n / (n + kappa) var_e + kappa / (n + kappa) rel_floor med,        med = median_e var_e  (numpy.median: even count -> mean of the two middle ones)
//     s_e   = sqrt(v_e) = sqrt(inverse mass)                                    -> DevChains::scale
// The floor is RELATIVE to the chain's own median variance: the coordinates of this posterior span six orders of magnitude in variance, and
// an absolute floor (Stan's 1e-3 * 5 / (n + 5)) sits three orders above the smallest of them -- it undoes the metric exactly where it matters.
// An entry that never moved (var = 0) gets the floor term alone.  A chain whose median variance is 0 (or whose window holds a non-finite
// state) keeps the metric it has, and the call reports it.
//
// One workgroup per chain; a lane walks the entries e = t, t + 256, ...  The median is an exact order statistic by radix select on the
// bit patterns (variances are >= 0: their bit patterns order as unsigned integers), eight 8-bit passes per rank, as summary.hip selects its
// quantiles.  Runs once per window: nothing here is tuned.
#include "magi_internal.h"

namespace {

constexpr int MA_WG = 256;

// bit pattern of the order statistic of rank `rank` (0-based) among v[0 .. n) (all >= 0 or NaN); every thread returns it
__device__ unsigned long long select_rank(const double* v, int n, int rank, int* hist /* LDS [256] */) {
    unsigned long long prefix = 0, mask = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[threadIdx.x] = 0;                                 // (MA_WG == 256 bins)
        __syncthreads();
        for (int e = threadIdx.x; e < n; e += MA_WG) {
            const unsigned long long key = (unsigned long long)__double_as_longlong(v[e]);
            if ((key & mask) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255)], 1);
        }
        __syncthreads();
        int cum = 0, b = 0;
        for (; b < 255; ++b) {                                 // (the rank lies in one of the bins: b stops at 255 at the latest)
            const int c = hist[b];
            if (cum + c > rank) break;
            cum += c;
        }
        rank -= cum;
        prefix |= (unsigned long long)b << shift;
        mask |= 0xFFull << shift;
        __syncthreads();                                       // (every thread has read hist before it is cleared again)
    }
    return prefix;
}

__global__ __launch_bounds__(MA_WG) void k_metric_adapt(int dim, int dimp, int n_win, double kappa, double rel_floor, const double* __restrict__ macc,
                                                        double* __restrict__ scale, double* __restrict__ work) {
    static_assert(MA_WG == 256, "one thread per histogram bin");
    __shared__ int hist[256];
    __shared__ int s_bad;
    __shared__ unsigned long long s_min;
    const int c = blockIdx.x, t = threadIdx.x;
    const double* m = macc + (size_t)c * 3 * dimp;
    double* var = work + (size_t)c * (dimp + 4);
    double* out = var + dimp;
    double* sc = scale + (size_t)c * dimp;
    if (t == 0) { s_bad = 0; s_min = ~0ull; }
    __syncthreads();
    const double n = (double)n_win;
    int bad = 0;
    for (int e = t; e < dim; e += MA_WG) {
        const double s1 = m[(size_t)dimp + e], s2 = m[(size_t)2 * dimp + e];
        double v = (s2 - s1 * s1 / n) / (n - 1.0);
        v = v > 0.0 ? v : (v == v ? 0.0 : v);                    // (a rounding residue below zero and -0.0, whose bit pattern would sort above every variance, count as +0; NaN stays)
        if (!(v <= 1.7976931348623157e308)) bad = 1;           // NaN or inf: a non-finite state inside the window
        var[e] = v;
    }
    if (bad) atomicOr(&s_bad, 1);
    __syncthreads();                                           // (var[] is complete for the workgroup: global writes of this block, read by it below)
    __threadfence_block();
    const double lo = __longlong_as_double((long long)select_rank(var, dim, (dim - 1) >> 1, hist));
    const double hi = __longlong_as_double((long long)select_rank(var, dim, dim >> 1, hist));
    const double med = 0.5 * (lo + hi);
    const bool keep = s_bad != 0 || !(med > 0.0);
    if (!keep) {
        const double w1 = n / (n + kappa), w0 = kappa / (n + kappa) * rel_floor * med;
        unsigned long long mn = ~0ull;
        for (int e = t; e < dim; e += MA_WG) {
            const double s = sqrt(w1 * var[e] + w0);
            sc[e] = s;
            const unsigned long long key = (unsigned long long)__double_as_longlong(s);       // (s > 0: ordered as its bit pattern)
            mn = key < mn ? key : mn;
        }
        atomicMin(&s_min, mn);
        __syncthreads();
    }
    if (t == 0) {
        out[0] = med;
        out[1] = keep ? 0.0 : __longlong_as_double((long long)s_min);
        out[2] = keep ? 1.0 : 0.0;
        out[3] = 0.0;
    }
}

}  // namespace

int magi_launch_metric_adapt(magi_handle* h, int n_chains, int n_win, double kappa, double rel_floor, const double* macc, double* scale, double* work,
                             hipStream_t s) {
    return magi_launch(h, "metric_adapt launch: ", k_metric_adapt, dim3(n_chains), dim3(MA_WG), s, h->pb.dim, h->pb.dimp, n_win, kappa, rel_floor, macc,
                       scale, work);
}
