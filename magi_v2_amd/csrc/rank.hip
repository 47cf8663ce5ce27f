// Rank-normalised convergence diagnostics (magi_rank_diagnostics, magi_sampler_rank_diagnostics): per scalar column of C chains x R draws
// the rank-normalised split R-hat, the bulk ESS and the tail ESS of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021) -- definitions in
// include/magi_hip.h and DESIGN.md 4.4b.  Works on the chunks chunk[column][S], S = C R, that summary.hip's k_sum_gather produces:
//   k_rank_sort     one workgroup per column: non-finite detection, then a key sort of the column into a second buffer.  The network is the
//                   bitonic sorter in its one-direction form (every compare-exchange puts the smaller key at the lower index: the first step
//                   of a merge pairs i with i ^ (k - 1), the others i with i ^ j), so the padding to a power of two is virtual -- a pair
//                   whose upper index is >= S is skipped -- and a column of any S sorts in S keys.  S <= RANK_LDS: in LDS.  Larger: tiles of
//                   RANK_LDS keys are sorted in LDS, then every merge runs its strides >= RANK_LDS in global memory and the rest in LDS,
//                   tile by tile.
//   k_rank_rank     per draw its lower and upper bound in the sorted column by value (binary search: -0.0 == +0.0 are tied although their
//                   keys differ) -> the 1-based average rank (lower + upper + 1) / 2, exact.
//   k_rank_z        in place: z = phi_inv((rank - 3/8) / (S + 1/4)).
//   k_rank_fill     the other derived series from the sorted column: the two tail indicators y <= v[floor((S - 1) p)], and the folded draws
//                   |y - med| with med the quantile of summary.hip at p = 0.5.
//   k_rank_combine  max / min over the legs with the NaN rules, written at out_index(mode, ..).
// R-hat and ESS of the four derived series are summary.hip's own (magi_colstats_take / _chunk: k_sum_moments, k_sum_ess), so every sum runs
// in that unit's fixed order; the only atomic here is the integer count of non-finite columns: results are bit-identical from run to run
// and do not depend on the chunking.  Does not depend on the drift (jit._DRIFT_FREE).
#include "colstat.h"

#include <cmath>

namespace {

using namespace colstat;

// keys a workgroup sorts in LDS: 64 KiB, so two workgroups (8 waves) share a CU's 160 KiB -- while one waits at a step's barrier the
// other exchanges -- and 8 chains x 1000 draws, the largest column of the benchmark shapes, still sort without a pass over global memory
constexpr int RANK_LDS = 8192;
constexpr int RANK_LDS_LOG = 13;
static_assert(1 << RANK_LDS_LOG == RANK_LDS, "a power of two: the tiles of the large sort are aligned blocks of the network");

// Inverse of the standard normal CDF at 0 < p < 1, to a few units of the last place of max(1, |x|).  Works on the lower tail mass
// pl = min(p, 1 - p) (1 - p is exact for p >= 1/2): the start of Abramowitz & Stegun 26.2.23 (absolute error < 4.5e-4), then three Halley
// steps on Phi(x) - pl, which triple the digits each.  Phi(x) is erfc(-x / sqrt 2) / 2 where pl <= 1/4; nearer the centre that difference
// would cancel, and the steps run on erf(x / sqrt 2) / 2 - (pl - 1/2) instead (pl - 1/2 is exact), whose error is relative to x.
__device__ inline double phi_inv(double p) {
    const double q = p - 0.5;
    if (q == 0.0) return 0.0;
    const double pl = q < 0.0 ? p : 1.0 - p;
    const double qa = fabs(q);
    const bool central = qa <= 0.25;
    const double t = sqrt(-2.0 * log(pl));
    double x = (2.515517 + t * (0.802853 + t * 0.010328)) / (1.0 + t * (1.432788 + t * (0.189269 + t * 0.001308))) - t;      // (x <= 0)
#pragma unroll 1
    for (int it = 0; it < 3; ++it) {
        const double dens = 0.3989422804014327 * exp(-0.5 * x * x);
        const double f = central ? 0.5 * erf(x * 0.7071067811865476) + qa : 0.5 * erfc(-x * 0.7071067811865476) - pl;
        const double u = f / dens;
        x -= u / (1.0 + 0.5 * x * u);
    }
    return q < 0.0 ? x : -x;
}

// one step of the sorting network over the n keys v[0 .. n): pair t has its lower index at bits (t >> lh, 0, t & (h - 1)), h = 2^lh, and its
// upper index h above it (flip: mirrored inside the block of 2 h instead).  The lower index grows with t, so a thread leaves at its first
// pair that starts beyond n; a pair whose upper index is beyond n would exchange with the virtual padding, the largest key: skipped.
template <class Cmpx>
__device__ __forceinline__ void net_step(int n, int lh, bool flip, Cmpx cmpx) {
    const int h = 1 << lh;
    for (int t = threadIdx.x;; t += SUM_WG) {
        const int off = t & (h - 1), i = ((t >> lh) << (lh + 1)) + off;
        if (i >= n) break;
        const int l = flip ? i + 2 * (h - off) - 1 : i + h;
        if (l < n) cmpx(i, l);
    }
}

// the steps of block size 2^lk0 .. (flip first) or, merge_only, the strides 2^(lk0 - 1) .. 1 of one merge, on the n keys in LDS
__device__ __forceinline__ void lds_net(unsigned long long* key, int n, int lk0, bool merge_only) {
    auto cmpx = [key](int i, int l) {
        const unsigned long long a = key[i], b = key[l];
        if (a > b) { key[i] = b; key[l] = a; }
    };
    if (merge_only) {
        for (int lh = lk0 - 1; lh >= 0; --lh) {
            net_step(n, lh, false, cmpx);
            __syncthreads();
        }
        return;
    }
    for (int lk = lk0; (1 << (lk - 1)) < n; ++lk) {
        net_step(n, lk - 1, true, cmpx);
        __syncthreads();
        for (int lh = lk - 2; lh >= 0; --lh) {
            net_step(n, lh, false, cmpx);
            __syncthreads();
        }
    }
}

// flag[column] = 1: a non-finite draw (first: detected and counted here; else read)
__global__ __launch_bounds__(SUM_WG) void k_rank_sort(int S, const double* __restrict__ src /* [nc][S] */, double* __restrict__ dst /* [nc][S] */,
                                                      int* __restrict__ flag, int first, int* __restrict__ n_nonfinite) {
    __shared__ unsigned long long key[RANK_LDS];
    const int tid = threadIdx.x;
    const double* row = src + (size_t)blockIdx.x * S;
    double* out = dst + (size_t)blockIdx.x * S;
    if (first) {
        int bad = 0;
        for (int e = tid; e < S; e += SUM_WG) bad |= !isfinite(row[e]);
        bad = __syncthreads_or(bad);
        if (tid == 0) {
            flag[blockIdx.x] = bad ? 1 : 0;
            if (bad) atomicAdd(n_nonfinite, 1);
        }
        if (bad) return;
    } else if (flag[blockIdx.x]) return;                       // (uniform over the workgroup)
    // tiles of RANK_LDS keys, each sorted in LDS (a column that fits is its one tile)
    for (int t0 = 0; t0 < S; t0 += RANK_LDS) {
        const int n = min(RANK_LDS, S - t0);
        for (int e = tid; e < n; e += SUM_WG) key[e] = to_key(row[t0 + e]);
        __syncthreads();
        lds_net(key, n, 1, false);
        for (int e = tid; e < n; e += SUM_WG) out[t0 + e] = from_key(key[e]);
        __syncthreads();                                       // (key is refilled; the stores are visible to the workgroup below)
    }
    if (S <= RANK_LDS) return;
    auto gcmpx = [out](int i, int l) {
        const double a = out[i], b = out[l];
        if (to_key(a) > to_key(b)) { out[i] = b; out[l] = a; }
    };
    for (int lk = RANK_LDS_LOG + 1; (1 << (lk - 1)) < S; ++lk) {      // (S <= 2^22: lk <= 22)
        net_step(S, lk - 1, true, gcmpx);
        __syncthreads();
        for (int lh = lk - 2; lh >= RANK_LDS_LOG; --lh) {
            net_step(S, lh, false, gcmpx);
            __syncthreads();
        }
        for (int t0 = 0; t0 < S; t0 += RANK_LDS) {
            const int n = min(RANK_LDS, S - t0);
            for (int e = tid; e < n; e += SUM_WG) key[e] = to_key(out[t0 + e]);
            __syncthreads();
            lds_net(key, n, RANK_LDS_LOG, true);
            for (int e = tid; e < n; e += SUM_WG) out[t0 + e] = from_key(key[e]);
            __syncthreads();
        }
    }
}

// grid (nc, ceil(S / SUM_WG)).  y and rank may be the same array (the folded series is ranked in place).
__global__ __launch_bounds__(SUM_WG) void k_rank_rank(int S, const double* y /* [nc][S] */, const double* __restrict__ sorted /* [nc][S] */,
                                                      const int* __restrict__ flag, double* rank /* [nc][S] */) {
    const int s = blockIdx.y * SUM_WG + threadIdx.x;
    if (s >= S) return;
    const size_t at = (size_t)blockIdx.x * S + s;
    if (flag[blockIdx.x]) { rank[at] = __builtin_nan(""); return; }
    const double* v = sorted + (size_t)blockIdx.x * S;
    const double x = y[at];
    int lo = 0, n = S;                                         // lo: the draws < x
    while (n > 0) {
        const int half = n >> 1;
        if (v[lo + half] < x) { lo += half + 1; n -= half + 1; }
        else n = half;
    }
    int hi = lo + 1;                                           // hi: the draws <= x (x itself is one of them: v[lo] == x)
    if (hi < S && v[hi] <= x) {
        n = S - hi;
        while (n > 0) {
            const int half = n >> 1;
            if (v[hi + half] <= x) { hi += half + 1; n -= half + 1; }
            else n = half;
        }
    }
    rank[at] = 0.5 * (double)(lo + hi + 1);
}

__global__ __launch_bounds__(SUM_WG) void k_rank_z(int S, const int* __restrict__ flag, double* __restrict__ w /* [nc][S]: rank -> z */) {
    const int s = blockIdx.y * SUM_WG + threadIdx.x;
    if (s >= S || flag[blockIdx.x]) return;                    // (a flagged column holds NaN already)
    const size_t at = (size_t)blockIdx.x * S + s;
    w[at] = phi_inv((w[at] - 0.375) / ((double)S + 0.25));
}

// which 0: the indicator y <= v[floor((S - 1) p)]; 1: the folded draws |y - med|
__global__ __launch_bounds__(SUM_WG) void k_rank_fill(int S, int which, double p, const double* __restrict__ y, const double* __restrict__ sorted,
                                                      const int* __restrict__ flag, double* __restrict__ w) {
    const int s = blockIdx.y * SUM_WG + threadIdx.x;
    if (s >= S) return;
    const size_t at = (size_t)blockIdx.x * S + s;
    if (flag[blockIdx.x]) { w[at] = __builtin_nan(""); return; }
    const double* v = sorted + (size_t)blockIdx.x * S;
    const double hq = (double)(S - 1) * p;
    int lo = (int)floor(hq);
    lo = lo < 0 ? 0 : lo > S - 1 ? S - 1 : lo;
    if (which == 0) {
        w[at] = y[at] <= v[lo] ? 1.0 : 0.0;
        return;
    }
    const double g = hq - (double)lo;
    const int hi = lo + 1 < S ? lo + 1 : S - 1;
    const double vlo = v[lo], vhi = v[hi];
    const double med = g == 0.0 ? vlo : vlo + g * (vhi - vlo);          // (k_sum_order's expression)
    w[at] = fabs(y[at] - med);
}

// chunk-local legs (rhat / ess of the series z, folded z, lower and upper indicator) -> the three diagnostics of columns [k0, k0 + nc).
// A series without a split R-hat has no ESS either: k_sum_ess flags the constant series itself, and this covers the series whose split
// chains are all one constant while the dropped middle draw of an odd R differs (W = var+ = 0: its tau would be the floor).
__global__ __launch_bounds__(SUM_WG) void k_rank_combine(int nc, long long k0, int mode, int N, int D, const double* __restrict__ rhat_z,
                                                         const double* __restrict__ rhat_f, const double* __restrict__ rhat_lo,
                                                         const double* __restrict__ rhat_hi, const double* __restrict__ ess_z,
                                                         const double* __restrict__ ess_lo, const double* __restrict__ ess_hi,
                                                         double* __restrict__ rhat_rank, double* __restrict__ ess_bulk, double* __restrict__ ess_tail) {
    const int c = blockIdx.x * SUM_WG + threadIdx.x;
    if (c >= nc) return;
    const long long o = out_index(mode, k0 + c, N, D);
    const double nan = __builtin_nan("");
    const double a = rhat_z[c], b = rhat_f[c];
    const double lo = isnan(rhat_lo[c]) ? nan : ess_lo[c], hi = isnan(rhat_hi[c]) ? nan : ess_hi[c];
    rhat_rank[o] = (isnan(a) || isnan(b)) ? nan : (a > b ? a : b);       // (a NaN leg gives NaN: explicitly, not fmax)
    ess_bulk[o] = isnan(a) ? nan : ess_z[c];
    ess_tail[o] = (isnan(lo) || isnan(hi)) ? nan : (lo < hi ? lo : hi);
}

struct RankOut { double *rhat, *bulk, *tail, *rank, *z, *zf; };

// one block of K columns of C x R draws, from the device (dsrc: column j of row r at dsrc[r ld + j]) or from the host (hsrc [C R][K]).
// Scratch: the chunk, the sorted columns, the derived series, the staging of the host route (its strided upload, then the transposed
// series on their way down), the chunk-local statistics of the four series and the three result arrays.
int rank_block(magi_handle* h, const char* who, const double* dsrc, const double* hsrc, long long ld, int C, int R, long long K, int mode, int N, int D,
               const SumLB& lb, const double2* tsup, const double4* prior, int max_lag, double tail_prob, const RankOut& o, int* nonfinite) {
    const size_t S = (size_t)C * R;
    const size_t cc = chunk_cols(h, S, (size_t)K);
    MagiScratch s(h, who);
    MagiColStats st[4];                                        // z, folded z, lower and upper indicator
    double *chunk, *sorted, *work, *stage, *d_rhat, *d_bulk, *d_tail;
    int *flag, *count;
    s.take(chunk, cc * S);
    s.take(sorted, cc * S);
    s.take(work, cc * S);
    s.take(stage, hsrc ? cc * S : 0);
    const SumProbs no_probs{};
    for (int j = 0; j < 4; ++j) magi_colstats_take(s, st[j], C, R, (long long)cc, (int)cc, 0, no_probs, max_lag, j != 1, false);
    s.take(d_rhat, (size_t)K); s.take(d_bulk, (size_t)K); s.take(d_tail, (size_t)K);
    s.take(flag, cc);
    s.take(count, 1, true);
    if (int rc = s.alloc()) return rc;
    const dim3 wg(SUM_WG);
    const unsigned sblocks = (unsigned)((S + SUM_WG - 1) / SUM_WG);
    for (size_t c0 = 0; c0 < (size_t)K && s.ok(); c0 += cc) {
        const int nc = (int)std::min(cc, (size_t)K - c0);
        const dim3 cells((unsigned)nc, sblocks);
        if (hsrc)
            s.note(hipMemcpy2DAsync(stage, (size_t)nc * sizeof(double), hsrc + c0, (size_t)K * sizeof(double), (size_t)nc * sizeof(double), S,
                                    hipMemcpyHostToDevice, h->stream));
        auto run = [&](int rc) { if (s.ok()) s.note(rc); };
        // the series in `work`, as the caller's [C R][K]
        auto series_down = [&](double* dst) {
            if (!dst || !s.ok()) return;
            s.note(magi_transpose(h, nc, (int)S, work, S, stage, (size_t)nc));
            if (s.ok())
                s.note(hipMemcpy2DAsync(dst + c0, (size_t)K * sizeof(double), stage, (size_t)nc * sizeof(double), (size_t)nc * sizeof(double), S,
                                        hipMemcpyDeviceToHost, h->stream));
        };
        auto rank_z = [&](const double* y, bool first, double* rank_out, double* z_out) {
            if (s.ok()) run(magi_launch(h, "k_rank_sort: ", k_rank_sort, dim3((unsigned)nc), wg, h->stream, (int)S, y, sorted, flag, first ? 1 : 0, count));
            if (s.ok()) run(magi_launch(h, "k_rank_rank: ", k_rank_rank, cells, wg, h->stream, (int)S, y, (const double*)sorted, (const int*)flag, work));
            series_down(rank_out);
            if (s.ok()) run(magi_launch(h, "k_rank_z: ", k_rank_z, cells, wg, h->stream, (int)S, (const int*)flag, work));
            series_down(z_out);
        };
        auto fill = [&](int which, double p) {
            if (s.ok()) run(magi_launch(h, "k_rank_fill: ", k_rank_fill, cells, wg, h->stream, (int)S, which, p, (const double*)chunk, (const double*)sorted,
                                        (const int*)flag, work));
        };
        auto stats = [&](int j) { if (s.ok()) run(magi_colstats_chunk(h, who, st[j], work, nc, 0, MODE_PLAIN, 1, 1)); };
        if (s.ok()) run(magi_sum_gather(h, (int)S, nc, dsrc ? dsrc + c0 : stage, dsrc ? ld : (long long)nc, mode, (int)c0, lb, tsup, prior, chunk));
        rank_z(chunk, true, o.rank, o.z);
        stats(0);
        fill(0, tail_prob);
        stats(2);
        fill(0, 1.0 - tail_prob);
        stats(3);
        fill(1, 0.5);                                          // (reads the median before the sorted column is overwritten below)
        rank_z(work, false, nullptr, o.zf);
        stats(1);
        if (s.ok())
            run(magi_launch(h, "k_rank_combine: ", k_rank_combine, dim3((unsigned)((nc + SUM_WG - 1) / SUM_WG)), wg, h->stream, nc, (long long)c0, mode, N, D,
                            (const double*)st[0].rhat, (const double*)st[1].rhat, (const double*)st[2].rhat, (const double*)st[3].rhat,
                            (const double*)st[0].ess, (const double*)st[2].ess, (const double*)st[3].ess, d_rhat, d_bulk, d_tail));
    }
    const size_t kb = (size_t)K * sizeof(double);
    s.down_opt(o.rhat, d_rhat, kb);
    s.down_opt(o.bulk, d_bulk, kb);
    s.down_opt(o.tail, d_tail, kb);
    int n_bad = 0;
    s.down(&n_bad, count, sizeof(int));
    if (int rc = s.finish()) return rc;
    if (nonfinite) *nonfinite += n_bad;
    return MAGI_OK;
}

int check_tail_prob(magi_handle* h, const char* who, double tail_prob) {
    if (!std::isfinite(tail_prob) || !(tail_prob > 0.0) || tail_prob > 0.5)
        return magi_fail(h, MAGI_E_BADARG, std::string(who) + ": tail_prob is not a finite number in (0, 0.5]");
    return MAGI_OK;
}

}  // namespace

int magi_rank_diagnostics(magi_handle* h, int C, int R, int K, const double* draws, int max_lag, double tail_prob, double* rhat_rank, double* ess_bulk,
                          double* ess_tail, double* rank, double* z, double* z_folded, int* n_nonfinite) {
    if (!h) return MAGI_E_BADARG;
    static const char* who = "magi_rank_diagnostics";
    if (!draws) return magi_fail(h, MAGI_E_BADARG, "magi_rank_diagnostics: draws is NULL");
    int rc = check_draws(h, who, C, R);
    if (rc) return rc;
    if (K < 1 || K > (1 << 24)) return magi_fail(h, MAGI_E_BADARG, "magi_rank_diagnostics: 1 <= K <= 2^24 columns");
    if ((rc = check_tail_prob(h, who, tail_prob))) return rc;
    (void)hipSetDevice(h->device);
    SumLB lb{};
    int count = 0;
    rc = rank_block(h, who, nullptr, draws, K, C, R, K, MODE_PLAIN, 1, 1, lb, nullptr, nullptr, max_lag, tail_prob,
                    RankOut{rhat_rank, ess_bulk, ess_tail, rank, z, z_folded}, &count);
    if (rc == MAGI_OK && n_nonfinite) *n_nonfinite = count;
    return rc;
}

int magi_sampler_rank_diagnostics(magi_handle* h, int chain0, int n_sel, int max_lag, double tail_prob,
                                  double* X_rhat_rank, double* X_ess_bulk, double* X_ess_tail,
                                  double* sig_rhat_rank, double* sig_ess_bulk, double* sig_ess_tail,
                                  double* th_rhat_rank, double* th_ess_bulk, double* th_ess_tail, int* n_nonfinite) {
    if (!h) return MAGI_E_BADARG;
    static const char* who = "magi_sampler_rank_diagnostics";
    MagiChainRange cr;
    int rc = magi_finished_chains(h, who, chain0, n_sel, &cr);
    if (rc) return rc;
    if ((rc = check_tail_prob(h, who, tail_prob))) return rc;
    const DevProblem& pb = h->pb;                              // the shapes; the bounds, supports and priors are cr.pb's: the member's own on a group
    const int R = cr.R;
    SumLB lb{};
    for (int d = 0; d < pb.D; ++d) lb.v[d] = cr.pb.LB[d];
    const double* base = cr.base;
    int count = 0;
    if (X_rhat_rank || X_ess_bulk || X_ess_tail || n_nonfinite)
        rc = rank_block(h, who, base, nullptr, pb.dimp, n_sel, R, pb.ND, MODE_X, pb.N, pb.D, lb, nullptr, nullptr, max_lag, tail_prob,
                        RankOut{X_rhat_rank, X_ess_bulk, X_ess_tail, nullptr, nullptr, nullptr}, &count);
    if (rc == MAGI_OK && (sig_rhat_rank || sig_ess_bulk || sig_ess_tail || n_nonfinite))
        rc = rank_block(h, who, base + pb.ND, nullptr, pb.dimp, n_sel, R, pb.D, MODE_SIGMA, pb.N, pb.D, lb, nullptr, cr.pb.prior, max_lag, tail_prob,
                        RankOut{sig_rhat_rank, sig_ess_bulk, sig_ess_tail, nullptr, nullptr, nullptr}, &count);
    if (rc == MAGI_OK && (th_rhat_rank || th_ess_bulk || th_ess_tail || n_nonfinite))
        rc = rank_block(h, who, base + pb.ND + pb.D, nullptr, pb.dimp, n_sel, R, pb.P, MODE_THETA, pb.N, pb.D, lb, cr.pb.tsup, nullptr, max_lag, tail_prob,
                        RankOut{th_rhat_rank, th_ess_bulk, th_ess_tail, nullptr, nullptr, nullptr}, &count);
    if (rc == MAGI_OK && n_nonfinite) *n_nonfinite = count;
    return rc;
}
