// Posterior predictive checks (magi_ppc, magi_sampler_ppc): replicated observations y_rep, their per-column mean, sd and quantiles, the
// PIT of every observation with the observation noise integrated analytically, and the posterior predictive p-values of four realised
// discrepancies of the standardised residuals -- definitions in include/magi_hip.h and DESIGN.md 4.8.  The scheme of elpd.hip (colstat.h):
//   k_ppc_gather  tiled gather + transpose through an LDS tile, as k_ll_gather: rows (draws) x columns of the source; sigma^2 of the tile's
//                 rows in LDS (softplus_ref(sig_pre) + LB or the MAGI_PRIOR_FIXED constant as k_sum_gather MODE_SIGMA forms it; the host
//                 route: the given array).  The arithmetic runs in the WRITE phase, where a wave holds one column and 64 draws: the
//                 column's link, weight, datum and extra variance are wave-uniform, one LDS tile serves three outputs, and the three
//                 chunks y_rep, u_obs, z0 [column][C R] are written coalesced.  One Philox block, one log / sqrt / sin / cos per (s, k).
//   k_ppc_pit     one workgroup per column: 1/S sum_s Phi(u_obs), in wg_sum's fixed order.
//   k_ppc_disc    one lane per draw: walks the chunk's columns ascending and carries sum u^2, sum u, max |u|, sum u_j u_(j+1) and the
//                 previous u of every (component, draw), for u_obs and for z0, in device memory across the chunks; the last chunk forms T.
//   k_ppc_pval    one workgroup per (component, statistic): integer counts only.
// Every floating-point sum runs in one fixed order and the only atomics are integer ones: results are bit-identical from run to run and
// do not depend on the chunking.  Does not depend on the drift (jit._DRIFT_FREE).
#include "colstat.h"

#include <cmath>
#include <vector>

namespace {

using namespace colstat;

struct PpcCount { int n[MAGI_MAX_D]; };        // columns with a datum per component
constexpr int ACC_FIELDS = 5;                  // sum u^2, sum u, max |u|, sum u_j u_(j+1), the previous u

// the columns' descriptors (gy, wt, ev, comp, oidx) point at the chunk's first column; k0 is that column's index in the call
__global__ __launch_bounds__(G_TILE * 4) void k_ppc_gather(int S, int R, int nc, long long k0, const double* __restrict__ src /* rows ld apart */, long long ld,
                                                           const int* __restrict__ oidx /* the entries e of the columns in a sample row; null: src holds the columns themselves */,
                                                           const double* __restrict__ sig /* [S][D] sigma^2; null: softplus_ref(src[row][off_sig + d]) + lb */,
                                                           int off_sig, int D, int links, SumLB lb, const double4* __restrict__ prior,
                                                           const double* __restrict__ gy /* g(y), NaN: none */, const double* __restrict__ wt,
                                                           const double* __restrict__ ev /* extra variance, or null */, const int* __restrict__ comp,
                                                           const unsigned* __restrict__ cid /* [C] Philox id of every chain */, unsigned long long seed,
                                                           double* __restrict__ yrep, double* __restrict__ uobs, double* __restrict__ z0c /* each [nc][S] */,
                                                           double* __restrict__ s2_out /* [S][D] the sigma^2 as formed here, or null */) {
    __shared__ double tile[G_TILE][G_TILE + 1];               // (+1: the column reads below fall on 32 different bank pairs)
    __shared__ double s2[G_TILE][MAGI_MAX_D];                 // sigma^2_d of the tile's rows
    const int r0 = blockIdx.x * G_TILE, c0 = blockIdx.y * G_TILE, tx = threadIdx.x, ty = threadIdx.y;
    for (int q = ty * G_TILE + tx; q < G_TILE * D; q += G_TILE * 4) {
        const int r = q / D, d = q - r * D;
        if (r0 + r < S) {
            double v;
            if (sig) {
                v = sig[(size_t)(r0 + r) * D + d];
            } else {
                v = softplus_ref(src[(size_t)(r0 + r) * (size_t)ld + off_sig + d]) + lb.v[d];
                if (prior) { const double4 pe = prior[d]; if (Prior::fixed(pe)) v = pe.y; }
            }
            s2[r][d] = v;
            if (s2_out && blockIdx.y == 0) s2_out[(size_t)(r0 + r) * D + d] = v;
        }
    }
    const bool col = c0 + tx < nc;
    int e = c0 + tx;
    if (oidx && col) e = oidx[c0 + tx];
    for (int r = ty; r < G_TILE; r += 4)
        if (r0 + r < S && col) tile[r][tx] = src[(size_t)(r0 + r) * (size_t)ld + e];
    __syncthreads();
    const int s = r0 + tx;
    if (s >= S) return;                                        // (no barrier below)
    const int ch = s / R, rr = s - ch * R;
    const unsigned chain = cid[ch];
    for (int c = ty; c < G_TILE; c += 4) {
        const int kk = c0 + c;                                 // (wave-uniform: a wave is one ty)
        if (kk >= nc) break;
        const int d = comp[kk], link = (links >> (2 * d)) & 3;
        const double w = wt[kk], g = gy[kk];
        const Philox4 p = philox4x32_10((unsigned)(k0 + kk), (unsigned)rr, chain, STREAM_PPC, seed);
        const double u1 = u01_53(p.x, p.y), u2 = u01_53(p.z, p.w);
        const double rad = sqrt(-2.0 * m_log(u1));
        const double ang = 2.0 * 3.141592653589793 * u2;
        const double z0 = rad * cos(ang), z1 = rad * sin(ang);
        double xl = tile[tx][c];
        if (ev) xl = xl + sqrt(ev[kk]) * z1;
        double gx = xl;
        if (link == ObsModel::LOG) gx = m_log(xl);
        else if (link == ObsModel::SQRT) gx = sqrt(xl);
        const double sg = s2[tx][d];
        const double gr = gx + sqrt(sg / w) * z0;
        double yr = gr;
        if (link == ObsModel::LOG) yr = m_exp(gr);
        else if (link == ObsModel::SQRT) { const double t = fmax(gr, 0.0); yr = t * t; }
        if (!isfinite(gx)) yr = __builtin_nan("");
        const size_t o = (size_t)kk * S + s;
        yrep[o] = yr;
        uobs[o] = (g - gx) * sqrt(w / sg);
        z0c[o] = z0;
    }
}

__global__ __launch_bounds__(SUM_WG) void k_ppc_pit(int S, const double* __restrict__ uobs, const double* __restrict__ gy, long long k0,
                                                    double* __restrict__ pit) {
    __shared__ double red[SUM_WG / 64];
    const int tid = threadIdx.x;
    const double* row = uobs + (size_t)blockIdx.x * S;
    const long long o = k0 + blockIdx.x;
    double a = 0.0;
    int bad = isnan(gy[blockIdx.x]);
    for (int e = tid; e < S; e += SUM_WG) {
        const double v = row[e];
        bad |= !isfinite(v);
        a += 0.5 * erfc(-v * 0.7071067811865476);
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0) pit[o] = __builtin_nan("");
        return;
    }
    a = wg_sum(a, red);
    if (tid == 0) pit[o] = a / (double)S;
}

// acc [2 sides][ACC_FIELDS][D][S], zero before the first chunk; T [2 sides][S][D][4], written by the last chunk (total: the columns with a datum)
__global__ __launch_bounds__(SUM_WG) void k_ppc_disc(int S, int nc, int D, const int* __restrict__ comp, const double* __restrict__ gy,
                                                     const double* __restrict__ uobs, const double* __restrict__ z0c, double* __restrict__ acc,
                                                     PpcCount before, PpcCount total, int last, double* __restrict__ T) {
    const int s = blockIdx.x * SUM_WG + threadIdx.x;
    if (s >= S) return;
    const size_t fs = (size_t)D * S;                           // one field of one side
    const double nan = __builtin_nan("");
#pragma unroll
    for (int d = 0; d < MAGI_MAX_D; ++d) {
        if (d >= D) break;
        for (int side = 0; side < 2; ++side) {
            const double* u = side ? z0c : uobs;
            double* a = acc + (size_t)side * ACC_FIELDS * fs + (size_t)d * S + s;
            double ss = a[0], su = a[fs], mx = a[2 * fs], cr = a[3 * fs], pv = a[4 * fs];
            int n = before.n[d];
            for (int c = 0; c < nc; ++c) {
                if (comp[c] != d || isnan(gy[c])) continue;    // (uniform over the workgroup)
                const double v = u[(size_t)c * S + s];
                ss += v * v;
                su += v;
                mx = fmax(mx, fabs(v));
                if (n > 0) cr += pv * v;
                pv = v;
                ++n;
            }
            a[0] = ss; a[fs] = su; a[2 * fs] = mx; a[3 * fs] = cr; a[4 * fs] = pv;
            if (last) {
                double* t = T + ((size_t)side * S * D + (size_t)s * D + d) * 4;
                const int nt = total.n[d];
                t[0] = nt > 0 ? ss : nan;
                t[1] = nt > 0 ? su / (double)nt : nan;
                t[2] = nt > 0 ? (isnan(ss) ? nan : mx) : nan;   // (fmax drops a NaN that the sums keep)
                t[3] = nt > 1 ? cr / ss : nan;
            }
        }
    }
}

__global__ __launch_bounds__(SUM_WG) void k_ppc_pval(int S, int D, const double* __restrict__ T, PpcCount total, double* __restrict__ pval /* [D][4] */,
                                                     int* __restrict__ n_excluded /* [D] */) {
    __shared__ int cnt[3];
    const int d = blockIdx.x >> 2, t = blockIdx.x & 3, tid = threadIdx.x;
    const double* To = T;
    const double* Tr = T + (size_t)S * D * 4;
    int nt = 0;
#pragma unroll
    for (int k = 0; k < MAGI_MAX_D; ++k) nt = k == d ? total.n[k] : nt;
    const int defined = nt > 1 ? 4 : nt > 0 ? 3 : 0;           // the statistics that exist for this component
    if (tid < 3) cnt[tid] = 0;
    __syncthreads();
    int ge = 0, fin = 0, exc = 0;
    for (int s = tid; s < S; s += SUM_WG) {
        const size_t o = ((size_t)s * D + d) * 4;
        const double a = To[o + t], b = Tr[o + t];
        if (isfinite(a) && isfinite(b)) { ++fin; ge += b >= a; }
        if (t == 0) {
            bool bad = false;
            for (int k = 0; k < defined; ++k) bad |= !isfinite(To[o + k]) || !isfinite(Tr[o + k]);
            exc += bad;
        }
    }
    atomicAdd(&cnt[0], ge);
    atomicAdd(&cnt[1], fin);
    atomicAdd(&cnt[2], exc);
    __syncthreads();
    if (tid == 0) {
        pval[blockIdx.x] = cnt[1] > 0 ? (double)cnt[0] / (double)cnt[1] : __builtin_nan("");
        if (t == 0) n_excluded[d] = cnt[2];
    }
}

struct PpcOut { double *y_rep, *mean, *sd, *quant, *pit, *T_obs, *T_rep, *pval; int *n_excl, *nonfinite; double* s2_out; };

// what both routes hand over: K columns of C x R draws, read from the device samples dsrc (rows ld apart, column k at entry oidx[k], sig_pre
// at off_sig under pb's bounds and fixed variances) or from the host array hsrc [C R][K] with sigma^2 hsig [C R][D]
struct PpcIn {
    const double *dsrc, *hsrc, *hsig;
    long long ld;
    int off_sig, D, links;
    SumLB lb;
    const double4* prior;
    std::vector<int> oidx, comp;
    std::vector<double> gy, w;
    const double* ev;
    std::vector<unsigned> cid;
    unsigned long long seed;
};

int ppc_block(magi_handle* h, const char* who, int C, int R, long long K, const PpcIn& in, int n_q, const SumProbs& probs, const PpcOut& o) {
    const size_t S = (size_t)C * R, k = (size_t)K, D = (size_t)in.D;
    const size_t cc = chunk_cols(h, 3 * S, k);                 // the three chunks together within CHUNK_DOUBLES (what elpd_block gives its one), unless a single column exceeds it: 3 C R doubles then
    const bool want_T = o.T_obs || o.T_rep || o.pval || o.n_excl;
    const bool only_s2 = o.s2_out && !(o.y_rep || o.mean || o.sd || o.quant || o.pit || want_T || o.nonfinite);      // sigma^2 alone: one column's gather forms it
    MagiScratch sc(h, who);
    MagiColStats st;
    double *yrep, *uobs, *z0c, *stage, *dsig, *dgy, *dw, *dev, *dpit, *acc, *dT, *dpval, *ds2;
    int *dcomp, *didx, *dexc;
    unsigned* dcid;
    sc.take(yrep, cc * S); sc.take(uobs, cc * S); sc.take(z0c, cc * S);
    sc.take(stage, in.hsrc ? cc * S : 0);
    sc.take(dsig, in.hsig ? S * D : 0);
    sc.take(dgy, k); sc.take(dw, k); sc.take(dev, in.ev ? k : 0); sc.take(dpit, k);
    sc.take(acc, want_T ? 2 * ACC_FIELDS * D * S : 0, true);
    sc.take(dT, want_T ? 2 * S * D * 4 : 0);
    sc.take(dpval, D * 4);
    sc.take(ds2, o.s2_out ? S * D : 0);
    sc.take(dcomp, k); sc.take(didx, in.oidx.size()); sc.take(dexc, D); sc.take(dcid, (size_t)C);
    const bool want_stats = o.mean || o.sd || o.quant || o.nonfinite;
    magi_colstats_take(sc, st, C, R, K, (int)cc, n_q, probs, 0, false, o.quant != nullptr);
    if (int rc = sc.alloc()) return rc;
    sc.up(dgy, in.gy.data(), k * sizeof(double));
    sc.up(dw, in.w.data(), k * sizeof(double));
    sc.up(dcomp, in.comp.data(), k * sizeof(int));
    sc.up(dcid, in.cid.data(), (size_t)C * sizeof(unsigned));
    if (in.ev) sc.up(dev, in.ev, k * sizeof(double));
    if (in.hsig) sc.up(dsig, in.hsig, S * D * sizeof(double));
    if (!in.oidx.empty()) sc.up(didx, in.oidx.data(), in.oidx.size() * sizeof(int));
    PpcCount total{}, before{};
    for (size_t c = 0; c < k; ++c)
        if (!std::isnan(in.gy[c])) ++total.n[in.comp[c]];
    std::vector<double> back(o.y_rep ? cc * S : 0);
    for (size_t c0 = 0; c0 < k && sc.ok(); c0 += cc) {
        const int nc = only_s2 ? 1 : (int)std::min(cc, k - c0);
        const bool last = c0 + cc >= k;
        if (in.hsrc)
            sc.note(hipMemcpy2DAsync(stage, (size_t)nc * sizeof(double), in.hsrc + c0, k * sizeof(double), (size_t)nc * sizeof(double), S,
                                     hipMemcpyHostToDevice, h->stream));
        if (sc.ok())
            sc.note(magi_launch(h, "k_ppc_gather: ", k_ppc_gather, dim3((unsigned)((S + G_TILE - 1) / G_TILE), (unsigned)((nc + G_TILE - 1) / G_TILE)),
                                dim3(G_TILE, 4), h->stream, (int)S, R, nc, (long long)c0, in.hsrc ? (const double*)stage : in.dsrc,
                                in.hsrc ? (long long)nc : in.ld, in.hsrc ? (const int*)nullptr : (const int*)(didx + c0),
                                in.hsig ? (const double*)dsig : (const double*)nullptr, in.off_sig, in.D, in.links, in.lb, in.prior,
                                (const double*)(dgy + c0), (const double*)(dw + c0), in.ev ? (const double*)(dev + c0) : (const double*)nullptr,
                                (const int*)(dcomp + c0), (const unsigned*)dcid, in.seed, yrep, uobs, z0c,
                                o.s2_out && c0 == 0 ? ds2 : (double*)nullptr));
        if (only_s2) break;
        if (sc.ok() && want_stats) sc.note(magi_colstats_chunk(h, who, st, yrep, nc, (long long)c0, MODE_PLAIN, 1, 1));
        if (sc.ok() && o.pit)
            sc.note(magi_launch(h, "k_ppc_pit: ", k_ppc_pit, dim3((unsigned)nc), dim3(SUM_WG), h->stream, (int)S, (const double*)uobs,
                                (const double*)(dgy + c0), (long long)c0, dpit));
        if (sc.ok() && want_T)
            sc.note(magi_launch(h, "k_ppc_disc: ", k_ppc_disc, dim3((unsigned)((S + SUM_WG - 1) / SUM_WG)), dim3(SUM_WG), h->stream, (int)S, nc, in.D,
                                (const int*)(dcomp + c0), (const double*)(dgy + c0), (const double*)uobs, (const double*)z0c, acc, before, total,
                                last ? 1 : 0, dT));
        for (int c = 0; c < nc; ++c)
            if (!std::isnan(in.gy[c0 + c])) ++before.n[in.comp[c0 + c]];
        if (sc.ok() && o.y_rep) {                              // chunk [nc][S] -> y_rep [S][K]
            sc.down(back.data(), yrep, (size_t)nc * S * sizeof(double));
            if (sc.ok()) sc.note(hipStreamSynchronize(h->stream));
            if (!sc.ok()) break;
            for (int c = 0; c < nc; ++c)
                for (size_t s = 0; s < S; ++s) o.y_rep[s * k + c0 + c] = back[(size_t)c * S + s];
        }
    }
    if (sc.ok() && want_T)
        sc.note(magi_launch(h, "k_ppc_pval: ", k_ppc_pval, dim3((unsigned)(D * 4)), dim3(SUM_WG), h->stream, (int)S, in.D, (const double*)dT, total, dpval, dexc));
    if (want_stats) magi_colstats_down(sc, st, o.mean, o.sd, o.quant, nullptr, nullptr, nullptr);
    sc.down_opt(o.pit, dpit, k * sizeof(double));
    if (want_T) {
        sc.down_opt(o.T_obs, dT, S * D * 4 * sizeof(double));
        sc.down_opt(o.T_rep, dT + S * D * 4, S * D * 4 * sizeof(double));
        sc.down_opt(o.pval, dpval, D * 4 * sizeof(double));
        sc.down_opt(o.n_excl, dexc, D * sizeof(int));
    }
    sc.down_opt(o.s2_out, ds2, S * D * sizeof(double));
    if (int rc = sc.finish()) return rc;
    if (o.nonfinite) *o.nonfinite = st.n_bad;
    return MAGI_OK;
}

double link_host(int link, double y) { return link == MAGI_LINK_LOG ? std::log(y) : link == MAGI_LINK_SQRT ? std::sqrt(y) : y; }

}  // namespace

int magi_ppc(magi_handle* h, int C, int R, int K, int D, const double* x, const int* comp, const double* sigma_sq, const int* link,
             const double* weight, const double* y, const double* extra_var, uint64_t seed, const int64_t* chain_ids, int n_q, const double* probs,
             double* y_rep, double* mean, double* sd, double* quant, double* pit, double* T_obs, double* T_rep, double* pval, int* n_T_excluded,
             int* n_nonfinite) {
    if (!h) return MAGI_E_BADARG;
    static const char* who = "magi_ppc";
    const std::string me = "magi_ppc: ";
    if (!x || !comp || !sigma_sq) return magi_fail(h, MAGI_E_BADARG, me + "x, comp or sigma_sq is NULL");
    int rc = check_draws(h, who, C, R);
    if (rc) return rc;
    if (K < 1 || K > (1 << 24)) return magi_fail(h, MAGI_E_BADARG, me + "1 <= K <= 2^24 columns");
    if (D < 1 || D > MAGI_MAX_D) return magi_fail(h, MAGI_E_BADARG, me + "1 <= D <= " + std::to_string(MAGI_MAX_D) + " components");
    SumProbs pr;
    if ((rc = check_probs(h, who, n_q, probs, pr))) return rc;
    PpcIn in{};
    in.hsrc = x; in.hsig = sigma_sq; in.ld = K; in.D = D; in.ev = extra_var; in.seed = seed;
    for (int d = 0; link && d < D; ++d) {
        if (link[d] < MAGI_LINK_IDENTITY || link[d] > MAGI_LINK_SQRT)
            return magi_fail(h, MAGI_E_BADARG, me + "link[" + std::to_string(d) + "] = " + std::to_string(link[d]) + " is none of MAGI_LINK_*");
        in.links |= link[d] << (2 * d);
    }
    const size_t S = (size_t)C * R;
    for (size_t i = 0; i < S * D; ++i)
        if (!std::isfinite(sigma_sq[i]) || !(sigma_sq[i] > 0.0))
            return magi_fail(h, MAGI_E_BADARG, me + "sigma_sq[" + std::to_string(i) + "] is not a finite number > 0");
    in.comp.assign(comp, comp + K);
    in.w.assign((size_t)K, 1.0);
    in.gy.assign((size_t)K, std::nan(""));
    for (int k = 0; k < K; ++k) {
        if (comp[k] < 0 || comp[k] >= D) return magi_fail(h, MAGI_E_BADARG, me + "comp[" + std::to_string(k) + "] is outside [0, D)");
        if (weight) {
            if (!std::isfinite(weight[k]) || !(weight[k] > 0.0)) return magi_fail(h, MAGI_E_BADARG, me + "weight[" + std::to_string(k) + "] is not a finite number > 0");
            in.w[k] = weight[k];
        }
        if (extra_var && (!std::isfinite(extra_var[k]) || extra_var[k] < 0.0))
            return magi_fail(h, MAGI_E_BADARG, me + "extra_var[" + std::to_string(k) + "] is not a finite number >= 0");
        if (y && !std::isnan(y[k])) {
            const int lk = (in.links >> (2 * comp[k])) & 3;
            if ((lk == MAGI_LINK_LOG && !(y[k] > 0.0)) || (lk == MAGI_LINK_SQRT && !(y[k] >= 0.0)))
                return magi_fail(h, MAGI_E_BADARG, me + "y[" + std::to_string(k) + "] is outside the domain of its link (log: y > 0, sqrt: y >= 0)");
            in.gy[k] = link_host(lk, y[k]);
        }
    }
    in.cid.resize((size_t)C);
    for (int c = 0; c < C; ++c) in.cid[c] = (unsigned)(chain_ids ? chain_ids[c] : (int64_t)c);
    (void)hipSetDevice(h->device);
    return ppc_block(h, who, C, R, K, in, n_q, pr, PpcOut{y_rep, mean, sd, quant, pit, T_obs, T_rep, pval, n_T_excluded, n_nonfinite, nullptr});
}

int magi_sampler_ppc(magi_handle* h, int chain0, int n_sel, uint64_t seed, int n_q, const double* probs, double* y_rep, double* mean, double* sd,
                     double* quant, double* pit, double* T_obs, double* T_rep, double* pval, int* n_T_excluded, int* n_nonfinite, int* obs_index,
                     int* n_obs_out, double* sigma_sq_out) {
    if (!h) return MAGI_E_BADARG;
    static const char* who = "magi_sampler_ppc";
    MagiChainRange cr;
    int rc = magi_finished_chains(h, who, chain0, n_sel, &cr);
    if (rc) return rc;
    SumProbs pr;
    if ((rc = check_probs(h, who, n_q, probs, pr))) return rc;
    const DevProblem& pb = cr.pb;
    std::vector<double> y((size_t)pb.ND), w;                  // yobs holds g_d(y) (magi_set_obs_model)
    MAGI_HIP_CHECK(h, hipMemcpy(y.data(), pb.yobs, y.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (pb.obsw) {
        w.resize((size_t)pb.ND);
        MAGI_HIP_CHECK(h, hipMemcpy(w.data(), pb.obsw, w.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    PpcIn in{};
    for (int e = 0; e < pb.ND; ++e)
        if (!std::isnan(y[e])) {
            in.oidx.push_back(e);
            in.comp.push_back(e / pb.N);
            in.gy.push_back(y[e]);
            in.w.push_back(pb.obsw ? w[e] : 1.0);
        }
    const int K = (int)in.oidx.size();
    if (n_obs_out) *n_obs_out = K;
    if (obs_index) std::copy(in.oidx.begin(), in.oidx.end(), obs_index);
    if (n_nonfinite) *n_nonfinite = 0;
    if (K == 0 || !(y_rep || mean || sd || quant || pit || T_obs || T_rep || pval || n_T_excluded || n_nonfinite || sigma_sq_out)) return MAGI_OK;
    std::vector<ChainCtl> ctl((size_t)n_sel);
    MAGI_HIP_CHECK(h, hipMemcpy(ctl.data(), h->ch.ctl + chain0, sizeof(ChainCtl) * n_sel, hipMemcpyDeviceToHost));
    in.cid.resize((size_t)n_sel);
    for (int c = 0; c < n_sel; ++c) in.cid[c] = (unsigned)ctl[c].chain_id;
    in.dsrc = cr.base; in.ld = pb.dimp; in.off_sig = pb.ND; in.D = pb.D; in.links = pb.obs_links; in.prior = pb.prior; in.seed = seed;
    for (int d = 0; d < pb.D && d < MAGI_MAX_D; ++d) in.lb.v[d] = pb.LB[d];
    return ppc_block(h, who, n_sel, cr.R, K, in, n_q, pr,
                     PpcOut{y_rep, mean, sd, quant, pit, T_obs, T_rep, pval, n_T_excluded, n_nonfinite, sigma_sq_out});
}
