// Internal declarations shared by the HIP translation units of libmagi_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/magi_hip.h"

#ifndef MAGI_MAX_D
#define MAGI_MAX_D 4        // compiled-in drifts have D <= 4, P <= 5; a library built for a traced drift with 5..8 components sets 8
#endif
#ifndef MAGI_MAX_P
#define MAGI_MAX_P 6        // a library built for a traced drift with 7 or 8 parameters sets 8
#endif
#define MAGI_MAX_DEPTH 12   // checkpoint slots for the iterative NUTS U-turn checks
#define MAGI_TAIL_THREADS 256
#define MAGI_WAVE 64

// a[d] for a runtime d without a runtime-indexed register array (which would live in scratch)
#if MAGI_MAX_D == 4
#define MAGI_SEL_D(a, d) (((d) == 0) ? (a)[0] : ((d) == 1) ? (a)[1] : ((d) == 2) ? (a)[2] : (a)[3])
#else
template <int N>
__host__ __device__ __forceinline__ double sel_n(const double (&a)[N], int d) {
    double v = a[N - 1];
#pragma unroll
    for (int k = N - 2; k >= 0; --k) v = (d == k) ? a[k] : v;
    return v;
}
#define MAGI_SEL_D(a, d) sel_n(a, d)
#endif

// ------------------------------------------------------------------------------------------
// Device-visible problem description (passed by value to kernels)
// ------------------------------------------------------------------------------------------
struct DevProblem {
    int N, D, P;
    int ld;        // row pitch (doubles) of the four matrices; even
    int band;      // -1 dense; else half-width b, rows hold columns [i-b, i+b]
    int drift;
    int ND;        // N*D
    int dim;       // N*D + D + P
    int dimp;      // dim rounded up to a multiple of 8
    double beta_inv;                       // 1.0 / beta              (magi_v2.py:348)
    double mu[MAGI_MAX_D];                 // magi_v2.py:114
    double N_ds[MAGI_MAX_D];               // magi_v2.py:53
    double LB[MAGI_MAX_D];                 // magi_v2.py:300
    const double* Csym;   // [D][N][ld]  (C^-1 + C^-T)/2
    const double* M;      // [D][N][ld]  m
    const double* Mt;     // [D][N][ld]  m^T
    const double* Ksym;   // [D][N][ld]  (K^-1 + K^-T)/2
    const double* yobs;   // [D][N], NaN = not observed        (magi_v2.py:96-100)
    // single-phase ("fused") operators of the sampler (see leap.hip / pack.hip):
    //   FH = Csym + m^T Ksym m (symmetric),  FE = Ksym m,  FK = Ksym (symmetric)
    // stored as packed TB x TB blocks, one per task: the lower block triangle of FH and FK (a block
    // serves A x and A^T x in one pass), every block of FE (serves FE xc and FE^T f) -- 2 N^2 D values
    // instead of the 4 N^2 D of four row-major stacks.
    const double* tiles;   // [n_tasks][TB][TB]
    const int* tasks;      // [n_tasks][4] = {d, kind, bi, bj}
    int n_tasks;
    const int* stasks;     // [n_stasks][8] = {d, kind, bi, bj, tile, tile1, kind1, 0}: the tasks of k_stream_sep -- the tasks above with the two
                           // diagonal blocks FH_bb, FK_bb of a component (half the work each) paired into one (tile1 >= 0), so all are equal
    int n_stasks;
    int nb;        // blocks per side, ceil(N / TB)
    int Np;        // nb * TB
    int wb;        // block half-band: blocks with |bi - bj| <= wb exist (nb when dense)
    int bandf;     // -1 dense; else half-width 3b of the fused operators (products of band-b matrices)
    const double* tgrid;   // [Np] times of the grid points (magi_set_times), padded with the last one; read by the kernels of a library whose
                           // drift uses t (DriftT<>::TDEP, point_time below) and by no other; nullptr until they are set
    const double2* tsup;   // [MAGI_MAX_P] support of every parameter (magi_set_theta_support; ThetaSup below): (sign, bound); nullptr: every
                           // parameter is positive, theta = softplus(pre) -- the kernels then run the instructions they ran without supports
    const double4* prior;  // [MAGI_MAX_D + MAGI_MAX_P] prior of every parameter entry, sigma^2_0.. then theta_0.. at MAGI_MAX_D (magi_set_prior; Prior
                           // below): (kind, a, b, 1 / b^2); nullptr: every prior is flat -- the kernels then run the instructions they ran without priors
    int fixed_mask;        // bit j: sigma^2_j is fixed (MAGI_PRIOR_FIXED) at LB[j], which then holds the constant itself; 0 without one.  A scalar of
                           // the problem and no table look-up: compute_par_entry also runs in the point kernel's boundary pass, where a load
                           // and a second mask cost the point kernel of a traced drift 48 B of scratch
    int obs_links;         // link g_d of component d's observations in bits 2d, 2d + 1 (magi_set_obs_model; ObsModel below): 0 identity, 1 log, 2 sqrt.
                           // A packed scalar for the reason fixed_mask is one: a per-lane d selects by a shift, not from a kernel-argument array
    const double* obsw;    // [D][N] known weight of every observation, laid out like yobs (1 where none was given, and at unobserved entries);
                           // nullptr: every weight is 1.  With obs_links == 0 and no weights the kernels run the instructions they ran without a model;
                           // otherwise yobs holds g_d(y)
    const float* tiles32;  // [demoted blocks][TB][TB] fp32 copies of the blocks the pack certified (pack.hip: the criterion), in the in-block order
                           // of tile32_index; a task names its copy in the upper bits of `kind` (task_slot32).  The same blocks in `tiles` hold the
                           // same rounded values as doubles.  Read by the VALU streaming kernels and their load-only twin only; nullptr: none demoted
    const int* ctasks;     // [n_carriers][3][4]: the carrier table of the VALU streaming kernels (pack.hip: carriers; option stream_carriers) -- a
                           // carrier workgroup runs the three tasks of its row side by side; a slot is a task's descriptor with ctask_word in
                           // place of d.  Read by the carrier launch and its load-only twin only
    int n_carriers;        // 0: the VALU kernels launch a 256-thread workgroup per task (as the group and matrix-core kernels always do)
};

// First word of a carrier slot: the task's index in `tasks` / `tiles` (-1: the slot is empty), whether ANY task of the carrier needs theta'
// (its workgroup then derives it and meets at the barrier behind it), and the task's component d.
__host__ __device__ inline int ctask_word(int tile, bool theta, int d) { return tile * 32 + (theta ? 16 : 0) + d; }
__host__ __device__ inline int ctask_tile(int word) { return word >> 5; }
__host__ __device__ inline bool ctask_theta(int word) { return (word & 16) != 0; }
__host__ __device__ inline int ctask_d(int word) { return word & 15; }
constexpr int MAGI_CARRIER_TASKS = 3;      // block tasks of a carrier workgroup = its units of 64 KB (an fp64 block weighs 2, a demoted one 1)

// A task's `kind` word: TileKind in the low byte; above it 1 + the block's index in tiles32 when the block is demoted, 0 = fp64 only.
constexpr int TK_SLOT_SHIFT = 8;
__host__ __device__ inline int task_kind(int word) { return word & ((1 << TK_SLOT_SHIFT) - 1); }
__host__ __device__ inline int task_slot32(int word) { return word >> TK_SLOT_SHIFT; }
// Where entry (r, c) of a demoted block sits in its fp32 copy: wave w = r / 32 of k_stream owns rows [32 w, 32 w + 32); a lane holds columns
// 2 l, 2 l + 1 of two consecutive rows in one 16-B load, and the 64 lanes of a load are contiguous (1 KB): [w][row pair][lane][row & 1][c & 1].
__host__ __device__ inline int tile32_index(int r, int c) { return ((((r >> 5) * 16 + ((r & 31) >> 1)) * 64 + (c >> 1)) << 2) + ((r & 1) << 1) + (c & 1); }
// THE threshold of the certified fp32 format (pack.hip): 2^-24 (fp32 rounding) x 2^-29 = 2^-53, the fp64 rounding of the reference sums.
constexpr double MAGI_DEMOTE_RATIO = 0x1p-29;

// Support of one parameter entry, as a table entry (x, y) = (sign, bound):
//   sign +1  theta = bound + softplus(pre)    (positive: bound 0; lower)      d theta / d pre =  sg
//   sign -1  theta = bound - softplus(pre)    (upper)                         d theta / d pre = -sg
//   sign  0  theta = pre                      (real)                          d theta / d pre =  1
// with sg = e^pre / (1 + e^pre).  The log-Jacobian term is pre - softplus(pre) for the bounded kinds and 0 for a real one, and its derivative
// is 1 - |d theta / d pre| for all of them (1 - sg, and 1 - 1 = 0): whoever holds d theta / d pre needs no second table look-up.
// `sup` is null (wave-uniform) when no support is set: the value is then formed by the expression it always was.
struct ThetaSup {
    static __device__ __forceinline__ double theta(bool has, double2 se, double pre, double sp) {
        return has ? (se.x == 0.0 ? pre : se.y + se.x * sp) : sp;
    }
    static __device__ __forceinline__ double dtheta(bool has, double2 se, double sg) { return has ? (se.x == 0.0 ? 1.0 : se.x * sg) : sg; }
    static __device__ __forceinline__ double logjac(bool has, double2 se, double pre, double sp) { return (has && se.x == 0.0) ? 0.0 : pre - sp; }
    // entry p of the table; (1, 0) without one.  p is clamped by the caller.
    static __device__ __forceinline__ double2 load(const double2* sup, int p) { return sup ? sup[p] : make_double2(1.0, 0.0); }
};

// Prior of one parameter entry on its NATURAL scale v (sigma^2 = softplus(pre) + LB; theta under its support), DESIGN 4.2d, as a table
// entry (x, y, z, w) = (kind MAGI_PRIOR_*, a, b, 1 / b^2).  Unnormalised:
//   flat       0                                        normal (m, s)     -(v - m)^2 / (2 s^2)
//   lognormal  -log v - (log v - m)^2 / (2 s^2)         gamma (k, r)      (k - 1) log v - r v
//   invgamma   -(a + 1) log v - b / v                   fixed c           sigma^2 entries only: v = c whatever pre is, see compute_par_entry
// log p joins the entry's log-Jacobian term where that term is summed into L, and its gradient (d log p / dv)(dv / dpre) is formed where the
// entry's gradient is -- both from the block's natural value and dv / dpre (leap_reduce, finalize_gradient), the gradient by `grad` below -- the ONE statement of it, so the
// theta' a stream kernel derives equals the decisions' to the bit (the products are explicit fma's or single operations: nothing left to
// contract differently from site to site).  The table pointer is null (wave-uniform) while every prior is flat.
struct Prior {
    enum { FLAT = 0, NORMAL = 1, LOGNORMAL = 2, GAMMA = 3, INVGAMMA = 4, FIXED = 5 };
    // entry j of the parameter block (j < D: sigma^2_j; else theta_{j - D}); the caller has tested the pointer
    static __device__ __forceinline__ double4 load(const double4* tab, int D, int j) { return tab[j < D ? j : min(MAGI_MAX_D + (j - D), MAGI_MAX_D + MAGI_MAX_P - 1)]; }
    static __device__ __forceinline__ bool flat(const double4& e) { return e.x == (double)FLAT; }
    static __device__ __forceinline__ bool fixed(const double4& e) { return e.x == (double)FIXED; }
    static __device__ inline double logp(const double4& e, double v);
    static __device__ inline double dlogp(const double4& e, double v);
    // g0: the entry's gradient without a prior; v, dv: its natural value and dv / dpre (PAR_SIG2, PAR_SGS / PAR_TH, PAR_SGT)
    static __device__ __forceinline__ double grad(const double4& e, double g0, double v, double dv) { return flat(e) ? g0 : fma(dlogp(e, v), dv, g0); }
    // a sigma^2 entry: under FIXED, PAR_SGS holds pre itself (d sigma^2 / d pre is 0 and needs no slot) and the gradient is that of -pre^2 / 2
    static __device__ __forceinline__ double grad_sigma(const double4& e, double g0, double s2, double sgs) { return fixed(e) ? -sgs : grad(e, g0, s2, sgs); }
};

// Member m of a problem group's device table (magi_group_create; leap.hip: k_stream_group).  The index is wave-uniform and the table
// read-only while the sampler runs: read through the constant address space, the fields are scalar loads issued where a kernel first uses
// them -- as the kernel-argument copy of a single problem is read -- and nothing is copied per lane.
__device__ __forceinline__ const DevProblem& group_member(const DevProblem* table, int m) {
    typedef const DevProblem __attribute__((address_space(4))) * const_pb_ptr;
    return *(const DevProblem*)(const_pb_ptr)(unsigned long long)(table + m);
}

// Per-chain vector slots (each dimp doubles) -------------------------------------------------
enum VecSlot {
    V_Q = 0,     // position buffer 0: X comp-major [D][N], sigma_pre[D], theta_pre[P]
    V_Q1,        // position buffer 1 (the sampler ping-pongs: plan.cur selects the one being evaluated)
    V_P,         // half-step momentum buffer 0
    V_P1,        // half-step momentum buffer 1
    V_PLEAF,     // momentum at the leaf (after the full step)
    V_G,         // UNtempered gradient of L at the evaluated position
    V_CX,        // Csym * xc           [D][N]
    V_R,         // f - m xc            [D][N]
    V_KR,        // Ksym * r            [D][N]   (fused path: Ksym * f)
    V_ETF,       // (validation kernels only)
    V_F,         // (unused)
    V_PL, V_QL, V_GL,       // left end of the trajectory
    V_PR, V_QR, V_GR,       // right end
    V_CANDQ, V_CANDG,       // trajectory-level proposal
    V_SUBQ, V_SUBG,         // subtree-level proposal
    V_RHO, V_RHOSUB,        // momentum sums (generalised U-turn)
    V_CKP0,                 // MAGI_MAX_DEPTH checkpoint momenta
    V_CKRHO0 = V_CKP0 + MAGI_MAX_DEPTH,
    V_COUNT = V_CKRHO0 + MAGI_MAX_DEPTH
};

enum ChainPhase { PH_INIT = 0, PH_LEAF = 1, PH_IDLE = 2,
                  PH_MERGED = 3,    // a subtree's end is being merged by the point phase (boundary op): the decisions of the next slot read its U-turn sums
                  PH_DRAWN = 4 };   // a transition's momentum is being drawn by the point phase: the decisions of the next slot read p.p

// Boundary work of a chain at a subtree / transition end: state-sized, element by element -- done by the POINT kernel of the slot (all its
// workgroups; leap_point.h: boundary_block) on the decisions' order (LeafPlan::vop), not by the decisions' single workgroup.
enum BoundaryOp {
    VOP_ENDS = 1,        // the finished subtree's last leaf becomes the trajectory's end `vdir`; rho += rho_sub; U-turn sums rho.p_other, rho.p_end
    VOP_CAND = 2,        // trajectory proposal <- subtree proposal (or the last leaf itself: VOP_TAKE_LEAF)
    VOP_TAKE_LEAF = 4,
    VOP_OUT = 8,         // sample row `vout` <- trajectory proposal
    VOP_DRAW = 16,       // transition `step_k` starts: momentum ~ N(0, I) at both ends, ends <- proposal, sum p.p
    VOP_DOUBLE = 32,     // a doubling starts from end `ndir`: first half / full step into buffer `cur` (+ operand mirrors, parameter block)
    VOP_ACC = 64         // a transition has ended while a metric window is open (DevChains::macc): window sums += the state the chain now holds
};

// Per-chain scalar state of the device-resident sampler ---------------------------------------
struct ChainCtl {
    int phase;
    int k;            // index of the transition in progress (0-based, burn-in included)
    int depth;        // doublings finished in this transition
    int it;           // leaf index inside the current subtree
    int nsteps;       // leaves in the current subtree (1 << depth)
    int dir;          // +1 forward / -1 backward
    int leaf_ctr;     // leaves so far in this transition (RNG counter)
    int cont;         // subtree still growing
    int nd;           // no divergence so far (subtree running value)
    int not_div;      // no divergence, committed at subtree ends
    int is_accepted;
    int lf_count;     // leapfrogs committed in this transition
    int sub_lf;
    int da_step;
    int done_epoch;   // last run epoch in which this chain reported itself idle
    int cur;          // position buffer holding the state being evaluated
    long long chain_id;
    long long total_leapfrogs;
    double eps;         // step size of this transition (> 0)
    double beta_k;      // temperature of this transition          (magi_v2.py:855)
    double beta_cache;  // temperature the cached target/grad of the proposal were computed at
    double init_energy;
    double e_sum_sub, e_sum;
    double cand_L, cand_energy, cand_weight, cand_bfac;
    double sub_L, sub_energy, sub_weight;
    double L_cur;
    double LL, LR, bfacL, bfacR;
    double bfac_cur;
    double da_step_size, da_error_sum, da_log_avg, da_log_shrink;
};

struct SamplerCfgDev {
    int total, burnin, n_adapt, max_depth, mode, hmc_L, anneal, stale;
    double step_size, target_accept, max_energy_diff, min_temp;
    unsigned long long seed;
};

struct GlobalCtl {
    int done_chains;   // chains idle in the current run epoch
    int n_chains;
    int all_done;      // every chain idle: the mat-vec kernels and the tail return immediately
    int stop_k;        // chains pause once they have finished this many transitions
    int epoch;         // incremented by the host at every magi_sampler_run
    int slots;         // leapfrog slots issued in this run before every chain was idle (counted by chain 0's decision workgroup)
    int pad[2];
};

// What the streaming kernel's epilogue must do for a chain in the next leapfrog slot; written by the
// tail (or the host for API calls), read by every workgroup of k_leap_*.
struct LeafPlan {
    int active;        // 0: leave the chain's state alone (idle chain)
    int skip;          // 1: the state in buffer `cur` was set up by the decisions while this slot's stream was already
                       //    running on something else: the point phase does nothing, the NEXT stream evaluates `cur` as is
    int leaf;          // 1: complete the leapfrog (momentum, sums, checkpoint, speculative next state)
    int cur;           // position / half-momentum buffer being evaluated (0/1)
    int even;          // write the U-turn checkpoint of this leaf
    int ck_slot;       // checkpoint slot to write (popcount of the leaf index)
    int nchk;          // U-turn checks folded into the epilogue (0..4)
    int chk_slot[4];   // their checkpoint slots
    unsigned leaf_ctr; // Philox counters of the two uniforms this leaf may need (STREAM_LEAF / STREAM_MERGE)
    unsigned depth;
    unsigned step_k;
    unsigned chain_id;
    double hs;         // 0.5 * eps * beta_k (signed)
    double eps;        // signed step
    unsigned long long seed;
    // boundary op (vop != 0: `leaf` is 0; with VOP_DOUBLE active = skip = 1 and `cur` is the buffer the NEXT stream evaluates, else active = 0)
    int vop;           // BoundaryOp bits
    int vleaf;         // position buffer of the subtree's last leaf (VOP_ENDS, VOP_TAKE_LEAF)
    int vdir;          // +1 / -1: the end the finished subtree grew (VOP_ENDS)
    int ndir;          // +1 / -1: the end the next doubling starts from (VOP_DOUBLE)
    long long vout;    // row of ch.samples (VOP_OUT)
    int sub_copy;      // leaf plans: the PREVIOUS leaf (position buffer cur ^ 1, gradient V_G as it stands) was accepted as the subtree's proposal:
                       // the point phase copies it to V_SUBQ / V_SUBG before it overwrites both (the D + P parameter entries: the decisions)
};

constexpr int MAGI_TB = 128;  // block edge of the packed single-phase operators
enum TileKind { TK_FH = 0, TK_FK = 1, TK_FE = 2 };
enum TileVec { TV_HX = 0, TV_EX = 1, TV_ETF = 2, TV_KF = 3 };

constexpr int PART_K = (1 + MAGI_MAX_D + MAGI_MAX_P + 1 + 8 + 3) / 4 * 4 < 24 ? 24 : (1 + MAGI_MAX_D + MAGI_MAX_P + 1 + 8 + 3) / 4 * 4;   // per workgroup and chain: t12, ss[D], tp[P], pp, 4 x (dA, dB)

struct DevChains {
    double* vec;          // [n_chains][V_COUNT][dimp]
    ChainCtl* ctl;        // [n_chains]
    LeafPlan* plan;       // [2][n_chains] ring by slot parity: the point phase of slot s executes plan[s & 1]
    double* part;         // [n_chains][PART_K][n_wg] partial sums of the point kernel
    int n_wg;             // workgroups along the grid axis of k_point
    double* tpart;        // [n_chains][4 (hx, ex, etf, kf)][D][nb][Np] block partials of the streaming kernel
    double* xop;          // [2 slot parities][ceil(n_chains / 16)][D][Np][16 chains]: the positions the stream of slot s evaluates, in the operand
                          // order of the matrix-core streaming kernel (a block's slice of 16 chains is contiguous), at xop[s & 1]: written by whoever
                          // sets that state up during slot s - 1 (the point phase's speculative next leaf, the decisions' new subtree start,
                          // k_prepare) -- the stream needs no plan to find it
    double* vop;          // separable drifts: operand mirror of the streaming kernel (SepLayout), written like xop; tpart then holds product slots
    double* par;          // [n_chains][PAR_COUNT] transformed parameters of the state in V_Q
    GlobalCtl* gctl;
    int n_chains;
    int mc;               // the matrix-core streaming kernel k_stream_mc serves this batch (three or more chains of a NON-separable drift): keep xop up to date
    int sep;              // the separable streaming kernel k_stream_sep serves this batch (separable drift and three or more chains, or
                          // MAGI_STREAM_FAMILY=mc): keep vop up to date, tpart holds product slots (SepLayout)
    // outputs
    double* samples;      // [n_chains][num_results][dimp]
    double* d_step_size;  // diag arrays [n_chains][total]
    double* d_lar;
    double* d_target;
    double* d_energy;
    double* d_beta;
    int* d_leapfrogs;
    int* d_depth;
    int* d_flags;         // bit0 has_divergence, bit1 reach_max_depth, bit2 is_accepted
    // diagonal metric (metric.hip, magi_sampler_set_metric).  HMC with M^-1 = diag(s^2) on q is HMC with the identity metric on z = q / s: the
    // momentum vectors hold the WHITENED momentum, and s enters only where momentum meets gradient or position,
    //     p_half = p + hs (s . g),   q' = q + eps (s . p_half);
    // the draw, p.p, rho, the checkpoints, every U-turn sum and the energies are those of the identity metric.
    const double* scale;  // [n_chains][dimp] s = sqrt(inverse mass) in state order; nullptr: identity
    double* macc;         // [n_chains][3][dimp] metric window: shift c, S1 = sum (q - c), S2 = sum (q - c)^2 over the states held after each
                          // transition that ended while the window was open (VOP_ACC); nullptr: no window
};

// s of entry e of chain cc (1 under the identity metric: a wave-uniform branch around the load, and x * 1.0 is x)
__device__ __forceinline__ double metric_scale(const DevChains& ch, size_t dimp, int cc, int e) {
    return ch.scale ? ch.scale[(size_t)cc * dimp + e] : 1.0;
}

// element (slot parity b, chain, component d, grid index i) of the operand-order mirror.  A grid point's chains are contiguous:
// 16 per point (one 128-B line), or 8 (64 B) when there are at most 8 chains -- every stream workgroup reads its operand slices of
// all chains from here, and with half-empty lines that traffic (L2 hits, in one burst at the kernel's start) is twice what it must be.
__host__ __device__ inline int xop_width(int n_chains) { return n_chains <= 8 ? 8 : 16; }
__host__ __device__ inline size_t xop_off(const DevProblem& pb, int n_chains, int b, int chain, int d, int i) {
    const size_t groups = (size_t)((n_chains + 15) >> 4);
    return ((((size_t)b * groups + (size_t)(chain >> 4)) * pb.D + d) * (size_t)pb.Np + i) * xop_width(n_chains) + (chain & 15);
}

__host__ __device__ inline size_t vec_off(const DevProblem& pb, int chain, int slot) {
    return ((size_t)chain * V_COUNT + (size_t)slot) * (size_t)pb.dimp;
}

// ------------------------------------------------------------------------------------------
// Kernel arguments are ~0.5 KB of structs passed by value; the compiler fetches their cache lines lazily, next to the
// first use, and every first touch of a line is a scalar-cache miss on the critical path of a 5 us kernel (k_point had
// four such waits in a row before its first vector load).  Touching every line up front turns them into one.
// ------------------------------------------------------------------------------------------
template <int BYTES>
__device__ __forceinline__ void kernarg_prefetch() {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const unsigned __attribute__((address_space(4))) * ka_ptr;
    ka_ptr ka = (ka_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    unsigned t = 0;
#pragma unroll
    for (int o = 0; o < BYTES; o += 64) t |= ka[o / 4];
    asm volatile("" ::"s"(t));
#endif
}

// ------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al. 2011), identical to oracle/magi_oracle.py::philox4x32
// ------------------------------------------------------------------------------------------
struct Philox4 { unsigned int x, y, z, w; };

__host__ __device__ inline Philox4 philox4x32_10(unsigned int c0, unsigned int c1, unsigned int c2,
                                                 unsigned int c3, unsigned long long key) {
    unsigned int k0 = (unsigned int)(key & 0xFFFFFFFFull), k1 = (unsigned int)(key >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        unsigned long long p0 = 0xD2511F53ull * (unsigned long long)c0;
        unsigned long long p1 = 0xCD9E8D57ull * (unsigned long long)c2;
        unsigned int hi0 = (unsigned int)(p0 >> 32), lo0 = (unsigned int)p0;
        unsigned int hi1 = (unsigned int)(p1 >> 32), lo1 = (unsigned int)p1;
        unsigned int n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox4{c0, c1, c2, c3};
}

__host__ __device__ inline double u01_53(unsigned int hi, unsigned int lo) {
    unsigned long long x = (((unsigned long long)hi << 32) | (unsigned long long)lo) >> 11;
    return ((double)x + 0.5) * 1.1102230246251565e-16;   // 2^-53
}

enum { STREAM_MOMENTUM = 0, STREAM_DIRECTION = 1, STREAM_LEAF = 2, STREAM_MERGE = 3, STREAM_HMC = 4,
       STREAM_PPC = 5 /* ppc.hip: the noise of the replicated observations, one block per (draw, column) */ };

__device__ inline double rng_uniform(unsigned int index, unsigned int step, unsigned int chain,
                                     unsigned int stream, unsigned long long key) {
    Philox4 r = philox4x32_10(index, step, chain, stream, key);
    return u01_53(r.x, r.y);
}

// ------------------------------------------------------------------------------------------
// scalar helpers.  fp64 transcendentals are ~100-300-instruction sequences; the sampler's tail is
// a run-once-per-launch kernel whose speed is set by instruction fetch, so each function exists
// ONCE per translation unit (noinline) instead of once per call site.
// ------------------------------------------------------------------------------------------
static __device__ __noinline__ double m_log(double x) { return log(x); }
static __device__ __noinline__ double m_exp(double x) { return exp(x); }
static __device__ __noinline__ double m_log1p(double x) { return log1p(x); }

__device__ inline double softplus_ref(double x) { return m_log(1.0 + m_exp(x)); }   // magi_v2.py:318

__device__ inline double Prior::logp(const double4& e, double v) {
    const int k = (int)e.x;
    if (k == NORMAL) { const double d = v - e.y; return -0.5 * (d * d) * e.w; }
    if (k == FLAT || k == FIXED) return 0.0;
    const double lv = m_log(v);
    if (k == LOGNORMAL) { const double d = lv - e.y; return -lv - 0.5 * (d * d) * e.w; }
    if (k == GAMMA) return (e.y - 1.0) * lv - e.z * v;
    return -(e.y + 1.0) * lv - e.z / v;
}
__device__ inline double Prior::dlogp(const double4& e, double v) {
    const int k = (int)e.x;
    if (k == NORMAL) return -((v - e.y) * e.w);
    if (k == LOGNORMAL) return -fma(m_log(v) - e.y, e.w, 1.0) / v;
    if (k == GAMMA) return (e.y - 1.0) / v - e.z;
    if (k == INVGAMMA) return (e.z / v - (e.y + 1.0)) / v;
    return 0.0;
}
__device__ inline double sigmoid(double x) { return 1.0 / (1.0 + m_exp(-x)); }

// Observation model: component d is observed through a link g_d -- identity, log or sqrt -- with Gaussian error of variance
// sigma^2_d on the LINK's scale, and observation k may carry a known weight w_k (a mean of n replicates counts n times):
//     t4 = sum_d (1 / sigma^2_d) sum_{k in obs_d} w_k (g_d(x_k) - g_d(y_k))^2
// The component still contributes ONE sum ss_d, so t3, t4, the sigma^2 gradient and the reduce are what they were; only the four places that
// form a point's squared residual and its x-derivative change (GridPoint::finish, point_block_sep, row_epilogue<3>, finalize_gradient), and
// they share this one statement of it.  yobs holds g_d(y) (transformed once, by magi_set_obs_model).  The link is evaluated at OBSERVED
// points only: outside its domain there (x <= 0 under log, x < 0 under sqrt) the residual is not finite, and so is the log posterior of
// that state -- the rule of a state outside a drift's domain.  `set` is wave-uniform; while it is false the callers run their old instructions.
struct ObsModel {
    enum { IDENTITY = 0, LOG = 1, SQRT = 2 };
    static __device__ __forceinline__ bool set(const DevProblem& pb) { return (pb.obs_links != 0) | (pb.obsw != nullptr); }
    // w (g(x) - gy)^2 of the observed entry e = d N + i, and `dss` = its x-derivative 2 w (g(x) - gy) g'(x); gy = g_d(y) as yobs holds it
    static __device__ __forceinline__ double resid(const DevProblem& pb, int d, size_t e, double x, double gy, double& dss) {
        const int link = (pb.obs_links >> (2 * d)) & 3;
        double gx = x, dg = 1.0;
        if (link == LOG) { gx = m_log(x); dg = 1.0 / x; }
        else if (link == SQRT) { gx = sqrt(x); dg = 0.5 / gx; }
        const double w = pb.obsw ? pb.obsw[e] : 1.0;
        const double df = gx - gy, wdf = w * df;
        dss = (2.0 * wdf) * dg;
        return wdf * df;
    }
};

__device__ inline double logaddexp(double a, double b) {
    if (a == -INFINITY && b == -INFINITY) return -INFINITY;
    double t = a - b;
    if (t > 0) return a + m_log1p(m_exp(-t));
    if (t <= 0) return b + m_log1p(m_exp(t));
    return t;   // NaN
}

__device__ inline double temperature(int step, double min_temp) {   // magi_v2.py:833-835
    return fmax(1.0 / m_log((double)step + 2.0), min_temp);
}

__device__ inline double rng_normal_elem(unsigned int e, unsigned int step, unsigned int chain,
                                         unsigned long long key) {
    Philox4 r = philox4x32_10(e >> 1, step, chain, STREAM_MOMENTUM, key);
    double u1 = u01_53(r.x, r.y), u2 = u01_53(r.z, r.w);
    double rad = sqrt(-2.0 * m_log(u1));
    double ang = 2.0 * 3.141592653589793 * u2;
    return (e & 1) ? rad * sin(ang) : rad * cos(ang);
}

// both normals of Philox pair j (elements 2 j and 2 j + 1): the same values as rng_normal_elem, with the Philox block, the
// logarithm and the square root evaluated once per pair instead of once per element
__device__ inline void rng_normal_pair(unsigned int j, unsigned int step, unsigned int chain, unsigned long long key, double& z0, double& z1) {
    Philox4 r = philox4x32_10(j, step, chain, STREAM_MOMENTUM, key);
    double u1 = u01_53(r.x, r.y), u2 = u01_53(r.z, r.w);
    double rad = sqrt(-2.0 * m_log(u1));
    double ang = 2.0 * 3.141592653589793 * u2;
    z0 = rad * cos(ang);
    z1 = rad * sin(ang);
}

// ------------------------------------------------------------------------------------------
// Transformed parameters of a state (magi_v2.py:318-323), computed ONCE per state by whoever
// writes V_Q (fp64 exp/log are ~100-instruction sequences: keeping them out of the per-row
// epilogues and out of the 1024-thread reduce is worth tens of microseconds per gradient).
// ------------------------------------------------------------------------------------------
enum ParOff { PAR_TH = 0, PAR_SGT = 8, PAR_LJT = 16, PAR_SIG2 = 24, PAR_SGS = 24 + MAGI_MAX_D, PAR_LJS = 24 + 2 * MAGI_MAX_D,
              PAR_LOG2PIS = 24 + 3 * MAGI_MAX_D,
              PAR_ULEAF = 56, PAR_UMERGE = 57 /* (unused) */,
              PAR_COUNT = 64 };

// entry j of the parameter block: j < D -> sigma_pre[j], else theta_pre[j - D]
// lb_tab: optional LDS copy of pb.LB (a per-lane select on the kernel-argument array compiles into a scratch table = a global
// round trip; the sampler's decision workgroup stages N_ds and LB in LDS once)
__device__ inline void compute_par_entry(const DevProblem& pb, int j, double pre, double* par, bool with_log2pis = true, const double* lb_tab = nullptr) {
    const double e = m_exp(pre);
    const double sp = m_log(1.0 + e);          // magi_v2.py:318-319
    const double sg = e / (1.0 + e);           // d softplus / d pre (= 1/(1+exp(-pre)) up to rounding)
    if (j < pb.D) {
        const double lb = lb_tab ? lb_tab[j] : MAGI_SEL_D(pb.LB, j);
        double s2 = sp + lb, dsg = sg, ljs = pre - sp;
        if (pb.fixed_mask) {                                       // (wave-uniform) a fixed sigma^2: the constant (held in LB), pre itself in PAR_SGS, -pre^2 / 2
            const bool fx = (pb.fixed_mask >> j) & 1;
            s2 = fx ? lb : s2;
            dsg = fx ? pre : dsg;
            ljs = fx ? -0.5 * (pre * pre) : ljs;
        }
        par[PAR_SIG2 + j] = s2;
        par[PAR_SGS + j] = dsg;
        par[PAR_LJS + j] = ljs;
        if (with_log2pis) par[PAR_LOG2PIS + j] = m_log(2.0 * 3.141592653589793 * s2);      // (leap_reduce evaluates it at the consumer)
    } else {
        // PAR_SGT holds d theta / d pre under the parameter's support (ThetaSup above; sg itself without a table)
        const int p = j - pb.D;
        const bool has = pb.tsup != nullptr;                       // (wave-uniform)
        const double2 se = ThetaSup::load(pb.tsup, min(p, MAGI_MAX_P - 1));
        const double th = ThetaSup::theta(has, se, pre, sp);
        const double ljt = ThetaSup::logjac(has, se, pre, sp);
        par[PAR_TH + p] = th;
        par[PAR_SGT + p] = ThetaSup::dtheta(has, se, sg);
        par[PAR_LJT + p] = ljt;
    }
}

// ------------------------------------------------------------------------------------------
// Drifts.  x[] = state at one grid point, th[] = the parameters on their natural scale (softplus'ed; ThetaSup under a support).
// A library built with -DMAGI_USER_DRIFT_HEADER="<file>" carries ONE drift traced from the caller's f_vec
// (magi_v2_amd/drift.py, jit.py) and instantiates the sampler's kernels for it alone.
// ------------------------------------------------------------------------------------------
template <int DRIFT> struct DriftT;
#ifdef MAGI_USER_DRIFT_HEADER
#include MAGI_USER_DRIFT_HEADER
#define MAGI_DRIFT_DISPATCH(drift, CALL) do { CALL(MAGI_DRIFT_USER); } while (0)
#else
#define MAGI_DRIFT_DISPATCH(drift, CALL)                         \
    do {                                                         \
        switch (drift) {                                         \
        case MAGI_DRIFT_SEIR3: CALL(MAGI_DRIFT_SEIR3); break;    \
        case MAGI_DRIFT_SEIR4: CALL(MAGI_DRIFT_SEIR4); break;    \
        default: CALL(MAGI_DRIFT_SIRW); break;                   \
        }                                                        \
    } while (0)
#endif
// (tm: the time of the grid point, point_time_rt below; the compiled-in drifts do not use it)
__device__ __forceinline__ double drift_f(int drift, int d, const double* x, const double* th, double tm) {
    (void)tm;
    switch (drift) {
#ifdef MAGI_USER_DRIFT_HEADER
    case MAGI_DRIFT_USER: return user_drift_f(d, x, th, tm);
#endif
    case MAGI_DRIFT_SEIR3: {   // vignette.ipynb cell 3
        double E = x[0], I = x[1], R = x[2], S = 1.0 - ((E + I) + R);
        if (d == 0) return (th[0] * S * I) - (th[2] * E);
        if (d == 1) return (th[2] * E) - (th[1] * I);
        return th[1] * I;
    }
    case MAGI_DRIFT_SEIR4: {
        double S = x[0], E = x[1], I = x[2];
        if (d == 0) return -th[0] * S * I;
        if (d == 1) return th[0] * S * I - th[2] * E;
        if (d == 2) return th[2] * E - th[1] * I;
        return th[1] * I;
    }
    default: {                 // MAGI_DRIFT_SIRW, test_magi_script.py:19-45
        double S = x[0], I = x[1], R = x[2], W = x[3];
        if (d == 0) return -th[0] * S * I + th[4] * W;
        if (d == 1) return th[0] * S * I - th[1] * I;
        if (d == 2) return th[1] * I - th[2] * R + th[3] * I * W;
        return th[2] * R - th[3] * I * W - th[4] * W;
    }
    }
}

// sum_d' g[d'] * d f_d' / d x_d   (column d of the Jacobian contracted with g)
__device__ __forceinline__ double drift_jt_g(int drift, int d, const double* x, const double* th, const double* g, double tm) {
    (void)tm;
    switch (drift) {
#ifdef MAGI_USER_DRIFT_HEADER
    case MAGI_DRIFT_USER: {
        double c[MAGI_MAX_D];
#pragma unroll
        for (int k = 0; k < MAGI_MAX_D; ++k) c[k] = 0.0;
        user_drift_jt(x, th, tm, g, c, nullptr);
        return MAGI_SEL_D(c, d);
    }
#endif
    case MAGI_DRIFT_SEIR3: {
        double E = x[0], I = x[1], R = x[2], S = 1.0 - ((E + I) + R);
        double b = th[0], gm = th[1], s = th[2];
        if (d == 0) return g[0] * (-b * I - s) + g[1] * s;
        if (d == 1) return g[0] * (b * S - b * I) - g[1] * gm + g[2] * gm;
        return -g[0] * b * I;
    }
    case MAGI_DRIFT_SEIR4: {
        double S = x[0], I = x[2];
        double b = th[0], gm = th[1], s = th[2];
        if (d == 0) return (g[1] - g[0]) * b * I;
        if (d == 1) return (g[2] - g[1]) * s;
        if (d == 2) return (g[1] - g[0]) * b * S + (g[3] - g[2]) * gm;
        return 0.0;
    }
    default: {
        double S = x[0], I = x[1], W = x[3];
        double be = th[0], ph = th[1], xi = th[2], ch = th[3], ka = th[4];
        if (d == 0) return (g[1] - g[0]) * be * I;
        if (d == 1) return -g[0] * be * S + g[1] * (be * S - ph) + g[2] * (ph + ch * W) - g[3] * ch * W;
        if (d == 2) return (g[3] - g[2]) * xi;
        return g[0] * ka + g[2] * ch * I + g[3] * (-ch * I - ka);
    }
    }
}

// out[p] += sum_d g[d] * d f_d / d theta_p
__device__ __forceinline__ void drift_tt_g_acc(int drift, const double (&x)[MAGI_MAX_D], const double (&th)[MAGI_MAX_P],
                                               const double (&g)[MAGI_MAX_D], double (&out)[MAGI_MAX_P], double tm) {
    (void)tm;
    // every case fills the same five scalars so the accumulation below keeps static indices
    double o0 = 0.0, o1 = 0.0, o2 = 0.0, o3 = 0.0, o4 = 0.0;
#ifdef MAGI_USER_DRIFT_HEADER
    if (drift == MAGI_DRIFT_USER) {
        double t[MAGI_MAX_P];
#pragma unroll
        for (int k = 0; k < MAGI_MAX_P; ++k) t[k] = 0.0;
        user_drift_jt(x, th, tm, g, nullptr, t);
#pragma unroll
        for (int k = 0; k < MAGI_MAX_P; ++k) out[k] += t[k];
        return;
    }
#endif
    switch (drift) {
    case MAGI_DRIFT_SEIR3: {
        const double E = x[0], I = x[1], R = x[2], S = 1.0 - ((E + I) + R);
        o0 = g[0] * S * I;
        o1 = (g[2] - g[1]) * I;
        o2 = (g[1] - g[0]) * E;
        break;
    }
    case MAGI_DRIFT_SEIR4: {
        const double S = x[0], E = x[1], I = x[2];
        o0 = (g[1] - g[0]) * S * I;
        o1 = (g[3] - g[2]) * I;
        o2 = (g[2] - g[1]) * E;
        break;
    }
    default: {
        const double S = x[0], I = x[1], R = x[2], W = x[3];
        o0 = (g[1] - g[0]) * S * I;
        o1 = (g[2] - g[1]) * I;
        o2 = (g[3] - g[2]) * R;
        o3 = (g[2] - g[3]) * I * W;
        o4 = (g[0] - g[3]) * W;
        break;
    }
    }
    out[0] += o0; out[1] += o1; out[2] += o2; out[3] += o3; out[4] += o4;
}

// ------------------------------------------------------------------------------------------
// Compile-time drifts for the sampler's kernels (D, P known -> no guards, no switch, small code)
// ------------------------------------------------------------------------------------------
// Separable form (SEP): f_d(x, theta) = sum_{k < nbasis(d)} coef_{d,k}(theta) phi_{d,k}(x).  The sampler's streaming kernel applies the
// operators to the theta-FREE basis vectors phi_{d,k}(x) (written by whoever sets a state up) and the point phase combines the products
// with coef(theta): the stream then needs no parameter that hangs on a global sum of the slot before (leap.hip, k_stream_sep).
// basis / coefs fill [D][NBMAX] with zeros in unused entries.
template <> struct DriftT<MAGI_DRIFT_SEIR3> {
    static constexpr int D = 3, P = 3;
    static constexpr bool TDEP = false;
    static constexpr bool SEP = true;
    static constexpr int NBMAX = 2;
    __host__ __device__ static constexpr int nbasis(int d) { return d == 2 ? 1 : 2; }
    static __device__ __forceinline__ void basis(const double (&x)[3], double (&ph)[3][2]) {
        const double E = x[0], I = x[1], R = x[2], S = 1.0 - ((E + I) + R);
        ph[0][0] = S * I; ph[0][1] = E;
        ph[1][0] = E; ph[1][1] = I;
        ph[2][0] = I; ph[2][1] = 0.0;
    }
    static __device__ __forceinline__ void coefs(const double (&th)[3], double (&c)[3][2]) {
        c[0][0] = th[0]; c[0][1] = -th[2];
        c[1][0] = th[2]; c[1][1] = -th[1];
        c[2][0] = th[1]; c[2][1] = 0.0;
    }
    static __device__ __forceinline__ void f(const double (&x)[3], const double (&th)[3], double (&o)[3]) {
        const double E = x[0], I = x[1], R = x[2], S = 1.0 - ((E + I) + R);
        o[0] = (th[0] * S * I) - (th[2] * E);
        o[1] = (th[2] * E) - (th[1] * I);
        o[2] = th[1] * I;
    }
    static __device__ __forceinline__ double f1(int d, const double (&x)[3], const double (&th)[3]) {
        const double E = x[0], I = x[1], R = x[2], S = 1.0 - ((E + I) + R);
        if (d == 0) return (th[0] * S * I) - (th[2] * E);
        if (d == 1) return (th[2] * E) - (th[1] * I);
        return th[1] * I;
    }
    // c[d] = sum_d' g[d'] df_d'/dx_d ; t[p] += sum_d g[d] df_d/dtheta_p
    static __device__ __forceinline__ void jt(const double (&x)[3], const double (&th)[3], const double (&g)[3], double (&c)[3], double (&t)[3]) {
        const double E = x[0], I = x[1], R = x[2], S = 1.0 - ((E + I) + R);
        const double b = th[0], gm = th[1], s = th[2];
        c[0] = g[0] * (-b * I - s) + g[1] * s;
        c[1] = g[0] * (b * S - b * I) - g[1] * gm + g[2] * gm;
        c[2] = -g[0] * b * I;
        t[0] += g[0] * S * I;
        t[1] += (g[2] - g[1]) * I;
        t[2] += (g[1] - g[0]) * E;
    }
};

template <> struct DriftT<MAGI_DRIFT_SEIR4> {
    static constexpr int D = 4, P = 3;
    static constexpr bool TDEP = false;
    static constexpr bool SEP = true;
    static constexpr int NBMAX = 2;
    __host__ __device__ static constexpr int nbasis(int d) { return (d == 0 || d == 3) ? 1 : 2; }
    static __device__ __forceinline__ void basis(const double (&x)[4], double (&ph)[4][2]) {
        const double S = x[0], E = x[1], I = x[2];
        ph[0][0] = S * I; ph[0][1] = 0.0;
        ph[1][0] = S * I; ph[1][1] = E;
        ph[2][0] = E; ph[2][1] = I;
        ph[3][0] = I; ph[3][1] = 0.0;
    }
    static __device__ __forceinline__ void coefs(const double (&th)[3], double (&c)[4][2]) {
        c[0][0] = -th[0]; c[0][1] = 0.0;
        c[1][0] = th[0]; c[1][1] = -th[2];
        c[2][0] = th[2]; c[2][1] = -th[1];
        c[3][0] = th[1]; c[3][1] = 0.0;
    }
    static __device__ __forceinline__ void f(const double (&x)[4], const double (&th)[3], double (&o)[4]) {
        const double S = x[0], E = x[1], I = x[2];
        o[0] = -th[0] * S * I;
        o[1] = th[0] * S * I - th[2] * E;
        o[2] = th[2] * E - th[1] * I;
        o[3] = th[1] * I;
    }
    static __device__ __forceinline__ double f1(int d, const double (&x)[4], const double (&th)[3]) {
        const double S = x[0], E = x[1], I = x[2];
        if (d == 0) return -th[0] * S * I;
        if (d == 1) return th[0] * S * I - th[2] * E;
        if (d == 2) return th[2] * E - th[1] * I;
        return th[1] * I;
    }
    static __device__ __forceinline__ void jt(const double (&x)[4], const double (&th)[3], const double (&g)[4], double (&c)[4], double (&t)[3]) {
        const double S = x[0], E = x[1], I = x[2];
        const double b = th[0], gm = th[1], s = th[2];
        c[0] = (g[1] - g[0]) * b * I;
        c[1] = (g[2] - g[1]) * s;
        c[2] = (g[1] - g[0]) * b * S + (g[3] - g[2]) * gm;
        c[3] = 0.0;
        t[0] += (g[1] - g[0]) * S * I;
        t[1] += (g[3] - g[2]) * I;
        t[2] += (g[2] - g[1]) * E;
    }
};

template <> struct DriftT<MAGI_DRIFT_SIRW> {
    static constexpr int D = 4, P = 5;
    static constexpr bool TDEP = false;
    static constexpr bool SEP = true;
    static constexpr int NBMAX = 3;
    __host__ __device__ static constexpr int nbasis(int d) { return d < 2 ? 2 : 3; }
    static __device__ __forceinline__ void basis(const double (&x)[4], double (&ph)[4][3]) {
        const double S = x[0], I = x[1], R = x[2], W = x[3];
        ph[0][0] = S * I; ph[0][1] = W; ph[0][2] = 0.0;
        ph[1][0] = S * I; ph[1][1] = I; ph[1][2] = 0.0;
        ph[2][0] = I; ph[2][1] = R; ph[2][2] = I * W;
        ph[3][0] = R; ph[3][1] = I * W; ph[3][2] = W;
    }
    static __device__ __forceinline__ void coefs(const double (&th)[5], double (&c)[4][3]) {
        c[0][0] = -th[0]; c[0][1] = th[4]; c[0][2] = 0.0;
        c[1][0] = th[0]; c[1][1] = -th[1]; c[1][2] = 0.0;
        c[2][0] = th[1]; c[2][1] = -th[2]; c[2][2] = th[3];
        c[3][0] = th[2]; c[3][1] = -th[3]; c[3][2] = -th[4];
    }
    static __device__ __forceinline__ void f(const double (&x)[4], const double (&th)[5], double (&o)[4]) {
        const double S = x[0], I = x[1], R = x[2], W = x[3];
        o[0] = -th[0] * S * I + th[4] * W;
        o[1] = th[0] * S * I - th[1] * I;
        o[2] = th[1] * I - th[2] * R + th[3] * I * W;
        o[3] = th[2] * R - th[3] * I * W - th[4] * W;
    }
    static __device__ __forceinline__ double f1(int d, const double (&x)[4], const double (&th)[5]) {
        const double S = x[0], I = x[1], R = x[2], W = x[3];
        if (d == 0) return -th[0] * S * I + th[4] * W;
        if (d == 1) return th[0] * S * I - th[1] * I;
        if (d == 2) return th[1] * I - th[2] * R + th[3] * I * W;
        return th[2] * R - th[3] * I * W - th[4] * W;
    }
    static __device__ __forceinline__ void jt(const double (&x)[4], const double (&th)[5], const double (&g)[4], double (&c)[4], double (&t)[5]) {
        const double S = x[0], I = x[1], R = x[2], W = x[3];
        const double be = th[0], ph = th[1], xi = th[2], ch = th[3], ka = th[4];
        c[0] = (g[1] - g[0]) * be * I;
        c[1] = -g[0] * be * S + g[1] * (be * S - ph) + g[2] * (ph + ch * W) - g[3] * ch * W;
        c[2] = (g[3] - g[2]) * xi;
        c[3] = g[0] * ka + g[2] * ch * I + g[3] * (-ch * I - ka);
        t[0] += (g[1] - g[0]) * S * I;
        t[1] += (g[2] - g[1]) * I;
        t[2] += (g[3] - g[2]) * R;
        t[3] += (g[2] - g[3]) * I * W;
        t[4] += (g[0] - g[3]) * W;
    }
};

// ------------------------------------------------------------------------------------------
// Time-dependent drifts (a traced f_vec that uses t: DriftT<>::TDEP).  The time of grid point i is pb.tgrid[i] (i < Np: the padding
// holds the last time, no load needs a bounds test).  Every drift evaluation of every kernel goes through the functions below; with
// TDEP false the time is the constant 0.0 that nothing reads -- no load, no instruction -- and the members are called with the
// signatures they have always had.
// ------------------------------------------------------------------------------------------
template <class DR>
__device__ __forceinline__ double point_time(const DevProblem& pb, int i) {
    if constexpr (DR::TDEP) return pb.tgrid[i];
    else return 0.0;
}
// for the kernels that take the drift id as a run-time value (logpost.hip, finalize_gradient)
__device__ __forceinline__ double point_time_rt(const DevProblem& pb, int i) {
#ifdef MAGI_USER_DRIFT_HEADER
    return point_time<DriftT<MAGI_DRIFT_USER>>(pb, i);
#else
    (void)pb; (void)i;
    return 0.0;
#endif
}
template <class DR>
__device__ __forceinline__ void drift_f_at(const double (&x)[DR::D], const double (&th)[DR::P], double tm, double (&o)[DR::D]) {
    if constexpr (DR::TDEP) DR::f(x, th, tm, o);
    else DR::f(x, th, o);
}
template <class DR>
__device__ __forceinline__ double drift_f1_at(int d, const double (&x)[DR::D], const double (&th)[DR::P], double tm) {
    if constexpr (DR::TDEP) return DR::f1(d, x, th, tm);
    else return DR::f1(d, x, th);
}
template <class DR>
__device__ __forceinline__ void drift_jt_at(const double (&x)[DR::D], const double (&th)[DR::P], double tm, const double (&g)[DR::D], double (&c)[DR::D],
                                            double (&t)[DR::P]) {
    if constexpr (DR::TDEP) DR::jt(x, th, tm, g, c, t);
    else DR::jt(x, th, g, c, t);
}
// o[d] = d f_d / d t at (x, tm): the emitted DriftT<>::ft of a time-dependent traced drift; every other drift has none and gets the
// constant 0 that the optimiser drops
template <class DR>
__device__ __forceinline__ void drift_ft_at(const double (&x)[DR::D], const double (&th)[DR::P], double tm, double (&o)[DR::D]) {
    if constexpr (DR::TDEP) DR::ft(x, th, tm, o);
    else {
#pragma unroll
        for (int d = 0; d < DR::D; ++d) o[d] = 0.0;
    }
}
template <class DR>
__device__ __forceinline__ void drift_basis_at(const double (&x)[DR::D], double tm, double (&ph)[DR::D][DR::NBMAX]) {
    if constexpr (DR::TDEP) DR::basis(x, tm, ph);
    else DR::basis(x, ph);
}

// ------------------------------------------------------------------------------------------
// Storage of the separable streaming path (k_stream_sep, leap.hip).
//   product slots of component d (tpart[chain][slot][other block][Np]; unused k stay zero):
//       d PS + 0: hx = FH xc     + 1: ex = FE xc     + 2 + k: etf_k = FE^T phi_{d,k}     + 2 + NBMAX + k: kf_k = FK phi_{d,k}
//   operand mirror vop[slot parity][chain group][d][plane][Np / 2][16][2]: plane 0 = xc_d of the group's chains (column = chain & 15),
//       plane 1 + z = basis group z: 16 matrix-core columns = (k, chain); with at most 8 chains (CW = 8) two basis functions share a
//       plane (k = 2 z + (col >> 3), chain = col & 7), else one per plane (k = z, chain = col).  Entries never written stay zero.
//       Inside a plane the grid points come in PAIRS: element (point i, column c) sits at vop_elem(i, c) = ((i >> 1) 16 + c) 2 + (i & 1), so
//       that the two points a lane of the streaming kernel needs for one matrix-core operand register pair are ONE 16-byte load (round 4:
//       the prologue of k_stream_sep is bound by the number of vector-memory instructions its CU has to issue, not by their latency).
// ------------------------------------------------------------------------------------------
template <int DRIFT> struct SepLayout {
    using DR = DriftT<DRIFT>;
    static constexpr int D = DR::D, NBMAX = DR::NBMAX;
    static constexpr int PS = 2 + 2 * NBMAX, PS_TOTAL = D * PS;
    __host__ __device__ static constexpr int slot_hx(int d) { return d * PS; }
    __host__ __device__ static constexpr int slot_ex(int d) { return d * PS + 1; }
    __host__ __device__ static constexpr int slot_etf(int d, int k) { return d * PS + 2 + k; }
    __host__ __device__ static constexpr int slot_kf(int d, int k) { return d * PS + 2 + NBMAX + k; }
    __host__ __device__ static constexpr bool slot_used(int slot) {
        const int d = slot / PS, r = slot - d * PS;
        return r < 2 || ((r - 2) % NBMAX) < DR::nbasis(d);
    }
    __host__ __device__ static constexpr int gz(int cw) { return (NBMAX * cw + 15) / 16; }          // basis planes per component
    __host__ __device__ static constexpr int planes(int cw) { return 1 + gz(cw); }
    __host__ __device__ static constexpr int plane_of(int cw, int k) { return 1 + (cw == 8 ? (k >> 1) : k); }
    __host__ __device__ static constexpr int col_of(int cw, int k, int chain_local) { return cw == 8 ? ((k & 1) * 8 + chain_local) : chain_local; }
};
// start of the (even) point i's pair inside plane `plane` (i even: block starts are multiples of 128)
__host__ __device__ inline size_t vop_off(int D, int planes, int Np, int groups, int b, int group, int d, int plane, int i) {
    return (((((size_t)b * groups + group) * D + d) * planes + plane) * (size_t)Np + i) * 16;
}
// element (point i, column c) relative to a plane's start
__host__ __device__ inline size_t vop_elem(int i, int c) { return ((size_t)(i >> 1) * 16 + (size_t)c) * 2 + (size_t)(i & 1); }

// ------------------------------------------------------------------------------------------
// reductions: 64-lane butterfly, then a fixed-order sum over the block's waves (deterministic)
// ------------------------------------------------------------------------------------------
// All cross-lane traffic stays on the VALU (DPP row operations + gfx950's v_permlane{16,32}_swap);
// the ds_bpermute path that __shfl_xor lowers to costs an LDS round trip per 32-bit half per step.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

// butterfly inside each row of 16 lanes: every lane ends with its row's sum
__device__ __forceinline__ double row16_sum(double v) {
    v += dpp_f64<0xB1>(v);    // quad_perm [1,0,3,2]
    v += dpp_f64<0x4E>(v);    // quad_perm [2,3,0,1]
    v += dpp_f64<0x141>(v);   // row_half_mirror
    v += dpp_f64<0x140>(v);   // row_mirror
    return v;
}

__device__ __forceinline__ double wave_sum(double v) {
    v = row16_sum(v);
    {   // rows 0<->1, 2<->3
        unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
        auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        v = __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
    }
    {   // lower 32 <-> upper 32
        unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
        auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        v = __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
    }
    return v;
}

// Block-wide sums of K values; every thread returns with all K totals.  sh: (K + 1) * 16 doubles.
// Stage 1: per-wave butterflies, one partial per wave.  Stage 2: wave 0 adds the <= 16 partials of
// each value with a row butterfly and publishes K totals (fixed order -> deterministic).
template <int K>
__device__ inline void block_sum(double (&v)[K], double* sh, int nw) {      // nw: the waves that call it (the others of the workgroup have ended)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave_sum(v[k]);
        if (lane == 0) sh[k * 16 + wave] = s;
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double x = (lane < nw) ? sh[k * 16 + (lane & 15)] : 0.0;
            if (lane >= 16) x = 0.0;
            x = row16_sum(x);
            if (lane == 0) sh[K * 16 + k] = x;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = sh[K * 16 + k];
    __syncthreads();
}

template <int K>
__device__ inline void block_sum(double (&v)[K], double* sh) { block_sum<K>(v, sh, (int)(blockDim.x >> 6)); }

// ------------------------------------------------------------------------------------------
// Reduce step of one gradient evaluation (all threads of the block must call it).
// Reads V_Q, V_CX, V_R, V_KR of the chain, writes the sigma_pre / theta_pre parts of V_G and
// returns the UNtempered log posterior L and t1..t4 of magi_v2.py:332-345.
// ------------------------------------------------------------------------------------------
struct FinalizeOut { double L, t1, t2, t3, t4; };

template <int NSEL>
__device__ __forceinline__ double select_lane(const double (&a)[NSEL], int base, int n, int j) {
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < NSEL; ++k)
        if (k >= base && k < base + n && j == k - base) v = a[k];
    return v;
}

// sh: [(2 + MAX_D + MAX_P) * 16] doubles, shs: [8] doubles of LDS scratch
__device__ inline FinalizeOut finalize_gradient(const DevProblem& pb, double* vb, const double* par, double* sh, double* shs) {
    const int N = pb.N, D = pb.D, P = pb.P, ND = pb.ND, dimp = pb.dimp;
    const double* q = vb + (size_t)V_Q * dimp;
    const double* Cx = vb + (size_t)V_CX * dimp;
    const double* r = vb + (size_t)V_R * dimp;
    const double* Kr = vb + (size_t)V_KR * dimp;
    double* g = vb + (size_t)V_G * dimp;

    double th[MAGI_MAX_P];
#pragma unroll
    for (int p = 0; p < MAGI_MAX_P; ++p) th[p] = (p < P) ? par[PAR_TH + p] : 0.0;

    constexpr int K = 2 + MAGI_MAX_D + MAGI_MAX_P;
    double t1s = 0.0, t2s = 0.0, ss[MAGI_MAX_D], tp[MAGI_MAX_P];
#pragma unroll
    for (int d = 0; d < MAGI_MAX_D; ++d) ss[d] = 0.0;
#pragma unroll
    for (int p = 0; p < MAGI_MAX_P; ++p) tp[p] = 0.0;

    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        double x[MAGI_MAX_D], g2[MAGI_MAX_D];
#pragma unroll
        for (int d = 0; d < MAGI_MAX_D; ++d) {
            if (d < D) {
                const int idx = d * N + i;
                const double xv = q[idx];
                x[d] = xv;
                t1s = fma(xv - pb.mu[d], Cx[idx], t1s);
                const double kr = Kr[idx];
                t2s = fma(r[idx], kr, t2s);
                g2[d] = 2.0 * kr;
                const double y = pb.yobs[idx];
                if (!isnan(y)) {
                    if (ObsModel::set(pb)) { double dss; ss[d] += ObsModel::resid(pb, d, (size_t)idx, xv, y, dss); }      // (observation model: wave-uniform)
                    else { const double df = xv - y; ss[d] = fma(df, df, ss[d]); }
                }
            } else { x[d] = 0.0; g2[d] = 0.0; }
        }
        drift_tt_g_acc(pb.drift, x, th, g2, tp, point_time_rt(pb, i));
    }
    double red[K];
    red[0] = t1s;
    red[1] = t2s;
#pragma unroll
    for (int d = 0; d < MAGI_MAX_D; ++d) red[2 + d] = ss[d];
#pragma unroll
    for (int p = 0; p < MAGI_MAX_P; ++p) red[2 + MAGI_MAX_D + p] = tp[p];
    block_sum<K>(red, sh);

    // scalar part: one wave, lane j <-> parameter j (no transcendental left: see compute_par_entry)
    if (threadIdx.x < 64) {
        const int j = threadIdx.x;
        double t3 = 0.0, t4 = 0.0, lj = 0.0;
        if (j < D) {
            const double s2 = par[PAR_SIG2 + j], sg = par[PAR_SGS + j];
            const double ssd = select_lane<K>(red, 2, MAGI_MAX_D, j);
            const double nds = MAGI_SEL_D(pb.N_ds, j);
            t3 = nds * par[PAR_LOG2PIS + j];
            t4 = ssd * (1.0 / s2);
            lj = par[PAR_LJS + j];
            const double dsig = nds / s2 - ssd / (s2 * s2);
            double gj = -0.5 * dsig * sg + (1.0 - sg);
            if (pb.prior) { const double4 pe = Prior::load(pb.prior, D, j); gj = Prior::grad_sigma(pe, gj, s2, sg); lj += Prior::logp(pe, s2); }
            g[ND + j] = gj;
        } else if (j < D + P) {
            const int p = j - D;
            const double sg = par[PAR_SGT + p];                     // d theta / d pre; the log-Jacobian's derivative is 1 - |sg| (ThetaSup)
            const double tpp = select_lane<K>(red, 2 + MAGI_MAX_D, MAGI_MAX_P, p);
            lj = par[PAR_LJT + p];
            double gj = -0.5 * pb.beta_inv * tpp * sg + (1.0 - fabs(sg));
            if (pb.prior) { const double4 pe = Prior::load(pb.prior, D, j); gj = Prior::grad(pe, gj, par[PAR_TH + p], sg); lj += Prior::logp(pe, par[PAR_TH + p]); }
            g[ND + D + p] = gj;
        }
        t3 = wave_sum(t3);
        t4 = wave_sum(t4);
        lj = wave_sum(lj);
        if (j == 0) {
            shs[0] = -0.5 * ((pb.beta_inv * (red[0] + red[1])) + (t3 + t4)) + lj;
            shs[1] = t3;
            shs[2] = t4;
        }
    }
    __syncthreads();   // V_G and shs complete for the whole block
    FinalizeOut o;
    o.t1 = red[0];
    o.t2 = red[1];
    o.L = shs[0];
    o.t3 = shs[1];
    o.t4 = shs[2];
    return o;
}

// ------------------------------------------------------------------------------------------
// Host-side handle
// ------------------------------------------------------------------------------------------
// Tuning / test switches of a handle.  The environment variables of the same names (MAGI_STREAM_FAMILY, ...) are read ONCE, when the
// handle is created; afterwards only magi_set_option changes them (no getenv on any compute path: a concurrent setenv cannot race a
// launch, and a stray variable cannot change what a running job computes between two calls).
#define MAGI_GEMM_REMAP_MIN_DEFAULT 10
struct MagiOptions {
    int stream_family = 0;              // 0 auto (leap.hip: magi_stream_kernel), 1 "mc": every batch on the matrix-core kernel, 2 "valu"
    int family_chains = 0;              // > 0: "auto" decides as if the batch had this many chains (the largest per-GPU share of a sharded job:
                                        // every rank then runs the same kernel family, whatever its own share -- shard.family_chains_for)
    int sep_pair_min = 256;             // pack.hip: pair the diagonal blocks FH_bb + FK_bb when there are more tasks than this
    int fused_parity = 0;               // magi_logpost_grad_fused evaluates as an even (0) / odd (1) leapfrog slot
    int stream_carriers = 0;            // pack.hip: launch the VALU streaming kernels in carrier workgroups, three block tasks on one CU filled by bytes: 0 never
                                        // (the default: measured slower, profiles/r22_carriers_ab.txt), -1 where that turns a launch of several rounds into
                                        // one round, 1 wherever a CU holds exactly one carrier
    int tile_demote = 1;                // pack.hip: store the operator blocks the criterion certifies as fp32 for the VALU streaming kernels (0: none)
    int gemm_remap_min = MAGI_GEMM_REMAP_MIN_DEFAULT;      // build.hip: super-block tile order from this many super-blocks per launch (24 until round 4;
                                        // while it is at its default, potrf's thin launches keep 24: GemmArgs::remap_min)
    int potrf_panels = 3;               // build.hip: 128-wide panels per block column of the Cholesky factorisation (3: best of 2..8 at N = 1024..8192, profiles/r04_potrf_lookahead_ab.txt)
    int potrf_lookahead_min = 4096;     // build.hip: grids from this size on factorise with look-ahead (0: never), see potrf
    long long slot_budget_graphs = 0;   // TEST HOOK: cap on the graph launches of one magi_sampler_run (0 = the computed bound)
    int summary_chunk_cols = 0;         // TEST HOOK: summary.hip gathers at most this many columns per chunk (0 = what the work space allows)
    int gp_chunk_rows = 0;              // TEST HOOK: gp.hip works on at most this many rows of t_new per chunk (0 = what the work space allows)
    int gp_profile = 0;                 // gp.hip: per-stage device times (HIP events, a synchronisation per stage; read by magi_gp_profile)
    int no_graph = 0;                   // launch the leapfrog slots directly (debugging, long rocprofv3 kernel traces)
    int fit_host_loop = 0;              // build.hip: the hyper-parameter fit with its scalar tail on the host (the tests' reference)
    int build_profile = 0, build_serial = 0;           // build.hip: per-class device times (serialises), one component per group
};
void magi_options_from_env(MagiOptions& o);               // capi.hip

// The streaming kernels: k_stream<1>, k_stream<2> (VALU), k_stream_mc, k_stream_sep<CW = 8 | 16> (matrix cores)
enum class StreamKernel { Valu1, Valu2, Mc, Sep8, Sep16 };

// optional per-class timing of the build (MAGI_BUILD_PROFILE=1): HIP events around every launch, so the
// build is serialised and slower -- diagnostics only
enum BuildClass { BC_MATERN = 0, BC_DIAG, BC_PANEL, BC_TRAIL, BC_TRTRI, BC_LAUUM, BC_PROD, BC_FUSED, BC_COUNT };
struct BuildProfile {
    double flops[BC_COUNT] = {}, ms[BC_COUNT] = {};
    long calls[BC_COUNT] = {};
    bool on = false;                    // armed by a dense build with opt.build_profile (and through the pack that follows), disarmed by a fit
    hipEvent_t e0 = nullptr, e1 = nullptr;      // created on the handle's device by the first profiled build
};

// The model a problem carries: supports of theta (magi_set_theta_support), priors of the D + P parameter entries (magi_set_prior), observation
// model (magi_set_obs_model) -- the host copies the getters and the checkpoint tag read, and the device tables pb.tsup / pb.prior / pb.obsw
// point at while the model is not the default.  A feature that adds model state adds it HERE: a member, its default in magi_model_default,
// its bytes in magi_model_mix; its setter ends in model_upload (capi.hip), which raises the sampler level of magi_stale.
struct MagiModel {
    int th_kind[MAGI_MAX_P] = {};
    double th_bound[MAGI_MAX_P] = {};
    int pr_kind[MAGI_MAX_D + MAGI_MAX_P] = {};
    double pr_a[MAGI_MAX_D + MAGI_MAX_P] = {}, pr_b[MAGI_MAX_D + MAGI_MAX_P] = {};
    double lb_orig[MAGI_MAX_D] = {};  // LB as magi_set_problem gave it (pb.LB holds the constant of a fixed sigma^2 instead)
    // the data as magi_set_problem gave them -- entry d N + i and UNtransformed value of observation k, so that the observation model can be
    // changed or reset without a new magi_set_problem --, the links and the weights (empty: none given)
    std::vector<int64_t> obs_e;
    std::vector<double> obs_y, obs_w;
    int ob_link[MAGI_MAX_D] = {};
    // allocated once and freed with the handle (a group's device table may hold their addresses): [MAGI_MAX_P], [MAGI_MAX_D + MAGI_MAX_P]
    double2* dTsup = nullptr;
    double4* dPrior = nullptr;
    double* dObsw = nullptr;          // [D][N] like dYobs: allocated on first use, freed with the problem (magi_model_default)
};

// THE default: every theta positive, every prior flat (LB as given), identity links, no weights -- the kernels' default paths.  The data
// (obs_e, obs_y, lb_orig) are the problem's, not the model's, and stay.  m == nullptr: the DevProblem half alone (a group's copy of a shape).
inline void magi_model_default(DevProblem& pb, MagiModel* m) {
    pb.tsup = nullptr; pb.prior = nullptr; pb.fixed_mask = 0; pb.obs_links = 0; pb.obsw = nullptr;
    if (!m) return;
    for (int p = 0; p < MAGI_MAX_P; ++p) { m->th_kind[p] = MAGI_THETA_POSITIVE; m->th_bound[p] = 0.0; }
    for (int j = 0; j < MAGI_MAX_D + MAGI_MAX_P; ++j) { m->pr_kind[j] = MAGI_PRIOR_FLAT; m->pr_a[j] = m->pr_b[j] = 0.0; }
    for (int d = 0; d < MAGI_MAX_D; ++d) { m->ob_link[d] = MAGI_LINK_IDENTITY; pb.LB[d] = m->lb_orig[d]; }
    m->obs_w.clear();
    if (m->dObsw) (void)hipFree(m->dObsw);
    m->dObsw = nullptr;
}

// What of the model a checkpoint's tag covers (capi.hip: ckpt_tag), through mix(pointer, bytes): each part only while it is set, so that a
// tag without a model is what it was before models existed.  Bytes and order are part of the checkpoint format.
template <typename Mix>
void magi_model_mix(const MagiModel& m, const DevProblem& pb, Mix&& mix) {
    if (pb.tsup) { mix(m.th_kind, sizeof(int) * pb.P); mix(m.th_bound, sizeof(double) * pb.P); }
    if (pb.prior) { const int n = pb.D + pb.P; mix(m.pr_kind, sizeof(int) * n); mix(m.pr_a, sizeof(double) * n); mix(m.pr_b, sizeof(double) * n); }
    if (pb.obs_links || pb.obsw) {
        mix(m.ob_link, sizeof(int) * pb.D);
        if (!m.obs_w.empty()) mix(m.obs_w.data(), sizeof(double) * m.obs_w.size());
    }
}

struct magi_handle {
    int device = 0;
    MagiOptions opt;
    hipStream_t stream = nullptr;
    std::string err;

    // matrices
    bool have_matrices = false;
    bool have_problem = false;
    DevProblem pb{};
    double *dCsym = nullptr, *dM = nullptr, *dMt = nullptr, *dKsym = nullptr, *dYobs = nullptr;
    double* dTimes = nullptr;        // pb.tgrid: the times of the grid points (magi_set_times), [times_cap >= pb.Np]
    int times_N = 0;                 // the N they were set for (0: not set; forgotten when the matrices change to another N)
    size_t times_cap = 0;
    MagiModel model;                 // supports, priors, observation model (above)
    size_t mat_elems = 0;
    // dense C^-1, m, K^-1 ([D][N][N], unmasked) as built or uploaded: authoritative until the caller uploads others; packed
    // (band mask, symmetrised / transposed copies, single-phase operator blocks) by magi_pack_matrices
    double* dDense[3] = {nullptr, nullptr, nullptr};
    int dense_N = 0, dense_D = 0;
    double* dTiles = nullptr;
    int* dTasks = nullptr;
    size_t tiles_cap = 0, tasks_cap = 0;
    float* dTiles32 = nullptr;       // pb.tiles32: fp32 copies of the demoted blocks (grown like dTiles, stale with it)
    size_t tiles32_cap = 0;
    // carriers of the current pack (pack.hip), decided or not: units of 64 KB per carrier; the block index of every slot (-1: empty); pb.n_carriers says
    // whether the VALU kernels launch them.  carrier_fits: a CU holds exactly one carrier workgroup (magi_carrier_one_per_cu, asked by magi_create)
    std::vector<int> carrier_units, carrier_slots, carrier_table;      // (carrier_table: the host copy of pb.ctasks, the source of its upload)
    bool carrier_fits = false;
    int n_demoted = 0;               // blocks of the current pack that have one (0 under the option tile_demote = 0, banded fused storage, N <= 256)
    // work space of the matrix build and the packing, kept between calls (grow-only): a repeated build at N = 8192 otherwise spends
    // more host time in hipMalloc / hipFree of ~35 GB than the GPU spends on the build
    enum { WS_KAP = 0, WS_P, WS_PP, WS_DINV, WS_PANEL, WS_TCS, WS_TM, WS_TKS, WS_TE, WS_APPLY, WS_TI, WS_TSUM, WS_COUNT };
    double* ws[WS_COUNT] = {};
    size_t ws_cap[WS_COUNT] = {};

    // chains
    int n_chains = 0;
    int cap_chains = 0;
    DevChains ch{};
    SamplerCfgDev cfg{};
    bool sampler_ready = false;
    StreamKernel stream_kernel = StreamKernel::Valu1;      // magi_stream_kernel(n_chains) at the last magi_ensure_chains
    int num_results = 0;
    // graph of G leapfrog slots
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    int graph_slots = 0;
    int graph_chains = 0;
    bool graph_valid = false;
    GlobalCtl* h_gctl = nullptr;     // pinned, 4 snapshots
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;
    int epoch = 0;
    long long* d_chain_ids = nullptr;
    double* d_fin = nullptr;         // [cap_chains][8] finalize outputs
    // diagonal metric (capi.hip: magi_sampler_set_metric ...; metric.hip).  ch.scale / ch.macc point at these while a metric is set / a
    // window is open and are null otherwise: kernel arguments, so a change between null and non-null drops the captured graph
    double* d_scale = nullptr;       // [cap_chains][dimp]
    double* d_macc = nullptr;        // [cap_chains][3][dimp]
    double* d_mwork = nullptr;       // [cap_chains][dimp + 4] k_metric_adapt: variances | median, min s, status
    std::vector<int> window_k0;      // transition index of every chain when the open window was opened (empty: no window)
    size_t samples_cap = 0, diag_cap = 0;
    size_t tpart_elems = 0, vop_elems = 0;      // doubles of ch.tpart / ch.vop as allocated (magi_ensure_chains: allocation and later memsets)
    // magi_sampler_profile: when set, the launchers of k_stream / k_point attach these events to the launch (hipExtLaunchKernel:
    // they take the kernel's own begin / end time stamps, what rocprofv3's kernel trace reports)
    hipEvent_t prof_e0 = nullptr, prof_e1 = nullptr;
    long long last_slots = 0, last_graphs = 0;      // of the last magi_sampler_run
    double* apply_pin = nullptr;     // pinned staging of magi_dense_apply (V | Y)
    // look-ahead of the blocked Cholesky (build.hip: potrf): a second stream whose queue may NOT use one CU of every XCD -- the
    // rank-k updates it carries leave those CUs to the diagonal-block kernel of the next block column -- and the fork / join events
    hipStream_t stream_trail = nullptr, stream_chain = nullptr;      // (the chain of a block column runs on a stream of the highest priority)
    hipEvent_t ev_la[3] = {nullptr, nullptr, nullptr};
    bool trail_unavailable = false;  // the masked stream could not be created: factorise without look-ahead
    hipEvent_t ev_pw[4] = {nullptr, nullptr, nullptr, nullptr};      // begin / end of the two factorisations of a dense build
    double potrf_wall_ms = 0.0, potrf_wall_flops = 0.0;              // of the last dense build (whole factorisations, not serialised)
    BuildProfile prof;                                               // of the last profiled dense build of THIS handle (build.hip)
    double gp_ms[5] = {};            // gp.hip: cross blocks, weights, application GEMM, its mu epilogue, statistics of the last call under the option gp_profile
    size_t apply_pin_cap = 0;
    // problem group (magi_group_create): group_n > 0 members whose chains this handle samples; it has no matrices of its own
    int group_n = 0;
    std::vector<magi_handle*> members;
    DevProblem* d_members = nullptr;     // [group_n] device table: the members' problems as of the last magi_sampler_init
    int group_per = 0;                   // chains per member (n_chains / group_n)
};

// error helpers -------------------------------------------------------------------------------
extern thread_local std::string g_magi_last_error;
int magi_fail(magi_handle* h, int code, const std::string& msg);

// What a call makes stale, in levels that each include the ones before: the captured graph; + the sampler (magi_sampler_init comes next);
// + the chain buffers, with the metric's; + the problem and its model (magi_set_problem comes next); + the packed matrices.
// capi.hip: magi_stale, under the table of who raises which -- the one place that clears these flags and destroys the graph.
enum MagiStale { STALE_GRAPH, STALE_SAMPLER, STALE_CHAINS, STALE_PROBLEM, STALE_MATRICES };
void magi_stale(magi_handle* h, MagiStale level);

// THE rule of a grow-only device buffer p with room for cap elements: enough room -> nothing happens; else the old block is freed and p,
// cap are cleared BEFORE the allocation, and cap is set only after it succeeded -- a failure leaves {nullptr, 0}, never a freed address or
// a capacity without memory.  Pointers that alias p (in a DevProblem, in DevChains) are the caller's to clear first.
template <typename T>
int magi_grow(magi_handle* h, T*& p, size_t& cap, size_t need, const char* what) {
    if (need <= cap) return MAGI_OK;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), need * sizeof(T));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        p = nullptr;
        return magi_fail(h, MAGI_E_HIP, std::string(what) + " allocation failed (" + std::to_string(need * sizeof(T) >> 20) + " MiB): " + hipGetErrorString(e));
    }
    cap = need;
    return MAGI_OK;
}

// work-space slot `k` with room for n doubles (magi_grow; freed by magi_destroy); nullptr + error on failure
double* magi_workspace(magi_handle* h, int k, size_t n);

#define MAGI_HIP_CHECK(h, expr)                                                                   \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess)                                                                     \
            return magi_fail((h), MAGI_E_HIP,                                                     \
                             std::string(#expr) + ": " + hipGetErrorString(_e) + " (" + __FILE__ + \
                                 ":" + std::to_string(__LINE__) + ")");                           \
    } while (0)

// Launches kernel k (`what` heads the error message); while magi_sampler_profile has set the handle's event pair, as an extended
// launch that records the kernel's own begin / end in them.
template <typename... P, typename... A>
int magi_launch(magi_handle* h, const char* what, void (*k)(P...), dim3 grid, dim3 block, hipStream_t s, A... args) {
    if (h->prof_e0) hipExtLaunchKernelGGL(k, grid, block, 0, s, h->prof_e0, h->prof_e1, 0, args...);
    else hipLaunchKernelGGL(k, grid, block, 0, s, args...);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return magi_fail(h, MAGI_E_HIP, std::string(what) + hipGetErrorString(e));
    return MAGI_OK;
}

// capi.hip: MAGI_OK where this library serves drift_id (a compiled-in drift, or MAGI_DRIFT_USER in a library built for a traced f_vec),
// else the error; hint: with the pointer to magi_v2_amd.jit in the message
int magi_check_drift_id(magi_handle* h, int drift_id, bool hint = true);

// summary.hip, for ode.hip and ode_adaptive.hip: both integrate into trj[T D][S_pad] with S_pad = roundup(S, MAGI_ODE_PAD) and status[S_pad];
// R = T D.  magi_ode_stats: mean, sd [R] and n_failed over the draws with status 0 (k_ode_stats); magi_ode_transpose: out[S][R].
// magi_transpose: in[rows][ld_in] -> out[cols][ld_out] (k_transpose; what magi_ode_transpose launches, and gp.hip for its draws).
constexpr int MAGI_ODE_PAD = 64;
int magi_ode_stats(magi_handle* h, int S, int S_pad, int R, const double* trj, const int* status, double* mean, double* sd, int* n_failed);
int magi_ode_transpose(magi_handle* h, int S, int S_pad, int R, const double* trj, double* out);
int magi_transpose(magi_handle* h, int rows, int cols, const double* in, size_t ld_in, double* out, size_t ld_out);

// launchers implemented in logpost.hip / sampler.hip ---------------------------------------------
int magi_launch_gradient(magi_handle* h, int n_chains, hipStream_t s);        // phases 1-3
int magi_launch_phase(magi_handle* h, int phase, int n_chains, hipStream_t s);
int magi_launch_finalize(magi_handle* h, int n_chains, double* d_out, hipStream_t s);
int magi_launch_stream(magi_handle* h, int n_chains, int parity, bool with_decisions, hipStream_t s);   // k_stream: block mat-vecs of slot `parity` (+ decisions of the previous slot)
int magi_launch_point(magi_handle* h, int n_chains, int parity, hipStream_t s);                            // k_point: leapfrog epilogue per grid point
int magi_launch_leap_finalize(magi_handle* h, int n_chains, double* d_out, hipStream_t s, int parity = 0);
int magi_leap_wgs(const DevProblem& pb);
int magi_launch_stream_group(magi_handle* h, int n_chains, int parity, bool with_decisions, hipStream_t s);   // leap_group.hip: the group twins
int magi_launch_point_group(magi_handle* h, int n_chains, int parity, hipStream_t s);                            // of the two above (magi_group_create)
StreamKernel magi_stream_kernel(const magi_handle* h, int n_chains);    // leap.hip: the streaming kernel that serves a batch of n_chains
int magi_build_profile_get(const magi_handle* h, double* flops, double* ms, long* calls);           // build.hip
int magi_fit_hparams_device(magi_handle* h, const double* I, int N, int D, const double* X, const double* mu, const double* mu_phi2,
                            const double* sd_phi2, const double* sig_loc, double nu, int iters, double lr, double jitter,
                            double* phi1, double* phi2, double* sig2, double* loss_trace);
bool magi_carrier_one_per_cu();                                                          // leap.hip: the occupancy query behind magi_handle::carrier_fits
int magi_launch_read_tiles(magi_handle* h, int rev, hipStream_t s);                     // load-only pass over the packed operator blocks
int magi_launch_plan_eval(magi_handle* h, int n_chains, hipStream_t s, int parity = 0);        // plan: evaluate buffer 0, no leapfrog                                       // workgroups along the grid axis
// build.hip: E = Ks M, H = Cs + M^T E for D dense [N][N] components (H overwrites Cs)
int magi_fused_operators(magi_handle* h, int N, int D, double* dCs_inout_H, const double* dM, const double* dKs, double* dE);
int magi_launch_prepare(magi_handle* h, int n_chains, hipStream_t s);   // fills par from V_Q
int magi_launch_mirror(magi_handle* h, int n_chains, hipStream_t s);    // leap.hip: separable drifts: operand mirror (both slot parities) from V_Q
bool magi_drift_separable(int drift);                                   // leap.hip
size_t magi_sep_tpart_elems(const DevProblem& pb, int n_chains);        // leap.hip: doubles in tpart / vop for the separable path
size_t magi_sep_vop_elems(const DevProblem& pb, int n_chains);
void magi_sep_traffic(const DevProblem& pb, int n_chains, double* stores, double* operands, double* point_reads, double* mirror_writes);   // leap.hip
int magi_launch_init_chains(magi_handle* h, const long long* d_chain_ids, hipStream_t s);
// metric.hip: the regularised diagonal metric of every chain from the window sums macc ([n][3][dimp], n_win states each) ->
// scale [n][dimp]; work [n][dimp + 4]: the variances, then {median, min s, status (0 set, 1 median 0: scale left as it was), -}
int magi_launch_metric_adapt(magi_handle* h, int n_chains, int n_win, double kappa, double rel_floor, const double* macc, double* scale,
                             double* work, hipStream_t s);
int magi_ensure_chains(magi_handle* h, int n_chains);
// build.hip: dense device matrices -> packed device storage (sym / transpose / band)
int magi_pack_matrices(magi_handle* h, int N, int D, int bandsize, const double* dC_inv, const double* dM,
                       const double* dK_inv);
int magi_build_matrices_device(magi_handle* h, const double* I, int N, int D, const double* phi1,
                               const double* phi2, double nu, int bandsize, double* C_inv, double* m,
                               double* K_inv);
// build.hip: the listed components of the resident dense stacks (allocated / zeroed when N, D change); no packing
int magi_build_dense_device(magi_handle* h, const double* I, int N, int D, int n_sel, const int* sel, const double* phi1,
                            const double* phi2, double nu);
int magi_ensure_dense(magi_handle* h, int N, int D);
// pack.hip: Y[d] = A_d V[d] or A_d^T V[d] for the resident dense stack `which` (0 C^-1, 1 m, 2 K^-1); V, Y device [D][N][nv]
int magi_dense_apply_device(magi_handle* h, int which, int trans, int nv, const double* dV, double* dY);
// thetainit.hip: Adam x iters on the theta objective of magi_v2.py:148-158 with the resident UNbanded stacks, one captured graph per step
int magi_theta_init_device(magi_handle* h, int drift, int P, const double* Xhat, const double* mu, int iters, double lr, double* theta, double* loss_trace);
// build.hip, for gp.hip: Ks, pKs (device [T][N], either may be null) = k, dk/dt* of the row times dT[T] against the grid times dI[N]
// (k_matern_cross: k_matern's arithmetic entry by entry, the coincident branch on equal times); the coincident value of Kappa_pp
int magi_matern_cross_launch(magi_handle* h, hipStream_t s, const double* dT, int T, const double* dI, int N, double phi1, double phi2, double nu,
                             double* dKs, double* dPKs);
double magi_matern_diag_pp(double phi1, double phi2, double nu);
// build.hip: the strided fp64 MFMA GEMM of the matrix build (k_gemm_f64 through launch_gemm), C(m, n) = sum_k A(m, k) B(n, k) with
// A(m, k) = A[m sAm + k sAk], B(n, k) = B[n sBn + k sBk], C(m, n) = C[m ldc + n], over inner x outer batches: batch* step the inner index,
// batch*2 the outer one.  Every output's k loop runs in the same order whatever the shape and the strides.
struct MagiGemm {
    const double* A; long sAm, sAk, batchA, batchA2;
    const double* B; long sBn, sBk, batchB, batchB2;
    double* C; long ldc, batchC, batchC2;
    int M, N, K, inner, outer;
};
int magi_gemm_strided(magi_handle* h, hipStream_t s, const MagiGemm& g);
// summary.hip: chains [chain0, chain0 + n_sel) of a sampler that has finished, for the post-processing entry points (who: the caller's
// name in the messages).  Refuses a sampler that is not initialised, a range outside its chains or across two members of a group, a
// chain with transitions left, and C = n_sel, R = num_results beyond the statistics' limits.
struct MagiChainRange {
    int member;                       // the group member that owns the chains, -1 without a group
    DevProblem pb;                    // the handle's problem, or the member's own as the sampler read it (magi_sampler_init)
    int R;                            // draws per chain
    const double* base;               // the first selected chain's rows in ch.samples (R rows of pb.dimp doubles per chain)
};
int magi_finished_chains(magi_handle* h, const char* who, int chain0, int n_sel, MagiChainRange* out);
int magi_matern_blocks_device(magi_handle* h, const double* I, int N, double phi1, double phi2, double nu,
                              double* Kappa, double* p_Kappa, double* Kappa_pp);
