/*
 * magi_hip.h -- C ABI of libmagi_hip.so, the MI355X (gfx950) engine for the MAGI hot path.
 *
 * The reference (sophiaxxiao/magi_v2) has no FFI: its boundary is the Python class surface
 * of magi_v2.py.  Each entry point below names the reference computation it replaces
 * (file:line relative to the reference tree).  The host-side mirror of that class lives in
 * magi_v2_amd/api.py and binds these symbols with ctypes; INTEGRATION.md shows the stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - plain C types only; every array is C-contiguous fp64 (or int64 where stated) and is
 *     owned by the caller; no pointer outlives the call except the opaque handle.
 *   - host layout of trajectories follows the reference: X[chain][N][D] (row-major [N,D]).
 *   - every int-returning function returns 0 on success and a negative MAGI_E_* code on
 *     failure; magi_last_error() gives the message (pass NULL for creation failures).
 *   - one handle per GPU; a handle is not thread-safe; different handles may be driven from
 *     different host threads.
 */
#ifndef MAGI_HIP_H
#define MAGI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct magi_handle magi_handle;

enum {
    MAGI_OK = 0,
    MAGI_E_BADARG = -1,   /* shape / pointer / state error                              */
    MAGI_E_HIP = -2,      /* a HIP runtime call failed                                  */
    MAGI_E_NOTSPD = -3,   /* Cholesky met a non-positive pivot (index in the message)   */
    MAGI_E_NAN = -4,      /* NaN in an initial state (reference asserts magi_v2.py:289-291) */
    MAGI_E_STATE = -5     /* call order violated (e.g. sampling before set_problem)     */
};

/* compiled-in ODE drifts f(t, X, theta) with analytic Jacobians:
 *   SEIR3: vignette.ipynb cell 3 (S implicit; theta = beta, gamma, sigma)
 *   SEIR4: the four data columns with S explicit (data/SEIR_seed=0.csv:1)
 *   SIRW : test_magi_script.py:19-45 (theta = beta, phi, xi, chi, kappa)          */
enum { MAGI_DRIFT_SEIR3 = 0, MAGI_DRIFT_SEIR4 = 1, MAGI_DRIFT_SIRW = 2,
       MAGI_DRIFT_USER = 3 /* only in a library specialised for a traced f_vec, see magi_user_drift_info */ };

enum { MAGI_MODE_NUTS = 0, MAGI_MODE_HMC = 1 };

/* Generic ODEs (callers magi_v2.py:155, 206, 335 pass an arbitrary f_vec): magi_v2_amd.drift traces the callable,
 * emits DriftT<MAGI_DRIFT_USER> and magi_v2_amd.jit compiles this library's kernels for it.  Returns 1 and fills
 * D, P when this library was built that way (it then accepts ONLY drift = MAGI_DRIFT_USER), else 0. */
int magi_user_drift_info(int* D, int* P);

/* 1 when this library was built for a traced f_vec that uses its first argument t, else 0 (the base library, a library built for a
 * drift that ignores t).  Such a library evaluates the drift of grid point i at the time t[i] given to magi_set_times. */
int magi_user_drift_time_dependent(void);

/* ---- lifetime --------------------------------------------------------------------------- */

/* Binds device `device_id`, creates the stream.  NULL on failure (see magi_last_error(NULL)). */
magi_handle* magi_create(int device_id);
void magi_destroy(magi_handle* h);
const char* magi_last_error(const magi_handle* h);
/* "magi_hip <version> gfx950" */
const char* magi_version(void);

/* ---- kernel matrices ---------------------------------------------------------------------- */

/* Replaces MAGI_v2._build_matrices (magi_v2.py:774-823), the pinv sites (magi_v2.py:126,128 /
 * 266,268 / 449,451) and the band approximation (magi_v2.py:271-274) for all D components:
 * Matern(nu) Kappa / p_Kappa / Kappa_pp assembly on the grid I[N], fp64 blocked Cholesky,
 * m = p_Kappa Kappa^-1, K = Kappa_pp - p_Kappa Kappa^-1 Kappa_p, C^-1, K^-1, band mask.
 * bandsize < 0 means dense.  The results stay resident on the device for the log-posterior
 * and sampler calls; C_inv / m / K_inv ([D][N][N] row-major host buffers) may each be NULL
 * when the caller does not want a host copy.  I need not be sorted for the dense outputs (row / column i belongs to I[i]);
 * `bandsize` and the banded packing assume a sorted grid. */
int magi_build_matrices(magi_handle* h, const double* I, int N, int D,
                        const double* phi1, const double* phi2, double nu, int bandsize,
                        double* C_inv, double* m, double* K_inv);

/* GP hyper-parameter fit: replaces MAGI_v2._fit_kernel_hparams (magi_v2.py:538-691) -- Adam (tf_keras defaults,
 * `learning_rate`, `num_iters` steps) on the softplus-reparameterised (phi1, phi2, sigma^2) of every component,
 * maximising  D * sum_d [ log N(x_d ; mu_d, phi1_d R_nu(phi2_d) + (sigma_d^2 + jitter) I) + TruncatedNormal priors ]
 * with the reference's priors (magi_v2.py:611-627: loc 1e-4 / sigma_sq_loc / mu_phi2, scales 1000 sqrt(D) /
 * 1000 sqrt(D) / sd_phi2 sqrt(D)).  X_filled[N][D] row-major (no NaN), mu[D] the GP means (magi_v2.py:559).
 * phi1 / phi2 / sigma_sq hold the starting values on entry (magi_v2.py:631-639) and the fitted values on return.
 * Every step is Matern assembly + Cholesky + inverse + trace terms on the GPU; loss_trace[num_iters] may be NULL.
 * jitter: TFP's GaussianProcess default 1e-6.  I need not be sorted (row n of X_filled belongs to I[n]); priors and starting values are
 * the caller's. */
int magi_fit_hparams(magi_handle* h, const double* I, int N, int D, const double* X_filled, const double* mu,
                     const double* mu_phi2, const double* sd_phi2, const double* sigma_sq_loc, double nu,
                     int num_iters, double learning_rate, double jitter,
                     double* phi1, double* phi2, double* sigma_sq, double* loss_trace);

/* The three Matern blocks alone (magi_v2.py:781-815) for one component; host outputs [N][N].  I need not be sorted: every entry
 * is a function of (I[i], I[j]) alone, so a permuted grid gives the permuted blocks bit for bit. */
int magi_matern_blocks(magi_handle* h, const double* I, int N, double phi1, double phi2, double nu,
                       double* Kappa, double* p_Kappa, double* Kappa_pp);

/* User-overwritten or golden matrices (the reference lets users overwrite C_d_invs, m_ds,
 * K_d_invs between fit and predict, magi_v2.py:77-80).  [D][N][N] row-major.  With
 * bandsize >= 0 entries with |i-j| > bandsize are dropped exactly as tf.linalg.band_part
 * does (magi_v2.py:271-274) and the matrices are kept in banded storage N x (2b+1).
 * What a matrix change does to the problem.  magi_set_matrices and magi_build_dense forget the problem, whatever the shape: magi_set_problem
 * must follow (it resets the model), and until it has, the model calls and their getters (magi_set_theta_support, magi_set_prior,
 * magi_set_obs_model, magi_get_*) return MAGI_E_STATE like every call that needs a problem; so do magi_build_matrices and
 * magi_pack_resident when N or D change.  magi_pack_resident and magi_build_matrices at an unchanged (N, D) keep the problem AND its
 * model: mu, N_ds, beta, the observations, the supports of theta, the priors (a fixed variance stays in place of its LB entry), the
 * links with the transformed data and the weights all stay in force on the new operands, exactly as if they had been set after the
 * change.  The sampler state and the captured graph are invalidated either way: magi_sampler_init comes next. */
int magi_set_matrices(magi_handle* h, int N, int D, int bandsize,
                      const double* C_inv, const double* m, const double* K_inv);

/* The three entry points above keep dense device copies of C^-1, m, K^-1 ([D][N][N], before the band mask) resident in the
 * handle; the calls below let a caller stage its work on them without moving N x N matrices over PCIe
 * (MAGI_v2.initial_fit builds the observed components, initialises theta against the UNbanded m / K^-1, builds the
 * unobserved components later and only then applies the band: magi_v2.py:122-128, 133-179, 262-274).
 *
 * magi_build_dense: Eqn.-6 matrices of the components sel[0 .. n_sel) (phi1 / phi2 indexed like sel) into the resident
 *   stacks of a D-component problem (stacks are allocated, and zero for components not built yet, when N or D change).
 *   Invalidates the packed operands until magi_pack_resident.
 * magi_pack_resident: band mask + packing of the resident stacks (what magi_build_matrices / magi_set_matrices do last).
 * magi_get_dense: host copies of the resident stacks with tf.linalg.band_part(., b, b) applied (bandsize < 0: as built);
 *   any pointer may be NULL.
 * magi_dense_apply: Y[d] = A_d V[d] (transpose = 0) or A_d^T V[d] for the resident stack `which` (0 = C^-1, 1 = m,
 *   2 = K^-1); V, Y host [D][N][nv], nv <= 8 -- the N x N products of the theta initialiser (magi_v2.py:142, 157-158). */
int magi_build_dense(magi_handle* h, const double* I, int N, int D, int n_sel, const int32_t* sel,
                     const double* phi1, const double* phi2, double nu);
int magi_pack_resident(magi_handle* h, int bandsize);
int magi_get_dense(magi_handle* h, int bandsize, double* C_inv, double* m, double* K_inv);
int magi_dense_apply(magi_handle* h, int which, int transpose, int nv, const double* V, double* Y);

/* ---- log posterior ------------------------------------------------------------------------ */

/* Constants captured by the reference's log-posterior closure (magi_v2.py:294-300):
 * mu[D] (magi_v2.py:114,259), N_ds[D] (:53), obs_idx[n_obs] = flat row-major indices into
 * X[N][D] of the non-NaN observations (:96), y[n_obs] (:100), beta = D|I|/sum N_d (:89),
 * LB[D] (:300), the drift and its parameter count P.  Requires matrices (for N, D). */
int magi_set_problem(magi_handle* h, const double* mu, const double* N_ds,
                     const int64_t* obs_idx, const double* y, int64_t n_obs,
                     double beta, const double* LB, int drift_id, int P);

/* The times of the grid points, t[n] with n = the N of the handle's matrices (build or set them first: MAGI_E_STATE without;
 * MAGI_E_BADARG for another n or a non-finite entry) -- the reference's self.I, which it passes to f_vec as t (magi_v2.py:155, 206,
 * 335).  Read by a library whose drift depends on time (magi_user_drift_time_dependent) in magi_theta_init, magi_logpost_grad*, the
 * sampler and as a member of a group; any other library stores and ignores them.  In a time-dependent library magi_set_problem
 * without times for the current N fails with MAGI_E_STATE: nothing is ever evaluated at t = 0 silently.  The call invalidates what
 * magi_set_problem invalidates (the sampler state, the captured graph); matrices of another N forget the times.  The times are
 * independent of the grid the matrices were built on.  A group handle has none of its own: MAGI_E_STATE. */
int magi_set_times(magi_handle* h, const double* t, int n);

/* Support of every ODE parameter (opt-in; the reference has theta = softplus(theta_pre) for all of them, magi_v2.py:303-306, 319, and
 * that stays the default).  The sampler, the momentum, the metric and dual averaging act on theta_pre as before; the support of
 * parameter p decides how theta_p, d theta_p / d pre and the log-Jacobian term of the target follow from it, with
 * sp = log(1 + exp(pre)) and sg = exp(pre) / (1 + exp(pre)):
 *   MAGI_THETA_POSITIVE   theta = sp              d theta = sg     log-Jacobian pre - sp   (its derivative 1 - sg)
 *   MAGI_THETA_LOWER      theta = bound + sp      d theta = sg     log-Jacobian pre - sp   (1 - sg)
 *   MAGI_THETA_UPPER      theta = bound - sp      d theta = -sg    log-Jacobian pre - sp   (1 - sg)
 *   MAGI_THETA_REAL       theta = pre             d theta = 1      log-Jacobian 0          (0)
 * kind[P], bound[P]; the bound of a POSITIVE or REAL entry is ignored and reported as 0.  kind = NULL: back to all-POSITIVE.  A handle
 * whose support was never set, or was set to all-POSITIVE, computes bit for bit what it computed without this call (the kernels test one
 * pointer and run the instructions they ran before).  The support belongs to the problem: magi_set_problem resets it to all-POSITIVE, so
 * the call comes after it; it governs magi_logpost_grad*, the next magi_sampler_init (it invalidates the sampler state and the captured
 * graph, as magi_set_times does), the theta block of magi_sampler_summarize, and the handle as a member of a group (each member brings
 * its own; members of one group may differ).  sigma^2 is not affected.  theta_pre in and out of every call stays theta_pre.
 * Errors, each leaving the handle as it was: MAGI_E_BADARG for P other than the problem's, a kind out of range, a non-finite bound of a
 * LOWER or UPPER entry; MAGI_E_STATE before magi_set_problem and on a group handle.  Checkpoints carry the support in their tag: a
 * checkpoint taken under one support is refused under another.
 *   magi_get_theta_support   the support in force; either output may be NULL. */
enum { MAGI_THETA_POSITIVE = 0, MAGI_THETA_LOWER = 1, MAGI_THETA_UPPER = 2, MAGI_THETA_REAL = 3 };
int magi_set_theta_support(magi_handle* h, int P, const int* kind, const double* bound);
int magi_get_theta_support(magi_handle* h, int P, int* kind, double* bound);

/* Priors on the parameter entries and known noise variances (opt-in; the reference has a flat prior on every sigma^2 and theta, and that
 * stays the default).  The n = D + P entries are ordered as in the parameter block: sigma^2_0 .. sigma^2_{D-1}, then theta_0 .. theta_{P-1}.
 * A prior acts on the NATURAL scale v of its entry -- sigma^2 = softplus(pre) + LB, theta under its support -- with the unnormalised log
 * density
 *   MAGI_PRIOR_FLAT       0
 *   MAGI_PRIOR_NORMAL     a = mean m, b = sd s > 0         -(v - m)^2 / (2 s^2)
 *   MAGI_PRIOR_LOGNORMAL  a = m, b = s > 0                 -log v - (log v - m)^2 / (2 s^2)
 *   MAGI_PRIOR_GAMMA      a = shape k > 0, b = rate r > 0  (k - 1) log v - r v
 *   MAGI_PRIOR_INVGAMMA   a = shape > 0, b = scale > 0     -(a + 1) log v - b / v
 *   MAGI_PRIOR_FIXED      a = value c > 0 (sigma^2 entries only; b ignored, reported as 0)
 * The log prior joins the log-Jacobian terms of the target: beta_temp (-(1/2)((1/beta)(t1 + t2) + (t3 + t4)) + logJ + sum log p) -- tempered
 * like the rest, not divided by the prior temperature beta; the gradient with respect to pre gains (d log p / dv)(dv / dpre).
 * FIXED: sigma^2_j = c whatever pre_j is (t3, t4 use c and give that entry no gradient); the entry's log-Jacobian term is replaced by
 * -pre_j^2 / 2, so pre_j stays in the state as an independent standard-normal coordinate and the marginal of everything else is the posterior
 * with sigma^2_j = c; the sigma^2 block of magi_sampler_summarize reports c.
 * kind = NULL: back to all-FLAT.  A handle whose priors were never set, or set to all-FLAT, computes bit for bit what it computed without
 * this call (the kernels test one pointer).  The priors belong to the problem: magi_set_problem resets them, and the call comes after
 * magi_set_theta_support where both are used; it governs magi_logpost_grad*, the next magi_sampler_init (it invalidates the sampler state and
 * the captured graph), and the handle as a member of a group (each member brings its own).
 * Errors, each leaving the handle as it was: MAGI_E_BADARG for n other than D + P, a kind out of range, a missing or non-finite parameter, a
 * parameter out of its range, FIXED on a theta entry, LOGNORMAL / GAMMA / INVGAMMA on a theta entry whose support is not inside (0, inf)
 * (POSITIVE, or LOWER with bound >= 0; magi_set_theta_support in turn refuses a support an installed prior does not allow); MAGI_E_STATE
 * before magi_set_problem and on a group handle.  Checkpoints carry the priors in their tag when any is set.
 *   magi_get_prior   the priors in force; any output may be NULL. */
enum { MAGI_PRIOR_FLAT = 0, MAGI_PRIOR_NORMAL = 1, MAGI_PRIOR_LOGNORMAL = 2, MAGI_PRIOR_GAMMA = 3, MAGI_PRIOR_INVGAMMA = 4, MAGI_PRIOR_FIXED = 5 };
int magi_set_prior(magi_handle* h, int n /* D + P */, const int* kind, const double* a, const double* b);
int magi_get_prior(magi_handle* h, int n /* D + P */, int* kind, double* a, double* b);

/* Observation model (opt-in; the reference observes every component as y = x + N(0, sigma^2_d) with one variance for all its points, and
 * that stays the default).  Component d is observed through a link g_d, with Gaussian error on the LINK's scale:
 *   MAGI_LINK_IDENTITY  g(x) = x                                         (the reference)
 *   MAGI_LINK_LOG       g(x) = log x     data y > 0                      (multiplicative error)
 *   MAGI_LINK_SQRT      g(x) = sqrt x    data y >= 0                     (counts, variance-stabilised)
 * and observation k -- in the order of magi_set_problem's obs_idx -- may carry a known weight w_k > 0 (the mean of n replicates: n):
 *   t4 = sum_d (1 / sigma^2_d) sum_{k in obs_d} w_k (g_d(x_k) - g_d(y_k))^2,   t3 = sum_d N_d log(2 pi sigma^2_d) as before;
 * the constant Jacobian of the data transform and sum log w_k are dropped (the density is unnormalised).  sigma^2_d is the variance on the
 * link's scale; the GP terms, the drift, theta, the samples and every summary see x itself.  The link is evaluated at observed points
 * only: a state with x <= 0 (log) or x < 0 (sqrt) THERE has a non-finite log posterior -- magi_logpost_grad* return NaN for that state and
 * leave the others of the batch untouched, the sampler counts the leaf as energy -inf -- as for a state outside a drift's domain.
 * link = NULL: every link the identity; weight = NULL: every weight 1; both NULL: back to the default.  A handle whose model was never set,
 * or set to all-IDENTITY without weights, computes bit for bit what it computed without this call (the kernels test one scalar and one
 * pointer).  The model belongs to the problem: magi_set_problem resets it (and the handle keeps the untransformed data, so the model can be
 * changed or reset without a new magi_set_problem); it governs magi_logpost_grad*, the next magi_sampler_init (it invalidates the sampler
 * state and the captured graph), and the handle as a member of a group (each member brings its own).  A fixed sigma^2 (MAGI_PRIOR_FIXED)
 * composes with it: the constant is then the variance on the link's scale.
 * Errors, each leaving the handle as it was: MAGI_E_BADARG for D or n_obs other than the problem's, a link out of range, a weight that is
 * not finite or not > 0, a datum outside its link's domain; MAGI_E_STATE before magi_set_problem and on a group handle.  Checkpoints carry
 * the model in their tag when one is set.
 *   magi_get_obs_model   the model in force (weights 1 when none were given); either output may be NULL. */
enum { MAGI_LINK_IDENTITY = 0, MAGI_LINK_LOG = 1, MAGI_LINK_SQRT = 2 };
int magi_set_obs_model(magi_handle* h, int D, const int* link /* [D] or NULL */, int64_t n_obs, const double* weight /* [n_obs], aligned with magi_set_problem's obs_idx, or NULL */);
int magi_get_obs_model(magi_handle* h, int D, int* link, int64_t n_obs, double* weight);

/* unnormalized_log_prob (magi_v2.py:308-348) and its gradient (TF autodiff in the reference,
 * induced by magi_v2.py:360-364) for n_chains independent states.
 * X[n_chains][N][D], sig_pre[n_chains][D], th_pre[n_chains][P] -> logp[n_chains],
 * gX[n_chains][N][D], gsig[n_chains][D], gth[n_chains][P] (any output may be NULL).
 * terms, if not NULL, receives t1..t4 per chain ([n_chains][4], magi_v2.py:332-345). */
int magi_logpost_grad(magi_handle* h, int n_chains, const double* X, const double* sig_pre,
                      const double* th_pre, double beta_temp,
                      double* logp, double* gX, double* gsig, double* gth, double* terms);

/* Same quantity through the sampler's single-phase formulation: operators
 * FH = Csym + m^T Ksym m, FE = Ksym m, FE^T, Ksym are applied to xc and f(X, theta) in ONE streaming
 * kernel.  Exposed so the formulation the sampler runs can be validated against the reference
 * op order above; terms = {t1 + t2, 0, t3, t4}. */
int magi_logpost_grad_fused(magi_handle* h, int n_chains, const double* X, const double* sig_pre,
                            const double* th_pre, double beta_temp,
                            double* logp, double* gX, double* gsig, double* gth, double* terms);

/* ---- sampler ------------------------------------------------------------------------------ */

/* Replaces the TFP wiring of predict (magi_v2.py:357-396) and LogAnnealedNUTS
 * (magi_v2.py:838-889).  Defaults via magi_sampler_cfg_default() are the reference's. */
typedef struct magi_sampler_cfg {
    int32_t num_results;          /* magi_v2.py:390                                         */
    int32_t num_burnin_steps;     /* magi_v2.py:391                                         */
    int32_t num_adaptation_steps; /* < 0 -> int(0.8 * num_burnin_steps), magi_v2.py:365     */
    int32_t max_tree_depth;       /* TFP default 10                                         */
    int32_t mode;                 /* MAGI_MODE_NUTS (reference) or MAGI_MODE_HMC (fixed L)  */
    int32_t hmc_leapfrogs;        /* L for MAGI_MODE_HMC                                    */
    int32_t anneal;               /* 1: beta_temp(k) = max(1/ln(k+2), min_temp), :833-835   */
    int32_t stale_cache;          /* 1: reuse the previous step's cached target/grad as TFP
                                     does (computed at the previous temperature)            */
    double step_size;             /* 0.1, magi_v2.py:364                                    */
    double target_accept_prob;    /* 0.75, magi_v2.py:366                                   */
    double max_energy_diff;       /* TFP default 1000                                       */
    double min_temp;              /* 0.1, magi_v2.py:357                                    */
} magi_sampler_cfg;

void magi_sampler_cfg_default(magi_sampler_cfg* cfg);

/* Start n_chains independent chains from pre-transformed states (the softplus-inverse inits
 * of magi_v2.py:374-383 are formed by the host layer).  chain_ids[n_chains] (may be NULL =
 * 0..n-1) select the Philox stream of each chain so results do not depend on how chains are
 * sharded over GPUs.  Fails with MAGI_E_NAN when a state holds NaN (magi_v2.py:289-291). */
int magi_sampler_init(magi_handle* h, const magi_sampler_cfg* cfg, int n_chains,
                      const double* X0, const double* sig_pre0, const double* th_pre0,
                      uint64_t seed, const int64_t* chain_ids);

/* Advance every chain by up to n_steps transitions (burn-in steps count); blocks until done.
 * leapfrogs_done, if not NULL, receives the gradient evaluations taken in this call (sum over
 * chains); kernel_ms the device time between the first and last launch of the call.
 * Between two magi_sampler_run calls of one run the chains stand at a transition boundary, and the calls that need the handle only for
 * its device, its stream or its resident dense matrices may be made: magi_summarize, magi_rank_diagnostics, magi_elpd, magi_gp_predict, magi_matern_cross,
 * magi_ode_solve, magi_ode_solve_adaptive, magi_dense_apply, magi_theta_init (it captures a graph of its own on the same stream) and
 * magi_fit_hparams; magi_sampler_rank_diagnostics too (it answers MAGI_E_STATE while a selected chain is unfinished and touches nothing
 * either way).  Each works in memory of its own, touches neither the chains, the problem nor the sampler's captured graph, and has
 * finished on the stream when it returns: the continued run is the uninterrupted one bit for bit.  (The calls that end a paused run
 * say so where they are declared: a matrix, problem, times or model change, magi_logpost_grad*, magi_time_gradient and
 * magi_sampler_profile -- the next magi_sampler_run then returns MAGI_E_STATE.)  Option "no_graph" may be switched between two calls
 * as well: direct launches and graph replay run the same kernels on the same arguments. */
int magi_sampler_run(magi_handle* h, int n_steps, int64_t* leapfrogs_done, double* kernel_ms);

/* Steps completed so far per chain (burn-in included). */
int magi_sampler_steps_done(magi_handle* h, int64_t* steps /* [n_chains] */);

/* Post-burn-in samples, pre-transform (sample_results of magi_v2.py:421):
 * X[n_chains][num_results][N][D], sig_pre[n_chains][num_results][D], th_pre[..][P]. */
int magi_sampler_get_samples(magi_handle* h, double* X, double* sig_pre, double* th_pre);

/* Per-step diagnostics for ALL steps taken so far (burn-in included), each [n_chains][n_total]
 * with n_total = num_burnin_steps + num_results; any pointer may be NULL.  These are the
 * NUTSKernelResults fields the reference traces (magi_v2.py:394). */
int magi_sampler_get_diag(magi_handle* h, double* step_size, double* log_accept_ratio,
                          int32_t* leapfrogs_taken, int32_t* tree_depth, int32_t* has_divergence,
                          int32_t* reach_max_depth, int32_t* is_accepted,
                          double* target_log_prob, double* energy, double* beta_temp);

/* Problem groups: ONE sampler over the chains of n_members problems of the same shape on one GPU -- one captured graph, one
 * [stream, point] kernel pair per leapfrog slot for all of them, one host thread (many small datasets: the GPU is mostly idle in one
 * problem's slot at N = 161).  members: handles of this library on one device, each with its matrices built / set and packed and
 * magi_set_problem done; they must agree in every shape (N, D, P, band, drift and what follows from them) and may differ in all their
 * data (matrices, observations, mu, N_ds, LB, beta).  *out receives a handle flagged as a group; on failure *out is NULL, the return
 * value is negative and magi_last_error(NULL) gives the message (mismatched shapes, a member without a problem, NULL members).
 *   - magi_sampler_init on a group takes n_chains = n_members x C states and chain ids, problem-major (C per member, ids may repeat
 *     across members), one cfg and one seed: the chains of member m then reproduce magi_sampler_init(member m, cfg, C, <its states>,
 *     seed, <its ids>) bit for bit.  It reads the members' problems as they stand at that call (a member changed later takes effect at
 *     the next magi_sampler_init), and rejects (MAGI_E_BADARG) n_chains that is not a multiple of n_members and a member whose own
 *     rule (magi_stream_kernel_name, option stream_family) would stream C chains on a matrix-core kernel: a group runs the VALU kernels
 *     k_stream_group<2> (C even) / k_stream_group<1> (C odd) only -- at N = 161, band 80 up to C = 16.
 *   - magi_sampler_run, _steps_done, _get_samples, _get_diag, _get_state, _run_stats, _profile, magi_sample, magi_set_option and
 *     magi_stream_kernel_name work on a group as on a handle, over all n_chains chains.
 *   - the calls that need matrices of their own return MAGI_E_STATE: matrix builds, magi_set_matrices, magi_set_problem, magi_logpost_grad*,
 *     the dense-stack calls, magi_fit_hparams, magi_theta_init, magi_time_gradient, magi_sampler_get_checkpoint / _set_checkpoint.
 *   - the group owns its chain buffers, stream, graph and a device copy of the members' problems, not the members: they must outlive
 *     it (magi_destroy(group) frees only what the group owns) and must not be re-built while it samples. */
int magi_group_create(magi_handle* const* members, int n_members, magi_handle** out);

/* Current state of every chain (checkpoint / hand-over to the CPU oracle in tests):
 * X[n_chains][N][D], sig_pre, th_pre, step_size[n_chains] (the dual-averaging "new step
 * size"), beta_cache[n_chains] (temperature at which the cached target was computed). */
int magi_sampler_get_state(magi_handle* h, double* X, double* sig_pre, double* th_pre,
                           double* step_size, double* beta_cache);

/* Checkpoint / resume (the reference has none: a run is all-or-nothing, magi_v2.py:386-425).  Between two magi_sampler_run
 * calls every chain stands at a transition boundary; its state is (X, sig_pre, th_pre) from magi_sampler_get_state plus
 * MAGI_CKPT_SCALARS doubles per chain from magi_sampler_get_checkpoint (transition index, dual-averaging state, cached
 * temperature, leapfrog count).  To resume -- in this or another process / handle: magi_sampler_init with the SAME cfg, seed
 * and chain_ids and the checkpointed states, then magi_sampler_set_checkpoint(scalars), then magi_sampler_run: the remaining
 * transitions are those the uninterrupted run would have made, bit for bit (the Philox streams are keyed by transition index
 * and chain id; target and gradient of the restored state are re-evaluated by the same kernels).  Samples and diagnostics of
 * the steps taken before the checkpoint belong to the run that took them.  The scalars carry a tag of (cfg, seed, chain id,
 * state size): magi_sampler_set_checkpoint rejects (MAGI_E_BADARG) a checkpoint taken under anything else, and any scalar that
 * is not finite / not a whole number where one is expected / outside its range. */
#define MAGI_CKPT_SCALARS 16
int magi_sampler_get_checkpoint(magi_handle* h, double* scalars /* [n_chains][MAGI_CKPT_SCALARS] */);
int magi_sampler_set_checkpoint(magi_handle* h, const double* scalars /* [n_chains][MAGI_CKPT_SCALARS] */);

/* Diagonal mass matrix (opt-in; TFP's NoUTurnSampler, hence the reference, has the identity metric only, and that stays the default).
 * A chain's metric is its inverse mass per entry of the state, in the host layouts of magi_sampler_init: inv_mass_X[n_chains][N][D],
 * inv_mass_sig[n_chains][D], inv_mass_th[n_chains][P].  With M^-1 = diag(s^2) the device keeps the WHITENED momentum (HMC on z = q / s
 * with the identity metric): the momentum draw, the kinetic energy, the U-turn tests, the energies and every diagnostic are those of
 * the identity metric on z, and s enters the two updates p_half = p + eps/2 (s . grad), q' = q + eps (s . p_half) alone.  The reference
 * run of a chain under metric s is therefore the oracle's NUTS / HMC step on z with fn(z) = (L(s . z), s . grad L(s . z)) and the same
 * Philox draws.  All four calls return MAGI_E_STATE before magi_sampler_init, which resets every chain to the identity metric with no
 * window open; they work on a group handle as on a handle (over all its chains).
 *   magi_sampler_set_metric   all three pointers NULL: back to the identity metric; else all three non-NULL, every entry finite and
 *       > 0 (MAGI_E_BADARG otherwise, nothing changed).  Legal between magi_sampler_run calls: the chains stand at a transition
 *       boundary with nothing of the next transition staged, so the new metric governs it from its first half step.
 *   magi_sampler_get_metric   the metric in force (ones under the identity metric); any pointer may be NULL.
 *   magi_sampler_metric_window(on)   1: open a window -- shift := the state every chain holds now, sums := 0; from now on the state a
 *       chain holds after each finished transition is added on the device.  0: close it without adapting.
 *   magi_sampler_adapt_metric   the open window -> the metric: per chain and entry, var = sample variance (ddof 1) of the n window
 *       states, inverse mass = n / (n + kappa) var + kappa / (n + kappa) rel_floor median(var) (the median over the chain's entries:
 *       a floor RELATIVE to the chain's own scale; Stan's constants are kappa = 5, and 1e-3 for its absolute floor).  n must be the
 *       number of transitions every chain has finished since the window was opened, n >= 2 (MAGI_E_BADARG otherwise, nothing changed,
 *       the window stays open).  A chain whose median variance is 0 or whose window holds a non-finite state keeps its metric; the call
 *       returns the number of such chains (>= 0; errors are negative).  restart_adapt_steps >= 0: dual averaging of every chain
 *       restarts at eps_new = eps_old min(s_old) / min(s_new) -- the step along the stiffest coordinate is kept; eps_old for a chain
 *       that kept its metric -- as a fresh DualAveragingStepSizeAdaptation(eps_new), and the sampler's num_adaptation_steps becomes
 *       restart_adapt_steps (counted from the restart).  restart_adapt_steps < 0: step size and adaptation are left alone.  step_size_out[n_chains] (may be NULL):
 *       every chain's step size after the call.  The window is closed.  (The metric is written in place and the dual-averaging state
 *       uploaded behind it: a MAGI_E_HIP from this call leaves the sampler undefined until the next magi_sampler_init.)
 * A call that switches between "no metric" and "a metric", or opens / closes a window, rebuilds the captured graph at the next
 * magi_sampler_run (the pointers are kernel arguments): keep such switches to one per window.
 * Checkpoints do not carry the metric: resume with magi_sampler_init (num_adaptation_steps = the value in force when the checkpoint was
 * taken), then magi_sampler_set_metric(what magi_sampler_get_metric returned), then magi_sampler_set_checkpoint. */
int magi_sampler_set_metric(magi_handle* h, const double* inv_mass_X, const double* inv_mass_sig, const double* inv_mass_th);
int magi_sampler_get_metric(magi_handle* h, double* inv_mass_X, double* inv_mass_sig, double* inv_mass_th);
int magi_sampler_metric_window(magi_handle* h, int on);
int magi_sampler_adapt_metric(magi_handle* h, int n, double kappa, double rel_floor, int restart_adapt_steps, double* step_size_out /* [n_chains] */);

/* One-call form: init + run(num_burnin + num_results) + get_samples. */
int magi_sample(magi_handle* h, const magi_sampler_cfg* cfg, int n_chains,
                const double* X0, const double* sig_pre0, const double* th_pre0,
                uint64_t seed, const int64_t* chain_ids,
                double* X_samps, double* sig_pre_samps, double* th_pre_samps);

/* theta initialiser of initial_fit (magi_v2.py:133-179): Adam(learning_rate) x num_iters, from theta[P] as passed
 * in (the reference starts at 1), on theta_objective = sum_d toNorm_d^T K_d^-1 toNorm_d with toNorm = reshape(f(Xhat, theta),
 * [D, N, 1]) - m_d (Xhat - mu)_d -- including the reference's reshape (:155-156) -- evaluated with the device-resident UNbanded
 * m and K^-1 stacks (the initialiser runs before the band approximation).  The whole loop stays on the device: one captured graph
 * per Adam step (drift values + theta-Jacobian, K^-1 r, K^-T r, reduction + update), the host waits once.  Xhat[N][D] row-major,
 * mu[D]; theta[P] in/out; loss_trace[num_iters] (optional) receives the objective at every step.  tf_keras Adam restated from its
 * documented defaults: parity unpinned. */
int magi_theta_init(magi_handle* h, int drift_id, int P, const double* Xhat, const double* mu, int num_iters, double learning_rate,
                    double* theta, double* loss_trace);

/* ---- self-test ------------------------------------------------------------------------------- */

/* Drift probe: evaluate THIS library's drift code by itself at n points, through the members the production kernels call (new
 * unit csrc/selftest.hip; nothing is re-derived inside it).  magi_v2_amd/selftest.py holds the result against the expressions the code
 * was generated from (a traced f_vec: the sympy evaluators of the same trace) before a freshly built library is first used.
 * x[n][D], th[P] (transformed parameters, as the drift sees them), g[n][D] ->
 * f[n][D], c[n][D] (c_k = sum_d g_d df_d/dx_k), t[n][P] (t_p = sum_d g_d df_d/dtheta_p).
 *   path 0: DriftT<>::f / jt (what k_point and the theta initialiser inline)
 *   path 1: the runtime-switch entries drift_f / drift_jt_g / drift_tt_g_acc (what the three-phase kernels call; for a traced drift
 *           the generated user_drift_f / user_drift_jt)
 *   path 2: the separable members (DriftT<>::coefs(theta), ::basis(x); what k_stream_sep and its point phase consume):
 *           f_d = sum_k coefs[d][k] * basis[d][k] only, c and t are not written (g, c, t may be NULL);
 *           MAGI_E_BADARG if DriftT<>::SEP is false
 *   path 3: DriftT<>::f1(d, ..) per component (what the streaming kernels k_stream / k_stream_mc inline); f only, as path 2
 * Needs a handle only for its device and stream: no matrices, no problem; a group handle is fine.  1 <= n <= 2^20. */
int magi_drift_probe(magi_handle* h, int drift_id, int P, int path, int n,
                     const double* x, const double* th, const double* g,
                     double* f, double* c, double* t);
/* magi_drift_probe with a time per point, tt[n] (NULL: every point at time 0, which is what magi_drift_probe does). */
int magi_drift_probe_at(magi_handle* h, int drift_id, int P, int path, int n,
                        const double* x, const double* th, const double* g,
                        double* f, double* c, double* t, const double* tt);

/* ---- posterior trajectories ------------------------------------------------------------------ */

/* Integrate THIS library's drift (DriftT<>::f, the arithmetic the sampler ran) for S draws at once, one lane per draw (unit
 * csrc/ode.hip): draw s starts at x0[s][D] with the parameters theta[s][P] (natural scale, as the drift sees them) and is reported at
 * the T times t_out (finite, strictly increasing; output 0 is x0 itself).
 * Scheme: classical RK4 with `substeps` steps per output interval, exactly magi_v2_amd.drift_examples.rk4: h = (t[j+1] - t[j]) /
 * substeps, sub-step k starts at s = t[j] + k h, stages at s, s + h/2, s + h/2, s + h, x += h/6 (k1 + 2 k2 + 2 k3 + k4).  A drift
 * that does not use t is given the constant 0.
 * status[s]: 0 when every output of draw s is finite, else j + 1 for the first interval [t[j], t[j+1]] whose output has a non-finite
 * component -- the index of the first non-finite output, 1 for a non-finite x0 (the outputs after it hold whatever the arithmetic
 * gives; other draws are not affected).  n_failed: draws with status != 0.
 * mean / sd [T][D]: mean and sample standard deviation (ddof = 1) over the draws with status 0, two passes in a fixed summation
 * order (bit-identical from run to run); the mean is NaN when no draw qualifies, the sd when fewer than two do.
 * traj[S][T][D], mean, sd, status, n_failed: each optional (NULL: not computed / not copied).
 * Drift ids as magi_drift_probe_at.  MAGI_E_BADARG (handle stays usable): S outside [1, 2^20], T outside [2, 2^16], substeps outside
 * [1, 1024], roundup(S, 64) T D > 2^28 (a 2 GiB device buffer), a wrong P, a NULL x0 / theta / t_out, a t_out that is not finite or
 * not strictly increasing.  Needs a handle only for its device and stream: no matrices, no problem; a group handle is fine. */
int magi_ode_solve(magi_handle* h, int drift_id, int P, int S,
                   const double* x0, const double* theta,
                   int T, const double* t_out, int substeps,
                   double* traj, double* mean, double* sd, int* status, int* n_failed);

/* The same draws integrated with error control (unit csrc/ode_adaptive.hip, one lane per draw like magi_ode_solve), for when no fixed `substeps`
 * is right: a stated tolerance, and stiff systems.  x0, theta, T, t_out, traj, mean, sd, status and n_failed mean what they mean in
 * magi_ode_solve.
 * method  MAGI_ODE_DOPRI5: Dormand-Prince 5(4), seven stages with the first the last of the step before (FSAL), advancing with the
 *           5th-order weights b; err = h sum (b_i - b*_i) k_i; q = 5.
 *         MAGI_ODE_ROS23: the Shampine-Reichelt modified Rosenbrock 2(3) pair (ode23s), for stiff draws.  d = 1 / (2 + sqrt 2),
 *           e32 = 6 + sqrt 2, J = df/dx and T = df/dt at (t, y) (T = 0 unless the traced drift uses t), W = I - h d J factored once per
 *           trial step by LU with partial pivoting;
 *             k1 = W^-1 (F0 + h d T),  F1 = f(t + h/2, y + h/2 k1),  k2 = W^-1 (F1 - k1) + k1,  y+ = y + h k2,  F2 = f(t + h, y+),
 *             k3 = W^-1 [F2 - e32 (k2 - F1) - 2 (k1 - F0) + h d T],  err = h/6 (k1 - 2 k2 + k3);  q = 3;  F2 is the next step's F0.
 * Controller (both methods).  h: the proposed step, first h0 if h0 > 0, else t_out[1] - t_out[0].  In interval j the trial step is
 *   h_trial = min(h, t_out[j+1] - t); a clipped step ends at t_out[j+1] itself: steps land exactly on every output time, there is no
 *   dense output.  A step is also clipped (stretched by less than 16 ulp) when h would leave less than 16 ulp(t_out[j+1]) of the
 *   interval: on a uniform grid h is often the interval's width up to rounding, and the remainder would be a step that underflows.
 *   errn = max_d |err_d| / (atol + rtol max(|y_d|, |y+_d|));  fac = clamp(0.9 errn^(-1/q), 0.2, 5), 5 when errn = 0.
 *   A trial with a non-finite |err_d| / (...) or y+_d, or a W with a pivot that is 0 or not finite, is rejected with fac = 0.2.
 *   errn <= 1: accepted; the step accepted right after a rejection does not grow (fac <- min(fac, 1)); h <- h_trial fac, and after a
 *     clipped step h <- max(h, h_trial fac), so that a dense output grid does not ratchet the step down.
 *   errn > 1: rejected, h <- h_trial min(fac, 1).
 *   Before every trial: accepted + rejected >= max_steps ends the draw with reason 2; h_trial < 16 ulp(t) ends it with reason 3.
 * reason[s]: 0 none, 1 non-finite state (x0), 2 step budget, 3 step underflow.  For reasons 2 and 3 status[s] is j + 1 of the interval
 *   that was not completed (1 for reason 1), and the outputs from there on are NaN: status keeps its meaning.  n_accepted[s],
 *   n_rejected[s]: the steps of draw s.  reason, n_accepted, n_rejected [S]: optional like the other outputs.
 * MAGI_E_BADARG (handle stays usable): the cases of magi_ode_solve (substeps aside); an unknown method; rtol outside [1e-13, 1e-1]; atol
 * < 0; rtol or atol not finite; h0 < 0 or not finite; max_steps outside [1, 2^24]. */
enum { MAGI_ODE_DOPRI5 = 1, MAGI_ODE_ROS23 = 2 };
int magi_ode_solve_adaptive(magi_handle* h, int drift_id, int P, int S,
                            const double* x0, const double* theta,
                            int T, const double* t_out, int method,
                            double rtol, double atol, double h0, int max_steps,
                            double* traj, double* mean, double* sd, int* status, int* reason,
                            int* n_accepted, int* n_rejected, int* n_failed);

/* ---- forward sensitivities and Fisher information ---------------------------------------------- */

/* Forward sensitivities of the trajectories of magi_ode_solve, and the Fisher information of a list of observations, per draw (unit
 * csrc/sens.hip): which parameters and initial states the solution depends on, through which components and times.  x0, theta, T,
 * t_out, substeps, traj, status and n_failed mean what they mean in magi_ode_solve (status looks at the state alone).
 * Columns: cols[c] in [0, P + D), distinct; q < P is theta_q, q >= P is component q - P of x0.  One lane per (draw, column).
 * Scheme: the variational equations beside the state, on the RK4 steps of magi_ode_solve restated: h = (t[j+1] - t[j]) / substeps,
 * stages at s, s + h/2, s + h/2, s + h, x += h/6 (k1 + 2 k2 + 2 k3 + k4).  With y_i = x + a_i h k_{i-1} the stage state and
 * z_i = s + a_i h l_{i-1} the stage sensitivity (a = 0, 1/2, 1/2, 1),
 *   l_i[d] = sum_k J_x[d][k](t_i, y_i) z_i[k] (k ascending) + dF[d](t_i, y_i),    s += h/6 (l1 + 2 l2 + 2 l3 + l4),
 * J_x = df/dx; dF = df/dtheta_q for q < P with s(t_0) = 0, and dF = 0 for q = P + e with s(t_0) = the unit vector e.  Rows of J_x and
 * df/dtheta come from DriftT<>::jt with unit vectors, at the stage's own y and time.  This is the exact derivative of the discrete map
 * that magi_ode_solve computes, not an approximation of it.  relative != 0: the stored value is s times the draw's own theta_q or x0
 * component (one multiply; the sensitivity to the log parameter); the integration itself is not scaled.
 * sens[S][T][D][n_col]; sens_mean / sens_sd [T][D][n_col]: mean and sd (ddof = 1) over the draws with status 0, as magi_ode_solve's.
 * Fisher information of n_obs observations (j_k, d_k, w_k) = (obs_j, obs_comp, obs_weight; obs_weight NULL: 1), links g_d = link[d]
 * (MAGI_LINK_*; NULL: identity) and the draw's variances sigma_sq[s][d] on the link's scale:
 *   F[s][a][b] = sum_k ((w_k / sigma_sq[s][d_k]) g'(x)^2) sens[s][j_k][d_k][a] sens[s][j_k][d_k][b],   x = traj[s][j_k][d_k],
 * g' = 1 (identity), 1 / x (log), 0.5 / sqrt(x) (sqrt); k ascending, no atomics; computed for a <= b and mirrored; the sens are the stored
 * ones (scaled when relative).  A draw with status != 0 or with a non-finite entry has NaN in all of F[s] and counts in
 * *n_fim_excluded; fim_mean[n_col][n_col] is the mean over the other draws in the fixed order of magi_ode_solve's mean.  n_obs = 0: no
 * Fisher information (fim, fim_mean, n_fim_excluded are not written).
 * traj, sens, sens_mean, sens_sd, fim [S][n_col][n_col], fim_mean, status, n_failed, n_fim_excluded: each optional.
 * MAGI_E_BADARG (handle stays usable): the cases of magi_ode_solve; n_col outside [1, P + D], cols NULL, a column out of range or
 * repeated; roundup(S, 64) T D n_col > 2^28; n_obs < 0 or > 2^24; with n_obs > 0: obs_j or obs_comp NULL, an obs_j outside [0, T), an
 * obs_comp outside [0, D), a weight or sigma_sq that is not a finite number > 0, sigma_sq NULL, a link that is none of MAGI_LINK_*.
 * Needs a handle only for its device and stream: no matrices, no problem; a group handle is fine. */
int magi_ode_sensitivities(magi_handle* h, int drift_id, int P, int S,
                           const double* x0, const double* theta,
                           int T, const double* t_out, int substeps,
                           int n_col, const int* cols, int relative,
                           int n_obs, const int* obs_j, const int* obs_comp, const double* obs_weight /* NULL: 1 */,
                           const double* sigma_sq /* [S][D] */, const int* link /* [D] or NULL */,
                           double* traj, double* sens, double* sens_mean, double* sens_sd,
                           double* fim, double* fim_mean, int* status, int* n_failed, int* n_fim_excluded);

/* magi_ode_sensitivities for the finished run's device-resident samples of the chains [chain0, chain0 + n_sel), every `thin`-th result
 * of each (results 0, thin, 2 thin, ...: S = n_sel ceil(num_results / thin) draws, chain-major): no draw crosses to the host first.  Draw
 * inputs: x0 = the draw's X at grid row start_index; theta on its natural scale under the handle's supports (magi_set_theta_support);
 * sigma_sq exactly what magi_sampler_ppc forms (softplus(sig_pre) + LB, or the MAGI_PRIOR_FIXED constant); links and weights are those of
 * the handle's observation model (magi_set_obs_model) -- on a group handle all of these are the member's own.  The drift is the
 * problem's.  grid_out[N]: the index in t_out of grid point i, or -1 (NULL: no Fisher information).  The observation list is the observed
 * entries e = d N + i in ascending e with grid_out[i] >= 0, as (grid_out[i], d, weight); *n_obs_used and obs_index[n_obs_used] (room for
 * N D) return it as magi_sampler_elpd does.  x0_out [S][D], theta_out [S][P], sigma_sq_out [S][D]: the draws as they were used.
 * The result is bit for bit what magi_ode_sensitivities returns for those draws, that list and the same t_out, substeps, cols and
 * relative.  Every output is optional.  State and argument errors: those of magi_sampler_summarize (MAGI_E_STATE unless the sampler is
 * initialised and the chains have finished; MAGI_E_BADARG for a chain range outside the sampler's or across two members of a group) and
 * those of magi_ode_sensitivities; MAGI_E_BADARG also for thin < 1, a start_index outside [0, N), a grid_out entry outside [-1, T).
 * Nothing of the handle's state changes: a call between two magi_sampler_runs does not disturb the chains. */
int magi_sampler_sensitivities(magi_handle* h, int chain0, int n_sel, int thin, int start_index,
                               int T, const double* t_out, int substeps, const int* grid_out,
                               int n_col, const int* cols, int relative,
                               double* traj, double* sens, double* sens_mean, double* sens_sd,
                               double* fim, double* fim_mean, int* status, int* n_failed, int* n_fim_excluded,
                               int* n_obs_used, int* obs_index,
                               double* x0_out, double* theta_out, double* sigma_sq_out);

/* ---- posterior summaries and convergence diagnostics ----------------------------------------- */

/* Summaries of K scalar columns of C chains x R draws (unit csrc/summary.hip; what the reference's notebooks do on the host with
 * X_samps.mean(axis=0) and np.quantile(X_samps, [0.025, 0.975], axis=0), plus the mixing diagnostics it has none of).  draws: host
 * [C][R][K].  Per column, with S = C R pooled draws:
 *   mean, sd      two passes in a fixed summation order (bit-identical from run to run); sd with ddof = 1, NaN when S < 2.
 *   quant[q][k]   v = the sorted pooled draws (exact order statistics), h = (S - 1) probs[q], lo = floor(h), g = h - lo:
 *                 v[lo] + g (v[min(lo + 1, S - 1)] - v[lo])   (numpy's "linear" method).
 *   rhat          split R-hat: n = R / 2, M = 2 C split chains (rows [0, n) and [R - n, R) of every chain: an odd R drops the middle draw),
 *                 their means ybar_m and variances s2_m (ddof = 1); W = mean_m s2_m, B/n = var_m(ybar_m, ddof = 1),
 *                 var+ = (n - 1) / n W + B/n, rhat = sqrt(var+ / W).
 *   ess           acov_m(t) = 1/n sum_{i < n - t} (y_i - ybar_m)(y_{i+t} - ybar_m); rho_0 = 1, rho_t = 1 - (W - mean_m acov_m(t)) / var+ for
 *                 1 <= t <= L = min(n - 1, max_lag) (max_lag <= 0: n - 1); pairs P_k = rho_{2k} + rho_{2k+1} for every k with 2 k + 1 <= L;
 *                 K* = the first k with P_k < 0 (the number of pairs if there is none); for k = 1 .. K* - 1 in turn P_k = min(P_k, P_{k-1});
 *                 tau = max(-1 + 2 sum_{k < K*} P_k, 1 / log10(M n)); ess = M n / tau.
 *   mcse_mean     sd / sqrt(ess).
 * rhat, ess and mcse_mean are NaN when R < 4.  A constant column (its smallest and largest draw are equal) has sd = 0 exactly and NaN
 * rhat, ess, mcse_mean.  A column with a non-finite draw has NaN in every statistic and counts in *n_nonfinite.
 * mean, sd, rhat, ess, mcse_mean [K], quant [n_q][K], n_nonfinite: each optional (NULL: not copied).
 * MAGI_E_BADARG (handle stays usable): C outside [1, 4096], R outside [1, 2^20], C R > 2^22, K outside [1, 2^24], n_q outside [0, 16],
 * a prob outside [0, 1] or not finite, draws NULL.  Needs a handle only for its device and stream: no matrices, no problem; a group
 * handle is fine.  Device memory of a call: the columns are gathered in chunks of at most
 * 64 MiB, with a staging buffer of the same size for the strided upload and at most 32 MiB of split-chain means -- 160 MiB whatever K is --
 * plus the result arrays, (5 + n_q) K doubles, which grow with K (2.8 GB at K = 2^24, n_q = 16; 0.7 MB at the sampler's K = 4096). */
int magi_summarize(magi_handle* h, int C, int R, int K, const double* draws,
                   int n_q, const double* probs, int max_lag,
                   double* mean, double* sd, double* quant, double* rhat, double* ess, double* mcse_mean,
                   int* n_nonfinite);

/* The same statistics of the sampler's device-resident post-burn-in samples, pooled over the chains [chain0, chain0 + n_sel): nothing
 * but the summaries crosses to the host (magi_sampler_get_samples moves every draw).  Three blocks of columns, each with the six
 * outputs of magi_summarize: X in the host layout ([N][D]; quant [n_q][N][D]) as stored, sigma_sqs [D] = softplus(sig_pre) + LB[d] and
 * thetas [P] = softplus(th_pre) (magi_v2.py:418-419); *n_nonfinite counts the columns of all three.  Every output is optional.
 * MAGI_E_STATE unless the sampler is initialised and every selected chain has finished all num_burnin_steps + num_results
 * transitions.  MAGI_E_BADARG: a chain range outside the sampler's chains, n_sel > 4096 or n_sel num_results > 2^22, n_q / probs as
 * magi_summarize; on a group handle a range that does not lie inside one member (chains are member-major; different members sample
 * different posteriors) -- LB is that member's. */
int magi_sampler_summarize(magi_handle* h, int chain0, int n_sel, int n_q, const double* probs, int max_lag,
                           double* X_mean, double* X_sd, double* X_quant, double* X_rhat, double* X_ess, double* X_mcse_mean,
                           double* sig_mean, double* sig_sd, double* sig_quant, double* sig_rhat, double* sig_ess, double* sig_mcse_mean,
                           double* th_mean, double* th_sd, double* th_quant, double* th_rhat, double* th_ess, double* th_mcse_mean,
                           int* n_nonfinite);

/* ---- rank-normalised convergence diagnostics -------------------------------------------------- */

/* Rank-normalised split R-hat, bulk ESS and tail ESS (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021; unit csrc/rank.hip, DESIGN.md
 * 4.4b) of K scalar columns of C chains x R draws.  draws: host [C][R][K]; the limits on C, R, C R and K are magi_summarize's.  Per column
 * y, with S = C R pooled draws, v = the sorted pooled draws, and rhat / ess the split R-hat and the ESS of magi_summarize (the same split,
 * Geyer truncation, max_lag and tau floor) applied to a derived series of the same shape:
 *   rank[s]       (the pooled draws < y[s]) + ((the pooled draws == y[s], itself included) + 1) / 2: the 1-based average rank, exact in a
 *                 double.  Equality is ==: -0.0 and +0.0 are tied.  The ranks are pooled over all S draws also when R is odd (the split then
 *                 drops the middle draw; ArviZ ranks the split draws: an O(1/S) difference for odd R).
 *   z[s]          Phi^-1((rank[s] - 3/8) / (S + 1/4)), Phi^-1 the inverse normal CDF in fp64 (a few ulp of max(1, |z|)).
 *   z_folded[s]   the same transform of f[s] = |y[s] - med|, med the quantile of magi_summarize at p = 0.5.  For an even S the two middle
 *                 draws lie equally far from med, and whether their folded values tie -- ranks (1.5, 1.5), (1, 2) or (2, 1) -- is decided
 *                 in the last place of med: a property of the definition (ArviZ's too).  Draws that differ in their last places, such as
 *                 a natural-scale transform evaluated by another library, can so move the folded leg of rhat_rank (by 8e-5 at S = 1000
 *                 in profiles/r20_exp_rank.json); for an odd S med is a draw and nothing of the kind happens.
 *   ess_bulk      ess(z).
 *   rhat_rank     max(rhat(z), rhat(z_folded)); NaN when either is NaN.
 *   ess_tail      min(ess(I_lo), ess(I_hi)), I_p[s] = 1 if y[s] <= v[floor((S - 1) p)] else 0 with p = tail_prob for I_lo and 1 - tail_prob
 *                 (formed in fp64) for I_hi: the lower order statistic stands where ArviZ interpolates the quantile.  NaN when either leg is
 *                 NaN, which it is when its indicator is a constant column.
 * All three are NaN for a constant column and when R < 4.  A series without a split R-hat has no ESS either: the constant series, and the
 * series whose split chains are all one constant while the dropped middle draw of an odd R differs (there magi_summarize's ess is that of
 * tau at its floor).  A column with a non-finite draw has NaN everywhere (rank, z, z_folded too) and
 * counts in *n_nonfinite.  rhat_rank, ess_bulk, ess_tail [K]; rank, z, z_folded [C][R][K] (for rank plots; the legs of rhat_rank are
 * magi_summarize's rhat of the z and z_folded returned here bit for bit, and so is ess_bulk its ess of z -- with one deviation from "the
 * ess of magi_summarize applied to z": where that series has no split R-hat, the rule above returns NaN and magi_summarize the ess of tau at
 * its floor); n_nonfinite: each optional (NULL: not copied).  Results are bit-identical from run to run.  MAGI_E_BADARG (handle stays usable): as magi_summarize, and a tail_prob outside
 * (0, 0.5] or not finite.  Needs a handle only for its device and stream.  Device memory of a call: the columns go in chunks of at most
 * 64 MiB; a call holds the chunk, its sorted columns, one derived series and the staging of the upload (and of the series on their way
 * down) -- four buffers of that size, three without the host's draws -- and four sets of split-chain means of at most 32 MiB: 384 MiB
 * whatever K is, plus 3 K doubles of results and the chunk-local statistics of the four series, 36 doubles per column of a chunk (a
 * chunk has min(K, 2^23 / (C R), 2^21) columns: 0.1 MB at the sampler's shapes, 576 MiB where K >= 2^21 columns have four draws each). */
int magi_rank_diagnostics(magi_handle* h, int C, int R, int K, const double* draws, int max_lag, double tail_prob,
                          double* rhat_rank, double* ess_bulk, double* ess_tail,
                          double* rank, double* z, double* z_folded, int* n_nonfinite);

/* The same three diagnostics of the sampler's device-resident post-burn-in samples, pooled over the chains [chain0, chain0 + n_sel): the
 * blocks, layouts and natural-scale transforms of magi_sampler_summarize (X [N][D], sigma_sqs [D], thetas [P]; a group member's own bounds,
 * supports and fixed variances); *n_nonfinite counts the columns of all three.  Every output is optional.  MAGI_E_STATE / MAGI_E_BADARG as
 * magi_sampler_summarize (sampler initialised, every selected chain finished, the chain range inside the sampler's chains and inside one
 * member of a group), then tail_prob as magi_rank_diagnostics.  Changes nothing of the handle's state. */
int magi_sampler_rank_diagnostics(magi_handle* h, int chain0, int n_sel, int max_lag, double tail_prob,
                                  double* X_rhat_rank, double* X_ess_bulk, double* X_ess_tail,
                                  double* sig_rhat_rank, double* sig_ess_bulk, double* sig_ess_tail,
                                  double* th_rhat_rank, double* th_ess_bulk, double* th_ess_tail,
                                  int* n_nonfinite);

/* ---- pointwise log-likelihood, WAIC and PSIS-LOO ----------------------------------------------- */

/* Which of two models of the same data predicts them better (unit csrc/elpd.hip).  Per column k of a log-likelihood
 * array loglik, host [C][R][K] -- l_s, s = c R + r, the log density of observation k under draw s -- with S = C R pooled draws:
 *   lpd           logsumexp_s l_s - log S: the log pointwise predictive density.
 *   p_waic        var_s l_s (ddof = 1, two passes; NaN when S < 2).
 *   elpd_waic     lpd - p_waic.
 *   khat, elpd_loo, p_loo   Pareto-smoothed importance sampling (Vehtari, Gelman, Gabry 2017, r_eff = 1).  Log ratios r_s = -l_s - max_s(-l_s)
 *                 (a -0.0 counts as +0.0).  Tail length M = min(floor(S / 5), ceil(3 sqrt(S))).  The draws are ordered ascending by (r, s);
 *                 the tail is the last M of them and the cutoff c is the r of the draw just below it.  If M < 5 or the tail's largest and
 *                 smallest r are equal there is no smoothing and khat = +inf.  Otherwise x_j = exp(r_tail,j) - exp(c), ascending, and the
 *                 fit is Zhang and Stephens': m = 30 + floor(sqrt(M)); theta_j = 1 / x_M + (1 - sqrt(m / (j - 1/2))) / (3 x_[floor(M/4 + 1/2)]),
 *                 j = 1 .. m; k_j = mean_i log1p(-theta_j x_i); l_j = M (log(-theta_j / k_j) - k_j - 1); w_j = 1 / sum_i exp(l_i - l_j);
 *                 theta = sum_j theta_j w_j; k = mean_i log1p(-theta x_i); sigma = -k / theta; khat = (k M + 5) / (M + 10).  If khat is
 *                 finite the tail draw of rank j (1-based) gets the log weight log(exp(c) + sigma / khat expm1(-khat log1p(-(j - 1/2) / M)))
 *                 (khat = 0: log(exp(c) - sigma log1p(-(j - 1/2) / M))); every other draw keeps lw_s = r_s.  All log weights are capped at 0.
 *                 elpd_loo = logsumexp_s(l_s + lw_s) - logsumexp_s(lw_s);  p_loo = lpd - elpd_loo.
 * A column with a non-finite l has NaN in every output and counts in *n_nonfinite.  Every sum runs in one fixed order: the results are
 * bit-identical from run to run and do not depend on the chunking (summary_chunk_cols).
 * lpd, p_waic, elpd_waic, elpd_loo, p_loo, khat [K], n_nonfinite: each optional (NULL: not copied).
 * MAGI_E_BADARG (handle stays usable): C, R, C R as magi_summarize; K outside [1, 2^24]; loglik NULL; elpd_loo, p_loo or khat asked
 * for with C R > 466033 -- the tail is sorted in LDS, 2048 (key, index) pairs, and M = ceil(3 sqrt(C R)) must fit; lpd, p_waic and
 * elpd_waic are served for every C R when the three are NULL.  Needs a handle only for its device and stream, as magi_summarize; device
 * memory of a call: the 64 MiB chunk, its staging buffer and 6 K doubles + K ints of results. */
int magi_elpd(magi_handle* h, int C, int R, int K, const double* loglik,
              double* lpd, double* p_waic, double* elpd_waic, double* elpd_loo, double* p_loo, double* khat,
              int* n_nonfinite);

/* The same six outputs for the observations of the finished sampler run, from its device-resident samples pooled over the chains
 * [chain0, chain0 + n_sel): no draw crosses to the host.  One column per observed entry e = d N + i (yobs[e] not NaN), in ascending e;
 * obs_index [n_obs] returns e, *n_obs_out their number n_obs (<= N D: arrays of N D entries always suffice, and a call with every other
 * output NULL returns the number alone).  The log-likelihood of entry e under draw s, with x = X_s[e] and sigma^2_d(s) =
 * softplus(sig_pre_d) + LB[d], or the constant of a MAGI_PRIOR_FIXED entry (the sigma^2 block of magi_sampler_summarize), is the
 * untempered observation density of magi_set_obs_model:
 *   l = -1/2 [ log(2 pi sigma^2_d / w_e) + w_e (g_d(x) - g_d(y_e))^2 / sigma^2_d ]
 * with the link g_d and the weight w_e of the handle's -- on a group handle the member's own -- observation model (identity and 1
 * without one).  A state outside a link's domain at an observed point gives a non-finite l, hence a NaN column.  The density is on the
 * LINK's scale: to compare models with different links add log|g_d'(y_e)| per observation (MAGI_v2.posterior_elpd(scale="data")).
 * loglik_out, optional: host [n_sel num_results][n_obs], the l themselves.  Every output is optional.
 * MAGI_E_STATE / MAGI_E_BADARG as magi_sampler_summarize (sampler initialised, every selected chain finished, the chain range inside
 * the sampler's chains and inside one member of a group), and the C R bound of elpd_loo, p_loo, khat above. */
int magi_sampler_elpd(magi_handle* h, int chain0, int n_sel,
                      double* lpd, double* p_waic, double* elpd_waic, double* elpd_loo, double* p_loo, double* khat,
                      int* obs_index, int* n_obs_out, double* loglik_out, int* n_nonfinite);

/* ---- posterior trajectories at any time: GP conditioning ---------------------------------------- */

/* Matern cross blocks (unit csrc/build.hip: k_matern_cross, the rectangular sibling of the kernel behind magi_matern_blocks).  Row times
 * t_new[T] against column times I[N]: Ks[m][j] = k(t_new[m], I[j]) and pKs[m][j] = d k / d t* at (t_new[m], I[j]), the derivative in the
 * FIRST argument (the sign convention of p_Kappa).  Same Bessel routine, recurrences and exponent forms as magi_matern_blocks, entry by
 * entry: with t_new = I the two outputs equal its Kappa and p_Kappa bit for bit.  The coincident-time values (phi1, 0) are taken where
 * t_new[m] == I[j] EXACTLY, not by index.  Ks, pKs: host [T][N], either may be NULL.  Needs a handle only for its device and stream.
 * MAGI_E_BADARG (handle stays usable): T outside [1, 2^16], N outside [1, 2^20], T N > 2^28, t_new or I NULL or not finite, phi1, phi2
 * not positive, nu <= 1. */
int magi_matern_cross(magi_handle* h, const double* t_new, int T, const double* I, int N,
                      double phi1, double phi2, double nu, double* Ks, double* pKs);

/* The draws of the trajectory at times t_new that need not be grid points (unit csrc/gp.hip).  Under MAGI's model, given a
 * draw's x_d(I), x_d(t*) is Gaussian.  Per component d, with C^-1_d the handle's resident dense stack AS STORED, UNTRANSPOSED and not
 * symmetrised (an uploaded matrix need not be symmetric), Ks_d and pKs_d the cross blocks of magi_matern_cross with (phi1[d], phi2[d], nu):
 *   W_d = Ks_d C^-1_d,  Wd_d = pKs_d C^-1_d         [T][N]: rows of Ks times columns of C^-1, W_d[m][k] = sum_j Ks_d[m][j] C^-1_d[j][k]
 *   x_new[s][m][d]  = mu_d + sum_k W_d[m][k] (X_s[k][d] - mu_d)        the conditional mean of x_d(t_new[m]) given draw s
 *   dx_new[s][m][d] =        sum_k Wd_d[m][k] (X_s[k][d] - mu_d)       the conditional mean of its derivative (at a grid time: m_d (x_d - mu_d))
 *   cond_var[m][d]  = max(0, phi1_d - sum_k W_d[m][k] Ks_d[m][k])      the conditional variance, the same for every draw
 *   dcond_var[m][d] = max(0, nu phi1_d / (phi2_d^2 (nu - 1)) - sum_k Wd_d[m][k] pKs_d[m][k])
 * The variances are clamped at 0: in floating point the difference reaches about -1e-11 at grid times, where it is 0.
 * Arithmetic: x_new = g + mu_d (1 - r) and dx_new = gd - mu_d rd, with g = sum_k W_d[m][k] X_s[k][d] and gd its twin accumulated by the fp64
 * matrix-core GEMM, k ascending, and r = sum_k W_d[m][k], rd = sum_k Wd_d[m][k] summed in one fixed order from the same W, Wd: mu is never
 * subtracted from a draw.  Results are bit-identical from run to run and do not depend on the chunking (gp_chunk_rows).
 * x_new and dx_new are CONDITIONAL MEANS: a draw of x(t*) itself is x_new + sqrt(cond_var) z with z ~ N(0, 1) per (s, m, d), and the
 * predictive sd of x(t*) is sqrt(x_sd^2 + cond_var) with x_sd the sd of x_new over the draws.  Outside [min I, max I] the mean reverts to mu
 * and the variance to phi1.  t_new need not be sorted or distinct and may coincide with grid times; I need not be sorted.
 * X: host [S][N][D].  x_new, dx_new: host [S][T][D]; cond_var, dcond_var: host [T][D]; every output is optional.
 * MAGI_E_STATE without resident dense matrices of this N, D (magi_build_matrices, magi_build_dense, magi_set_matrices).  MAGI_E_BADARG
 * (handle stays usable): T outside [1, 2^16], S outside [1, 2^20], x_new or dx_new asked for with S T D > 2^28, N < 2, D outside
 * [1, MAGI_MAX_D], a NULL input, a non-finite t_new, I or mu, phi1 or phi2 not positive, nu <= 1.  Device memory of a call: the rows of
 * t_new go in chunks so that none of the buffers (cross blocks, weights, the two chunks of draws, their staging) exceeds 64 MiB unless a
 * single row needs more; the draws X themselves are uploaded whole. */
int magi_gp_predict(magi_handle* h, const double* I, int N, int D, const double* phi1, const double* phi2, double nu,
                    const double* mu, int T, const double* t_new, int S, const double* X,
                    double* x_new, double* dx_new, double* cond_var, double* dcond_var);

/* The same for the finished sampler run, from its device-resident samples of the chains [chain0, chain0 + n_sel) read in place (no draw
 * is copied, transposed or downloaded), with mu the problem's and N, D the problem's; I, phi1, phi2, nu are the caller's: the grid and the
 * hyper-parameters the resident matrices were built with (an uploaded C^-1 is used as it is).  x_new, dx_new: host
 * [n_sel num_results][T][D] -- bit for bit what magi_gp_predict returns for the downloaded samples.  The twelve summaries, [T][D] and
 * quant [n_q][T][D], are the statistics of magi_summarize over x_new and over dx_new as [n_sel][num_results][T D] draws, bit for bit, computed
 * on the device; *n_nonfinite counts the columns of x_new with a non-finite draw, and those of dx_new when a dx statistic is asked for.
 * Every output is optional.  MAGI_E_STATE / MAGI_E_BADARG as magi_sampler_summarize (sampler initialised, every selected chain finished,
 * the chain range inside the sampler's chains and inside one member of a group: the matrices and mu are that member's) and as
 * magi_gp_predict (S = n_sel num_results); MAGI_E_STATE also when the resident dense matrices are not the problem's N, D. */
int magi_sampler_gp_predict(magi_handle* h, int chain0, int n_sel, const double* I, const double* phi1, const double* phi2, double nu,
                            int T, const double* t_new, int n_q, const double* probs, int max_lag,
                            double* x_new, double* dx_new, double* cond_var, double* dcond_var,
                            double* x_mean, double* x_sd, double* x_quant, double* x_rhat, double* x_ess, double* x_mcse_mean,
                            double* dx_mean, double* dx_sd, double* dx_quant, double* dx_rhat, double* dx_ess, double* dx_mcse_mean,
                            int* n_nonfinite);

/* Diagnostics: device time (ms, HIP events) of the stages of the last magi_gp_predict / magi_sampler_gp_predict made while the switch
 * gp_profile was set -- cross blocks; weights and variances; the application GEMM; its mu epilogue; statistics -- zeros otherwise (the
 * transposes and downloads of x_new / dx_new are not among them).  ms: 5 entries. */
int magi_gp_profile(magi_handle* h, double* ms);

/* ---- posterior predictive checks ---------------------------------------------------------------- */

/* Could the model have produced the data (unit csrc/ppc.hip): replicated observations y_rep, their per-column
 * statistics, the PIT of every observation and the posterior predictive p-values of four realised discrepancies.
 * Draw s = c R + r (chain c, result r) of S = C R pooled draws; column k belongs to component d = comp[k]; g_d is the component's link
 * (MAGI_LINK_*), w_k > 0 the column's weight (1 without one), sigma^2_d(s) the draw's variance on the link's scale, y_k the observation
 * (NaN: none -- the column is a pure prediction).
 * Noise.  One Philox4x32-10 block per (s, k): (x, y, z, w) = philox4x32_10(k, r, chain_id[c], STREAM_PPC = 5, seed), a stream of its own
 * beside the sampler's five; u1 = u01_53(x, y), u2 = u01_53(z, w), rad = sqrt(-2 log u1), ang = 2 pi u2, z0 = rad cos(ang), z1 = rad sin(ang).
 * k is the column's index in the call; chain_id[c] is the chain's Philox id (magi_sampler_init's chain_ids) on the sampler route and the
 * caller's chain_ids[c] (c when NULL) on the host route: a result does not depend on how chains are selected or sharded.
 * Replicate.
 *   x_lat  = x[s][k] + sqrt(extra_var[k]) z1           (x[s][k] itself when extra_var is NULL)
 *   gy_rep = g_d(x_lat) + sqrt(sigma^2_d(s) / w_k) z0
 *   y_rep  = g_d^-1(gy_rep) on the data's scale: gy_rep (identity), exp(gy_rep) (log), max(gy_rep, 0)^2 (sqrt: a negative root has no
 *            datum; the map stays monotone, so quantiles commute with it).
 * The link is evaluated as the observation model evaluates it; where g_d(x_lat) is not finite (x_lat <= 0 under log, < 0 under sqrt)
 * y_rep[s][k] is NaN.
 * Per column.  mean, sd, quant [n_q][K] of y_rep over the S draws: bit for bit what magi_summarize gives for the same matrix.
 *   pit[k] = 1/S sum_s 1/2 erfc(-u_obs[s][k] / sqrt 2),   u_obs[s][k] = (g_d(y_k) - g_d(x_lat)) sqrt(w_k / sigma^2_d(s)):
 * the PIT with the observation noise integrated analytically; NaN where y_k is NaN and where any term is not finite.
 * Per draw and component: realised discrepancies of u_1 .. u_n, the values over the columns of component d with a y that is not NaN, in
 * ascending column order, once for u = u_obs[s][.] (T_obs) and once for u = z0[s][.] (T_rep: the replicate's standardised residual IS
 * z0, used directly and not recovered through g^-1):
 *   T[0] = sum u^2 (chi2)   T[1] = sum u / n (mean)   T[2] = max |u| (maxabs)   T[3] = sum_{j<n} u_j u_{j+1} / sum u_j^2 (acf1; NaN for n < 2)
 *   pval[d][t] = #{s: T_rep >= T_obs} / #{s: both finite};  n_T_excluded[d] = #{s: a T of (s, d) is not finite though defined} -- T[3] of
 *   a component with n < 2 is undefined for every draw and excludes none.  A component without such a column has NaN p-values and NaN T.
 * Every floating-point sum runs in one fixed order (columns ascending for T, one workgroup's fixed reduction for pit) and there are no
 * floating-point atomics: the results are bit-identical from run to run and do not depend on the chunking (summary_chunk_cols).
 * x: host [C R][K]; comp [K]; sigma_sq [C R][D]; link [D] or NULL (identity); weight, y, extra_var [K] or NULL; chain_ids [C] or NULL.
 * y_rep [C R][K]; mean, sd, pit [K]; quant [n_q][K]; T_obs, T_rep [C R][D][4]; pval [D][4]; n_T_excluded [D]; *n_nonfinite counts the
 * columns of y_rep with a non-finite draw (their mean, sd and quantiles are NaN).  Every output is optional.
 * MAGI_E_BADARG (handle stays usable): C, R, C R as magi_summarize; K outside [1, 2^24]; D outside [1, MAGI_MAX_D (4; 8 in a library built
 * for a wider traced drift)]; a comp outside [0, D); a link that is none of MAGI_LINK_*; a weight or sigma_sq not positive and finite; a
 * negative or non-finite extra_var; a y outside its link's domain; n_q / probs as magi_summarize; a NULL x, comp or sigma_sq.  Needs a
 * handle only for its device and stream, as magi_summarize.  Device memory of a call: three chunks [columns][C R] of together at most 64
 * MiB (3 C R doubles where a single column of the three exceeds that: up to 96 MiB at C R = 2^22), the staging of the strided upload, 18 C R D doubles of discrepancy accumulators and statistics, and the results. */
int magi_ppc(magi_handle* h, int C, int R, int K, int D, const double* x, const int* comp, const double* sigma_sq, const int* link,
             const double* weight, const double* y, const double* extra_var, uint64_t seed, const int64_t* chain_ids,
             int n_q, const double* probs,
             double* y_rep, double* mean, double* sd, double* quant, double* pit,
             double* T_obs, double* T_rep, double* pval, int* n_T_excluded, int* n_nonfinite);

/* The same for the observations of the finished sampler run, from its device-resident samples of the chains [chain0, chain0 + n_sel) read
 * in place: no draw crosses to the host.  One column per observed entry e = d N + i in ascending e -- obs_index, *n_obs_out and the call
 * that returns only the count exactly as magi_sampler_elpd -- with x = X_s[e], sigma^2_d(s) = softplus(sig_pre_d) + LB[d] or the constant
 * of a MAGI_PRIOR_FIXED entry, and the links and weights of the handle's -- on a group handle the member's own -- observation model; no
 * extra_var.  Bit for bit what magi_ppc returns for the downloaded draws with these sigma^2, which sigma_sq_out, optional, host
 * [n_sel num_results][D], returns as the kernel formed them (asked for alone, nothing else is computed).  y_rep: host [n_sel num_results][n_obs]; the other outputs as magi_ppc with K =
 * n_obs.  MAGI_E_STATE / MAGI_E_BADARG as magi_sampler_summarize (sampler initialised, every selected chain finished, the chain range
 * inside the sampler's chains and inside one member of a group), n_q / probs as magi_summarize.  Changes nothing of the handle's state. */
int magi_sampler_ppc(magi_handle* h, int chain0, int n_sel, uint64_t seed, int n_q, const double* probs,
                     double* y_rep, double* mean, double* sd, double* quant, double* pit,
                     double* T_obs, double* T_rep, double* pval, int* n_T_excluded, int* n_nonfinite,
                     int* obs_index, int* n_obs_out, double* sigma_sq_out);

/* ---- multi-GPU ---------------------------------------------------------------------------------
 * There is deliberately NO magi_gather in this ABI (SURVEY 8b had listed one).  The path shards by independent (dataset, chain) units with
 * no exchange while sampling (one handle per GPU, one process per GPU); its only collective is ONE gather of the post-burn-in samples at
 * the end of a job, and that one lives where the job's process group already lives: magi_v2_amd/shard.py calls torch.distributed.gather
 * (backend "nccl" = RCCL over xGMI) on the arrays magi_sampler_get_samples returned.  A C-side gather would have to bootstrap a second
 * RCCL communicator (ncclGetUniqueId handed through the caller, ncclCommInitRank per handle) beside the one the host framework owns, for
 * 52 MB per GPU once per job (< 1 ms over xGMI).  A binding in another host language gathers the same host arrays with its own collective. */

/* ---- instrumentation (bench.py roofline leg) ----------------------------------------------- */

/* Launch one gradient evaluation (the 3 mat-vec phases + reduce) `reps` times on the handle's
 * stream, bracketed by HIP events on that stream; phase_ms[8] receives the average device
 * time per launch of phase 1, 2, 3, the reduce kernel, the sampler's streaming kernel (single-phase
 * block mat-vecs, k_stream), its reduce (k_leap_finalize), its point kernel (k_point) and, in [7], a
 * load-only pass over the same packed operator blocks with the same access pattern (the ceiling the
 * memory system offers k_stream for this layout and working set), measured in separate event-bracketed loops.  Uses the states currently on the
 * device (n_chains as last set). */
int magi_time_gradient(magi_handle* h, int n_chains, int reps, double* total_ms_per_eval, double* phase_ms);

/* Of the last magi_sampler_run: leapfrog slots (kernel pairs [k_stream, k_point]) issued before every chain had finished --
 * counted on the device -- and graph launches (of 128 slots each; MAGI_GRAPH_SLOTS) the host made.  A slot advances every unfinished chain by one
 * leaf or one set-up step, so slots_issued >= the leapfrogs of the busiest chain. */
int magi_sampler_run_stats(magi_handle* h, int64_t* slots_issued, int64_t* graphs_launched);

/* In-sampler kernel durations: continues the chains for n_slots leapfrog slots launched one by one (no graph) with HIP events
 * attached to every launch (hipExtLaunchKernel start / stop events = the kernel's own begin / end time stamps, the quantity
 * rocprofv3 --kernel-trace reports), decisions riding along as in production.  stream_us / point_us = mean device time per
 * launch of the streaming kernel and of k_point; leapfrogs_done = gradient evaluations taken (sum over chains).  The chains are
 * left inside a transition: the sampler must be re-initialised afterwards (MAGI_E_STATE otherwise). */
int magi_sampler_profile(magi_handle* h, int n_slots, double* stream_us, double* point_us, int64_t* leapfrogs_done);

/* phase_bytes[8]: bytes each of those seven kernels must move per launch for the current matrices
 * and n_chains, for the kernel family that serves a batch of n_chains (magi_stream_kernel_name):
 * [4] = the streaming kernel: packed operator blocks + what it stores (+ for k_stream_sep its operand planes, once per XCD);
 * [6] = k_point; [7] = the algorithmic bytes of one gradient evaluation as SURVEY 8d counts them (3 D N W 8 + C 10 N D 8). */
int magi_gradient_bytes(magi_handle* h, int n_chains, double* phase_bytes);

/* Storage formats of the packed operator blocks (option "tile_demote"): n_blocks = the 128 x 128 blocks of the current
 * matrices, n_demoted = those of them the packing certified and stores a second time as fp32 -- an off-diagonal block whose row and
 * column abs-sums are at most 2^-29 of the abs-sums of the same rows / columns of the diagonal blocks that feed the same outputs, so
 * that its fp32 rounding (2^-24) moves an output by no more than the fp64 rounding of the diagonal block's own product.  The VALU
 * streaming kernels read a demoted block's fp32 copy; its fp64 entries hold the same (rounded) values, so every kernel family
 * multiplies one operator.  No block is skipped and all arithmetic is fp64.  block_bytes = the operator bytes one launch of the
 * streaming kernel that serves n_chains reads (the first term of magi_gradient_bytes' [4]).  Any pointer may be null. */
int magi_tile_formats(magi_handle* h, int n_chains, int64_t* n_blocks, int64_t* n_demoted, double* block_bytes);

/* Carrier workgroups of the VALU streaming kernels (option "stream_carriers"): the packing weighs a block 2 units of
 * 64 KB when a VALU kernel reads it as fp64 and 1 when it reads the fp32 copy, and fills carriers of up to three blocks to 3 units -- [fp64 +
 * fp32] or [fp32 x 3], what does not fill one in the last carriers.  Where the launch is in carriers, k_stream<1 | 2> run one 768-thread
 * workgroup per carrier, at most one per CU, each block on four waves of its own with the arithmetic and the partial slots of the 256-thread
 * launch: results are bit-identical and no checkpoint depends on it.  on = whether the current pack launches carriers (the option's resolved
 * value: off by default; -1 = where one workgroup per block needs more than one round on this device and the carriers fit in one); n_carriers and units[0 ..
 * n_carriers) = the carriers of the current pack and their units, filled whether they are launched or not (cap = the room in units).  Any
 * pointer may be null.  The group and matrix-core kernels always run a workgroup per block. */
int magi_stream_carriers(magi_handle* h, int* on, int* n_carriers, int* units, int cap);
/* The carrier table itself: tasks[3 c + s] = the block (its index among magi_tile_formats' n_blocks) in slot s of carrier c, -1 = empty. */
int magi_stream_carrier_tasks(magi_handle* h, int* tasks, int cap);

/* Name of the streaming kernel a batch of n_chains runs on with the current matrices, problem and options:
 * "k_stream<1>", "k_stream<2>" (VALU), "k_stream_sep<CW=8|16>" (matrix cores, separable drift), "k_stream_mc". */
int magi_stream_kernel_name(magi_handle* h, int n_chains, char* buf, int cap);

/* Tuning / test switches of a handle (csrc/magi_internal.h: MagiOptions; one table in csrc/capi.hip).  The environment variables
 * are read ONCE, by magi_create; afterwards only this call changes an option (no getenv on a compute path).  A variable outside an
 * option's range keeps the default, as this call rejects such a value (MAGI_E_BADARG).  A flag is on for a non-zero value; its
 * variable turns it on by being present, whatever its value.  Options, with their variables:
 *   "stream_family"       MAGI_STREAM_FAMILY        0 auto, 1 mc, 2 valu (variable: "mc" / "valu"); takes effect at the next
 *                                                   magi_sampler_init / log-posterior call
 *   "family_chains"       MAGI_FAMILY_CHAINS        0..4096; > 0: "auto" chooses the kernel family as if the batch had this many
 *                                                   chains -- a sharded job passes its largest per-GPU share on every rank, so that a
 *                                                   chain's samples do not depend on how many chains share its GPU
 *   "sep_pair_min"        MAGI_SEP_PAIR_MIN         clamped to 0..2^30; read at the next packing
 *   "fused_parity"        MAGI_FUSED_PARITY         1: magi_logpost_grad_fused evaluates as an odd leapfrog slot
 *   "gemm_remap_min"     MAGI_GEMM_REMAP_MIN       clamped to 0..2^30
 *   "potrf_panels"        MAGI_POTRF_PANELS         1..16
 *   "potrf_lookahead_min" MAGI_POTRF_LOOKAHEAD_MIN  >= 0
 *   "no_graph"            MAGI_NO_GRAPH             flag
 *   "fit_host_loop"       MAGI_FIT_HOST_LOOP        flag
 *   "build_profile"       MAGI_BUILD_PROFILE        flag
 *   "build_serial"        MAGI_BUILD_SERIAL         flag
 *   "slot_budget_graphs"  (none: a test hook)       cap on the graph launches of one magi_sampler_run; 0 = the computed bound
 * Beside the options, one test switch of the summaries (no environment variable, no effect on any result): summary_chunk_cols, 0..2^24;
 * > 0: magi_summarize / magi_sampler_summarize and magi_elpd / magi_sampler_elpd gather at most this many columns per chunk (0 = what the
 * work space allows).  Likewise the two of the GP conditioning: gp_chunk_rows, 0..2^16; > 0: magi_gp_predict / magi_sampler_gp_predict work on
 * at most this many rows of t_new per chunk (no effect on any result); gp_profile, a flag: they time their stages (magi_gp_profile; a
 * synchronisation per stage).  And the storage switch of the packing, tile_demote, 0 or 1 (default 1; the variable MAGI_TILE_DEMOTE = 0 or 1 is
 * read by magi_create): 1: the packing stores the operator blocks it can certify a second time as fp32 for the VALU streaming kernels
 * (magi_tile_formats); 0: every block fp64, as before the format existed; read at the next packing.  And the launch shape of the VALU streaming
 * kernels, stream_carriers, -1, 0 or 1 (default 0; the variable MAGI_STREAM_CARRIERS is read by magi_create): 0: a workgroup per block; -1: carrier
 * workgroups (magi_stream_carriers) where they turn a launch of several rounds into one (measured SLOWER than the default at N = 1024 on an
 * MI355X: profiles/r22_carriers_ab.txt); 1: wherever a CU holds exactly one carrier workgroup
 * (tests at small shapes); read at the next packing; no result depends on it. */
int magi_set_option(magi_handle* h, const char* name, int64_t value);

/* Diagnostics: per-class device time of the last magi_build_matrices run with option "build_profile" set
 * (HIP events around every launch; the build is serialised while profiling).
 * Classes, in order: matern, diag-block Cholesky+inverse, potrf panel, potrf trailing SYRK, trtri,
 * T^T T, m / K products, single-phase operators.  flops = fp64 operations actually issued.  One more row follows the
 * classes and is filled by EVERY dense build of the handle, profiled or not: "potrf_wall" = the two blocked Cholesky
 * factorisations as a whole on the device clock (ms; flops = N^3 / 3 per matrix) -- the only figure that shows the
 * look-ahead of the factorisation (option "potrf_lookahead_min": grids from that size on fork their rank-k updates
 * to a second, CU-masked stream; 0 = never), which the serialising per-launch profile switches off.  Returns the
 * number of rows (9); arrays must hold at least 16 entries. */
int magi_build_profile(magi_handle* h, double* flops, double* ms, int64_t* calls);

/* Diagnostics: the 64-double transformed-parameter block of a chain (softplus / sigmoid / log
 * terms of the state in flight; in a -DMAGI_STAMPS=<kernel> dev build entries 40.. hold timing stamps, csrc/stamps.h). */
int magi_debug_par(magi_handle* h, int chain, double* out64);

#ifdef __cplusplus
}
#endif
#endif /* MAGI_HIP_H */
