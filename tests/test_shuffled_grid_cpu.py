"""The shuffled-grid fixture (tests/util.py: shuffled_grid) held to its conditions on the oracle alone: no GPU.

tests/test_shuffled_grid_gpu.py and the shuffled cases of tests/test_fullsize_gpu.py / tests/test_fit_gpu.py are worth what is asserted here.
The device's sequence of the matrix build is emulated in fp64 numpy:
    Kappa -> Cholesky -> T = L^-1 (lower) -> C^-1 = T^T T;   Wt = -T p_Kappa, m = Wt^T T;   K = Kappa_pp - Wt^T Wt (lower part mirrored)
    -> second Cholesky -> T2 -> K^-1 = T2^T T2
with the Matern blocks from the cancellation-free columns (orc.matern_block_columns_accurate).  The literal formulas (orc.matern_blocks) are
NOT used: their Kappa_pp loses digits at small lags, and the K^-1 K_ref = I residual of this emulation then sits 5 to 300 times above its bar,
sorted and shuffled alike -- a loss of the reference's formula, not of the build.

The residuals and their bars are those of tests/test_build_gpu.py::test_build_multi_block_inverse_property:
    |C^-1 Kappa - I| < 50 cond eps,    relmax(m, p_Kappa Kappa^-1) < 50 cond eps,    |K^-1 K_ref - I| < 200 cond eps sqrt(cond_K).
"The perturbation": one lower 128 x 128 block of T (or of T2) set to zero before the products -- what a trtri level that never ran, a
remainder pass with a wrong row count, a triangular k range one block short or a rank-k update that dropped a tile leave behind."""
import numpy as np
import pytest
from scipy.linalg import solve_triangular

from magi_v2_amd import host
from oracle import magi_oracle as orc
from tests.util import shuffled_grid

EPS = np.finfo(float).eps
NB = 128
PHIS = [(0.03, 0.3), (0.2, 0.15)]            # (phi1, phi2) of the two components the GPU builds use
N_EMU, SEED = 513, 11
FIT_N, FIT_SEED = 300, 5                     # the fit tests of tests/test_fit_gpu.py: their size and the seed of their permutation
FIT_LOSS_RTOL = 1e-8                         # ... and their bar on the loss trace


def lower_blocks(N):
    nb = (N + NB - 1) // NB
    return [(bi, bj) for bi in range(nb) for bj in range(bi + 1)]


def zero_block(T, blk):
    T = T.copy()
    T[blk[0] * NB:(blk[0] + 1) * NB, blk[1] * NB:(blk[1] + 1) * NB] = 0.0
    return T


def relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


class Emulation:
    """The build of one component on grid I, its truth and its bars; residuals as fractions of their bars."""

    def __init__(self, I, phi1, phi2):
        N = len(I)
        self.N = N
        self.Kap, self.pK, self.Kpp = orc.matern_block_columns_accurate(I, np.arange(N), phi1, phi2)
        self.T = solve_triangular(np.linalg.cholesky(self.Kap), np.eye(N), lower=True)
        self.cond = np.linalg.cond(self.Kap)
        self.m_ref = np.linalg.solve(self.Kap, self.pK.T).T
        K_ref = self.Kpp - self.m_ref @ (-self.pK)
        self.K_ref = 0.5 * (K_ref + K_ref.T)
        self.condK = np.linalg.cond(self.K_ref)
        self.bar_C = self.bar_m = 50 * self.cond * EPS
        self.bar_K = 200 * self.cond * EPS * self.condK ** 0.5
        self.T2 = self.second_factor(self.T)

    def second_factor(self, T):
        Wt = -T @ self.pK
        K = np.tril(self.Kpp - Wt.T @ Wt)
        K = K + np.tril(K, -1).T
        return solve_triangular(np.linalg.cholesky(K), np.eye(self.N), lower=True)

    def res_C(self, T):
        return np.abs(T.T @ T @ self.Kap - np.eye(self.N)).max() / self.bar_C

    def res_m(self, T):
        return relmax((-T @ self.pK).T @ T, self.m_ref) / self.bar_m

    def res_K(self, T2):
        return np.abs(T2.T @ T2 @ self.K_ref - np.eye(self.N)).max() / self.bar_K


_emu = {}


def emulation(N, order, d):
    """Computed once per session and shared: treat it as read-only."""
    key = (N, order, d)
    if key not in _emu:
        I, perm = shuffled_grid(N, SEED)
        _emu[key] = Emulation(I[perm] if order == "shuffled" else I, *PHIS[d])
    return _emu[key]


@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("N", [300, N_EMU, 700])
def test_a_reference_has_100x_of_room_on_the_shuffled_grid(N, d):
    """(a) The emulated build stays within 1 / 100 of each bar on the shuffled grid: a GPU build that misses a bar there is wrong, not
    unlucky.  Measured at these sizes and seed: at most 7.6e-3, 2.0e-3 and 2.9e-4 of the bars."""
    e = emulation(N, "shuffled", d)
    got = (e.res_C(e.T), e.res_m(e.T), e.res_K(e.T2))
    print(f"N={N} phi={PHIS[d]} cond={e.cond:.6e} condK={e.condK:.3e} fractions of the bars: C {got[0]:.2e} m {got[1]:.2e} K {got[2]:.2e}")
    assert max(got) <= 1e-2, got


@pytest.mark.parametrize("d", [0, 1])
def test_bc_every_factor_block_counts_shuffled_and_some_do_not_sorted(d):
    """(b) Shuffled: zeroing ANY single lower 128-block of T moves the C^-1 and the m residual, and of T2 the K^-1 residual, to at least
    1000 times its bar.  (c) Sorted: the least effect over the blocks leaves every residual within its bar -- the gap the shuffled
    tests close.  Also: the shuffled matrix has the condition number of the sorted one (same eigenvalues), so the bars are the same.
    Measured, least effect over the 15 blocks as a multiple of the bar (C^-1, m, K^-1): shuffled 4.0e8, 6.7e7, 3.5e5 at phi = (0.03, 0.3) and
    7.4e9, 2.2e9, 1.2e7 at (0.2, 0.15); sorted 1.1e-2, 5.4e-4, 1.3e-4 and 5.2e-3, 1.2e-3, 1.5e-4 -- the unperturbed residuals."""
    sh, so = emulation(N_EMU, "shuffled", d), emulation(N_EMU, "sorted", d)
    assert abs(sh.cond - so.cond) <= 1e-6 * so.cond and abs(sh.condK - so.condK) <= 1e-4 * so.condK
    worst = {}
    for name, e in (("shuffled", sh), ("sorted", so)):
        rc, rm, rk = [], [], []
        for blk in lower_blocks(N_EMU):
            Tz = zero_block(e.T, blk)
            rc.append(e.res_C(Tz))
            rm.append(e.res_m(Tz))
            rk.append(e.res_K(zero_block(e.T2, blk)))
        worst[name] = (min(rc), min(rm), min(rk))
        print(f"{name} phi={PHIS[d]}: least effect of a zeroed block, as a fraction of the bar: C {min(rc):.2e} m {min(rm):.2e} K {min(rk):.2e}")
    assert min(worst["shuffled"]) >= 1000.0, worst
    assert max(worst["sorted"]) <= 1.0, worst


def test_b_far_block_is_invisible_sorted_and_catastrophic_shuffled():
    """The header of the issue as one number pair: the far blocks of T (rows 384 and beyond, columns 0 to 127) set to zero."""
    for order, check in (("sorted", lambda r0, r1: r1 == r0), ("shuffled", lambda r0, r1: r1 > 1e6 * max(r0, 1.0))):
        e = emulation(N_EMU, order, 1)
        Tz = e.T.copy()
        Tz[384:, :128] = 0.0
        r0, r1 = e.res_C(e.T), e.res_C(Tz)
        print(f"{order}: |C^-1 Kappa - I| / bar = {r0:.3e} before, {r1:.3e} after")
        assert check(r0, r1), (order, r0, r1)


def test_d_matern_blocks_commute_with_the_shuffle_bit_for_bit():
    """(d) The truth side's blocks of the shuffled grid ARE the sorted ones re-indexed, and p_Kappa is exactly antisymmetric."""
    I, perm = shuffled_grid(N_EMU, SEED)
    for phi1, phi2 in PHIS:
        so = orc.matern_block_columns_accurate(I, np.arange(N_EMU), phi1, phi2)
        sh = orc.matern_block_columns_accurate(I[perm], np.arange(N_EMU), phi1, phi2)
        for a, b in zip(sh, so):
            assert np.array_equal(a, b[np.ix_(perm, perm)])
        assert np.array_equal(sh[1], -sh[1].T)
        assert np.array_equal(sh[0], sh[0].T) and np.array_equal(sh[2], sh[2].T)


def fit_problem():
    """The rows the fit tests of tests/test_fit_gpu.py use and the hyper-parameters they start from (both from the SORTED rows)."""
    I, X_obs, _, _ = host.synthetic_seir(FIT_N, seed=0)
    X = host.linear_interpolate(X_obs)[:, :2]
    perm = shuffled_grid(FIT_N, FIT_SEED)[1]
    return I, X, perm, orc.hparams_initial(X)


def test_e_marginal_likelihood_is_invariant_under_a_shuffle():
    """(e) Everything of the fit after the priors: log N(x; mu, S) and its gradient of (I[perm], x[perm]) equal those of (I, x)."""
    I, X, perm, init = fit_problem()
    for d in range(2):
        mu = X[:, d].mean()
        args = (mu, init["phi1s"][d], init["phi2s"][d], init["sigma_sqs"][d])
        ll0, g0 = orc.gp_marginal_and_grad(I, X[:, d], *args)
        ll1, g1 = orc.gp_marginal_and_grad(I[perm], X[perm, d], *args)
        print(f"component {d}: ll {ll0!r} {ll1!r}  grad {g0} {g1}")
        assert abs(ll1 - ll0) <= 1e-12 * abs(ll0)
        np.testing.assert_allclose(g1, g0, rtol=1e-12, atol=0)


def test_f_every_block_of_the_fits_inverse_counts_on_the_shuffled_grid():
    """(f) The fit on the shuffled rows, at the hyper-parameters it starts from: zeroing any single lower 128-block of S^-1 (and its mirror)
    moves the objective of the first Adam step -- the first entry of the loss trace, D (log likelihood + log prior) summed over the
    components -- by at least 1000 times the bar the GPU test puts on that entry (rtol 1e-8).  The likelihood alone carries it for both
    components (the gradient is not needed: measured, the least relative change is 0.74, block (2, 1) of component 0); on the sorted rows the
    far block (2, 0) moves it by 1e-16, less than that bar.
    The device reads S^-1 in a = S^-1 r (k_fit_gemv; r^T a is the likelihood's quadratic form) and in the trace terms (k_fit_terms)."""
    I, X, perm, init = fit_problem()
    D = 2
    loss0 = orc_loss0(I, X)
    least = {}
    for order, p in (("shuffled", perm), ("sorted", np.arange(FIT_N))):
        effects = []
        for d in range(D):
            Kap = orc.matern_blocks(I[p].reshape(-1, 1), init["phi1s"][d], init["phi2s"][d])[0]
            Sinv = np.linalg.inv(Kap + (init["sigma_sqs"][d] + 1e-6) * np.eye(FIT_N))
            r = X[p, d] - X[:, d].mean()
            for blk in lower_blocks(FIT_N):
                Z = zero_block(Sinv, blk)
                Z = zero_block(Z.T, blk).T                                    # (the mirror; a diagonal block is zeroed once)
                d_ll = -0.5 * (r @ (Z @ r) - r @ (Sinv @ r))                  # the change of the likelihood's quadratic form
                effects.append((abs(D * d_ll) / abs(loss0), d, blk))
        least[order] = min(effects)
        print(f"{order}: least |d loss| / |loss| over components and blocks: {least[order]}  (loss {loss0:.6f})")
    assert least["shuffled"][0] >= 1000.0 * FIT_LOSS_RTOL, least
    assert least["sorted"][0] <= FIT_LOSS_RTOL and least["sorted"][2] == (2, 0), least


def orc_loss0(I, X):
    trace = []
    orc.fit_kernel_hparams(I, X, num_iters=1, trace=trace)
    return trace[0]
