"""What keeps the structureless fixture (tests/util.py: structureless_problem) honest, on the CPU oracle alone:

  * every single 128 x 128 block of every stack and component MATTERS: zeroing it moves the oracle's gradient by >= 1e-6 of its scale, 1000 x
    the loosest tolerance the GPU tests (tests/test_structureless_gpu.py) apply to it -- so a kernel that drops, transposes or misplaces
    any one block fails there;
  * the inputs cost nothing in conditioning: the fp64 oracle agrees with its own evaluation in ``longdouble`` to <= 1e-13, and so does the
    single-phase expansion the sampler's kernels evaluate -- the GPU tolerances (1e-10 / 1e-9) sit >= 1e3 x above the reference's own floor;
  * why the fixture exists: on a Matern-built problem (N = 512, 4 block rows) every block with |bi - bj| >= 2 can be zeroed and value and
    gradients move by < 1e-9 -- below the bar of the comparisons made on such matrices.

Also here: the cases the GPU tests of the same fixture run on, and the oracle's drift-table entries for the two traced drifts among them."""
import dataclasses

import numpy as np
import pytest

from oracle import magi_oracle as orc
from tests.util import structureless_problem, structureless_states, synthetic_seir_problem

TB = 128                                                  # edge of an operator block (csrc/magi_internal.h: MAGI_TB)
TRACED = ("ptrans", "seir_seasonal")                      # k_stream_mc (V x / (K + x) is not separable); a drift that uses t

# (N, drift) of the log-posterior comparisons: the block-edge sizes with SEIR-3 and SIRW (three basis functions: a second plane on grid.z),
# the production shape N = 1024 x 4 (544 tasks, paired stasks, permuted launch order), the two traced drifts at N = 513
EDGE_SIZES = (127, 128, 129, 255, 256, 257, 384, 513)
LOGPOST_CASES = [(N, d) for N in EDGE_SIZES for d in ("seir3", "sirw")] + [(1024, "seir4")] + [(513, d) for d in TRACED]
# (N, drift) of the sampler comparisons (spd=True)
SAMPLER_CASES = [(N, d) for N in (384, 513) for d in ("seir3", "sirw")]
STATE_BATCHES = (1, 2, 3, 8, 9, 16, 17)                   # states per call: k_stream<1>, <2>, Sep8, Sep16, a second chain group with a ragged tail
# band edges at N = 513 (nb = 5): diagonal; wb = 1 (far blocks skipped); 3b = 126 / 129 (wb 1 -> 2); 6b + 1 = 511 / 517 (banded against dense
# fused storage); 2b + 1 = 511 / 513 (banded against dense three-phase storage)
BANDS = (0, 20, 42, 43, 85, 86, 255, 256)
BAND_DRIFTS = ("seir3", "sirw")


def fixture_seed(N, drift, spd=False, band=None):
    """One seed per fixture (the banded ones share theirs across bands): the conditions below hold for these."""
    return 7927 * N + 31 * sorted(("seir3", "seir4", "sirw") + TRACED).index(drift) + (500000 if spd else 0) + (0 if band is None else 5)


def register_traced(drift, N):
    """The oracle's drift-table entry of a traced example on the fixture's grid (Jacobians by complex step, independent of the sympy tracing);
    returns the magi_v2_amd Drift, or None for a built-in."""
    if drift not in TRACED:
        return None
    from magi_v2_amd import drift as drift_mod
    from magi_v2_amd.drift_examples import EXAMPLES, TIME_EXAMPLES
    from tests.test_time_drift_cpu import oracle_drift_at
    f_vec, D, P = (EXAMPLES | TIME_EXAMPLES)[drift]
    orc.DRIFTS[drift] = (oracle_drift_at(f_vec, np.arange(N) * 0.025), D, P)
    return drift_mod.resolve(f_vec, D, P)


def fixture(N, drift, spd=False, band=None, salt=0):
    register_traced(drift, N)
    return structureless_problem(N, drift, fixture_seed(N, drift, spd, band) + salt, spd=spd, band=band)


def _scaled_gap(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def _longdouble(pr):
    ld = lambda a: np.asarray(a, dtype=np.longdouble)
    return dataclasses.replace(pr, mu=ld(pr.mu), C_inv=ld(pr.C_inv), m=ld(pr.m), K_inv=ld(pr.K_inv), N_ds=ld(pr.N_ds), y=ld(pr.y), LB=ld(pr.LB),
                               beta=np.longdouble(pr.beta))


def logpost_grad_longdouble(X, sp, tp, temp, pr_ld):
    """orc.logpost_grad with every input in ``longdouble`` (x87 extended: 64-bit mantissa): all sums and products of the matrix terms carry
    11 more bits.  (The drift tables store their Jacobians in fp64 arrays: one rounding per entry, no accumulation.)"""
    ld = lambda a: np.asarray(a, dtype=np.longdouble)
    return orc.logpost_grad(ld(X), ld(sp), ld(tp), np.longdouble(temp), pr_ld)


@pytest.mark.parametrize("N,drift,spd", [(N, d, False) for N, d in LOGPOST_CASES if N > 2 * TB] + [(N, d, True) for N, d in SAMPLER_CASES])
def test_every_single_block_moves_the_gradient(N, drift, spd):
    """The sensitivity CONDITION of the fixture (seeds and scales are picked so that it holds; it is not a measurement of the kernels)."""
    pr, X = fixture(N, drift, spd)
    Xb, sp, tp = structureless_states(pr, X, 1, 0)
    _, gX0, _, gt0 = orc.logpost_grad(Xb[0], sp[0], tp[0], 1.0, pr)
    nb = (N + TB - 1) // TB
    assert nb >= 3
    moves = []
    for A in (pr.C_inv, pr.m, pr.K_inv):
        for d in range(pr.D):
            for bi in range(nb):
                for bj in range(nb):
                    blk = A[d, bi * TB:(bi + 1) * TB, bj * TB:(bj + 1) * TB]
                    keep = blk.copy()
                    blk[...] = 0.0
                    _, gX, _, gt = orc.logpost_grad(Xb[0], sp[0], tp[0], 1.0, pr)
                    blk[...] = keep
                    moves.append(max(_scaled_gap(gX, gX0), _scaled_gap(gt, gt0)))
    print(f"single-block sensitivity N={N} {drift} spd={spd}: {len(moves)} blocks, min {min(moves):.3g} max {max(moves):.3g}")
    assert min(moves) >= 1e-6, min(moves)


def test_the_matrix_terms_carry_weight_in_the_value_at_every_test_state():
    """The scaling condition of the fixture: (t1 + t2) / beta >= 0.1 |t3 + t4| at every state the GPU tests evaluate (structureless_states(pr, X, n, 0)),
    so that the VALUE comparison sees the matrices (unscaled: 1e-2 of it)."""
    worst = np.inf
    cases = [(N, d, None) for N, d in LOGPOST_CASES] + [(513, d, b) for d in BAND_DRIFTS for b in BANDS]
    for N, drift, band in cases:
        pr, X = fixture(N, drift, band=band)
        for n in (STATE_BATCHES if band is None and drift not in TRACED and N in (513, 1024) else (1, 5)):
            Xb, sp, tp = structureless_states(pr, X, n, 0)
            for c in range(n):
                t1, t2, t3, t4, _, _ = orc.logpost_terms(Xb[c], sp[c], tp[c], pr)
                ratio = (t1 + t2) / pr.beta / abs(t3 + t4)
                assert ratio >= 0.1, (N, drift, band, n, c, t1, t2, t3, t4)
                worst = min(worst, ratio)
    print(f"smallest (t1 + t2) / beta / |t3 + t4| over the test states: {worst:.3g}")


@pytest.mark.parametrize("N,drift", [c for c in LOGPOST_CASES if c[1] not in TRACED])
def test_fp64_oracle_and_single_phase_expansion_sit_at_the_longdouble_floor(N, drift):
    pr, X = fixture(N, drift)
    pr_ld = _longdouble(pr)
    Xb, sp, tp = structureless_states(pr, X, 2, 1)
    worst = {"oracle": 0.0, "single-phase": 0.0}
    for c in range(2):
        got, want = orc.logpost_grad(Xb[c], sp[c], tp[c], 0.8, pr), logpost_grad_longdouble(Xb[c], sp[c], tp[c], 0.8, pr_ld)
        worst["oracle"] = max(worst["oracle"], abs(float(got[0] - want[0]) / float(want[0])), *[_scaled_gap(a, b) for a, b in zip(got[1:], want[1:])])
        # the sampler's formulation, t1 + t2 = xc^T FH xc - 2 f^T FE xc + f^T FK f  (csrc/pack.hip), in plain fp64 numpy
        Cs, Ks = 0.5 * (pr.C_inv + np.transpose(pr.C_inv, (0, 2, 1))), 0.5 * (pr.K_inv + np.transpose(pr.K_inv, (0, 2, 1)))
        FE = Ks @ pr.m
        FH = np.transpose(pr.m, (0, 2, 1)) @ FE + Cs
        xc = (Xb[c] - pr.mu).T
        f = orc.DRIFTS[drift][0](Xb[c], np.log1p(np.exp(tp[c])))[0].T
        quad = lambda a, A, b: float(np.einsum("dn,dnm,dm->", a, A, b))
        single = quad(xc, FH, xc) - 2.0 * quad(f, FE, xc) + quad(f, Ks, f)
        t1l, t2l = orc.logpost_terms(np.asarray(Xb[c], dtype=np.longdouble), np.asarray(sp[c], dtype=np.longdouble), np.asarray(tp[c], dtype=np.longdouble), pr_ld)[:2]
        worst["single-phase"] = max(worst["single-phase"], abs(float(single - (t1l + t2l)) / float(t1l + t2l)))
    print(f"longdouble floor N={N} {drift}: fp64 oracle {worst['oracle']:.3g}, single-phase expansion {worst['single-phase']:.3g}")
    assert worst["oracle"] <= 1e-13 and worst["single-phase"] <= 1e-13, worst


def test_matern_matrices_are_blind_to_every_block_beyond_the_first_neighbours():
    """The reason for the fixture: on the oracle-built SEIR-4 problem at N = 512 (4 block rows) all |bi - bj| >= 2 blocks of all three stacks
    can be zeroed and the log posterior and its gradients move by < 1e-9 of their scale.  Do not "simplify" the fixture back to such
    matrices: every comparison on them leaves the far blocks untested."""
    N = 512
    I, X_obs, truth, th = synthetic_seir_problem(N, seed=0)
    Xi = orc.linear_interpolate(X_obs)
    hp = orc.hparams_initial(Xi)
    C_inv, m, K_inv = orc.build_all(I.reshape(-1, 1), hp["phi1s"], hp["phi2s"], 2.01, None)
    N_ds = (~np.isnan(X_obs)).sum(axis=0).astype(np.float64)
    idx = np.where(~np.isnan(X_obs).flatten())[0]
    Xhat = orc.cubic_smoother(I, Xi)
    LB = orc.sigma_sqs_lower_bound(Xhat)
    pr = orc.Problem(I=I, mu=Xi.mean(axis=0), C_inv=C_inv, m=m, K_inv=K_inv, N_ds=N_ds, obs_idx=idx, y=X_obs.reshape(-1)[idx],
                     beta=float(4 * N / N_ds.sum()), LB=LB, drift="seir4", P=3)
    X0, sp, tp = orc.initial_state(Xhat, hp["sigma_sqs"], th, LB)
    X = X0 + 0.01 * np.random.default_rng(512).standard_normal(X0.shape)
    bi = np.arange(N) // TB
    near = (np.abs(bi[:, None] - bi[None, :]) <= 1)
    pr_near = dataclasses.replace(pr, C_inv=C_inv * near, m=m * near, K_inv=K_inv * near)
    full, cut = orc.logpost_grad(X, sp, tp, 0.8, pr), orc.logpost_grad(X, sp, tp, 0.8, pr_near)
    moves = {"value": abs(cut[0] - full[0]) / abs(full[0]), "dX": _scaled_gap(cut[1], full[1]), "dtheta": _scaled_gap(cut[3], full[3])}
    print("Matern N=512: zeroing all |bi-bj|>=2 blocks moves", {k: f"{v:.3g}" for k, v in moves.items()})
    assert max(moves.values()) < 1e-9, moves
    # (control: the first neighbours do matter -- the comparison above is not blind to everything)
    diag = dataclasses.replace(pr, C_inv=C_inv * (bi[:, None] == bi[None, :]), m=m * (bi[:, None] == bi[None, :]), K_inv=K_inv * (bi[:, None] == bi[None, :]))
    assert _scaled_gap(orc.logpost_grad(X, sp, tp, 0.8, diag)[1], full[1]) > 1e-3
