"""The certified fp32 block format on the GPU (csrc/pack.hip, leap_stream_body.h; option tile_demote): the pack demotes what the criterion
of tests/test_tile_demote_cpu.py demotes; a demoted block is streamed and multiplied like any other, with exactly its fp32-rounded values
in fp64 arithmetic; with the option off, and where nothing qualifies, nothing changes; a chain at a demoting shape stays within the fused
path's tolerances of the same chain on fp64 blocks."""
import functools

import numpy as np
import pytest

from oracle import magi_oracle as orc
from tests.test_structureless_cpu import fixture
from tests.test_tile_demote_cpu import TB, block_split, fused_operators, matern_seir
from tests.util import engine_for

pytestmark = pytest.mark.gpu

BLOCK_BYTES = TB * TB * 8


def _seir_engine(N, band=None, options=None):
    """(engine, initial state) of the benchmark's SEIR-4 problem at grid size N, matrices built on the GPU."""
    from magi_v2_amd import host
    from magi_v2_amd.engine import MagiEngine
    I, phi1s, phi2s, X_obs = matern_seir(N)
    Xi = host.linear_interpolate(X_obs)
    hp = host.hparams_initial(Xi)
    N_ds, beta, idx, y = host.observation_bookkeeping(X_obs, X_obs)
    Xhat = host.cubic_smoother(I, Xi)
    LB = host.sigma_sqs_lower_bound(Xhat)
    sp, tp = host.softplus_inverse_inits(hp["sigma_sqs"], np.ones(3), LB)
    eng = MagiEngine(0)
    for name, value in (options or {}).items():
        eng.set_option(name, value)
    eng.build_matrices(I, phi1s, phi2s, 2.01, bandsize=band, want_host=False)
    eng.set_problem(Xi.mean(axis=0), N_ds.astype(float), idx, y, beta, LB, "seir4")
    return eng, (Xhat, sp, tp)


def _short_run(eng, state, chains, splits=(3,), depth=4, deep=True):
    """3 NUTS transitions (1 burn-in + 2 results, trees capped at `depth`) of `chains` chains from one state: (X, sigma, theta, integers, target)."""
    rep = lambda v: np.repeat(np.asarray(v)[None], chains, axis=0)
    cfg = eng.default_cfg(num_results=2, num_burnin_steps=1, step_size=1e-3, max_tree_depth=depth, stale_cache=0)
    eng.sampler_init(cfg, *[rep(v) for v in state], seed=77, chain_ids=list(range(5, 5 + chains)))
    for n in splits:
        eng.sampler_run(n)
    X, sp, tp = eng.sampler_samples()
    d = eng.sampler_diag()
    print("leapfrogs", d.leapfrogs_taken.tolist())
    assert not deep or d.leapfrogs_taken.max() >= 7              # (trees of depth 3 and more: the run is not a row of rejected first leaves)
    return X, sp, tp, np.stack([d.leapfrogs_taken, d.tree_depth, d.is_accepted, d.has_divergence, d.reach_max_depth]), d.target_log_prob


def _assert_runs_identical(a, b, what):
    for x, y, name in zip(a, b, ("X", "sigma_pre", "theta_pre", "integer diagnostics", "target_log_prob")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {name}")


# ---- the pack agrees with the criterion ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,blocks,demoted", [(512, 144, 48), (1024, 544, 336)])
def test_pack_demotes_the_far_blocks_of_matern_operators(N, blocks, demoted):
    eng, _ = _seir_engine(N)
    try:
        nb, nd, by = eng.tile_formats(1)
        print(f"N={N}: {nb} blocks, {nd} demoted, {by / 1e6:.1f} MB per launch of {eng.stream_kernel_name(1)}")
        assert (nb, nd) == (blocks, demoted)
        assert by == (blocks - demoted) * BLOCK_BYTES + demoted * BLOCK_BYTES / 2
        for n in (1, 2):                                         # the VALU kernels read the narrow copies ...
            assert eng.stream_kernel_name(n) == f"k_stream<{n}>"
            assert eng.gradient_bytes(n)[4] == by + n * 2 * TB * 8 * blocks
        assert eng.stream_kernel_name(8).startswith("k_stream_sep")      # ... the matrix-core kernels every block's doubles
        assert eng.tile_formats(8)[2] == blocks * BLOCK_BYTES
    finally:
        eng.close()


# ---- nothing is skipped and nothing else is rounded ------------------------------------------------------------------------------

FAR_N, FAR_SCALE, BIG = 384, 2.0 ** -40, 2.0 ** 20


@functools.lru_cache(maxsize=None)
def _far_block_case():
    """Hand-made stacks at N = 384 (three block rows), SEIR-4.  C^-1 and K^-1 are symmetric: diagonal blocks G G^T / 128 + I, the first
    off-diagonal blocks 0.05 N(0, 1) / sqrt(128), block (2, 0) (and its mirror) at 2^-40 N(0, 1) / sqrt(128); m = I.  The fused operators
    are then known exactly: FK = FE = K^-1 and FH = C^-1 + K^-1 (one rounding per entry), and the far blocks -- FH, FK (2, 0) and
    FE (2, 0), (0, 2) of every component -- are the demoted ones.  Returns the problem, the same problem whose stacks reproduce the
    operators with their far blocks rounded to fp32 (K' = r32(K), C' = r32(C + K) - r32(K): a difference of two floats of like
    magnitude, exact in fp64), and the base state."""
    pr, X = fixture(FAR_N, "seir4", spd=True)
    rng = np.random.default_rng(1905)
    D = 4

    def stack():
        A = np.zeros((D, FAR_N, FAR_N))
        for d in range(D):
            for b in range(3):
                G = rng.standard_normal((TB, TB))
                A[d, b * TB:(b + 1) * TB, b * TB:(b + 1) * TB] = G @ G.T / TB + np.eye(TB)
            for b in range(2):
                O = 0.05 * rng.standard_normal((TB, TB)) / np.sqrt(TB)
                A[d, (b + 1) * TB:(b + 2) * TB, b * TB:(b + 1) * TB] = O
                A[d, b * TB:(b + 1) * TB, (b + 1) * TB:(b + 2) * TB] = O.T
            F = FAR_SCALE * rng.standard_normal((TB, TB)) / np.sqrt(TB)
            A[d, 2 * TB:, :TB] = F
            A[d, :TB, 2 * TB:] = F.T
        return A

    import dataclasses
    C, K = stack(), stack()
    m = np.broadcast_to(np.eye(FAR_N), (D, FAR_N, FAR_N)).copy()
    exact = dataclasses.replace(pr, C_inv=C, m=m, K_inv=K)
    r32 = lambda A: A.astype(np.float32).astype(np.float64)
    Cr, Kr = C.copy(), K.copy()
    for rows, cols in ((slice(2 * TB, None), slice(0, TB)), (slice(0, TB), slice(2 * TB, None))):
        Kr[:, rows, cols] = r32(K[:, rows, cols])
        Cr[:, rows, cols] = r32((C + K)[:, rows, cols]) - Kr[:, rows, cols]
        assert np.array_equal((Cr + Kr)[:, rows, cols], r32((C + K)[:, rows, cols]))
    rounded = dataclasses.replace(pr, C_inv=Cr, m=m, K_inv=Kr)
    return exact, rounded, X


def _far_states(pr, X):
    """Two states: the fixture's smooth state with the grid points of block column 0 (state 0) / of block row 2 (state 1) times 2^20 --
    xc and f are large on the columns (rows) of block (2, 0) only, and the block's share of the products that land in block row 2 (0) is
    1e-6 and more of them.  With (sigma_pre, theta_pre) of the structureless fixtures."""
    from tests.util import STRUCTURELESS_SIG_PRE, structureless_theta
    Xa, Xb = X.copy(), X.copy()
    Xa[:TB] *= BIG
    Xb[2 * TB:] *= BIG
    sp = np.full((2, pr.D), STRUCTURELESS_SIG_PRE)
    tp = np.repeat(np.log(np.expm1(structureless_theta(pr.drift)))[None], 2, axis=0)
    return np.stack([Xa, Xb]), sp, tp


def _far_bound(pr, X, th_pre):
    """|change of gX| that rounding the far blocks to fp32 can cause, entry by entry: gX = -(1 / beta) (FH xc - FE^T f + J^T (FK f - FE xc))
    + the observation term, so  |d gX[i, d]| <= (1 / beta) (e_hx + e_etf + sum_d' |df_d' / dx_d|(i) (e_kf + e_ex)[i, d'])  with each
    e = 2^-24 |B| |v| over the far blocks B of the operator (FH, FK: block (2, 0) and its transpose; FE: (2, 0) and (0, 2))."""
    FH, FK, FE = (np.abs(A) for A in fused_operators(pr.C_inv, pr.m, pr.K_inv))
    th = np.log1p(np.exp(th_pre))
    S, E, I = X[:, 0], X[:, 1], X[:, 2]
    f = np.stack([-th[0] * S * I, th[0] * S * I - th[2] * E, th[2] * E - th[1] * I, th[1] * I], axis=1)
    J = np.zeros((len(X), 4, 4))                                # J[i, d', d] = |df_d' / dx_d|
    J[:, 0, 0] = J[:, 1, 0] = np.abs(th[0] * I)
    J[:, 0, 2] = J[:, 1, 2] = np.abs(th[0] * S)
    J[:, 1, 1] = J[:, 2, 1] = th[2]
    J[:, 2, 2] = J[:, 3, 2] = th[1]
    axc, af = np.abs(X - pr.mu[None]), np.abs(f)

    def far(A, v, transpose=False):                            # [N, D]: sum over the far blocks only
        out = np.zeros_like(v)
        for d in range(4):
            M = A[d].T if transpose else A[d]
            out[2 * TB:, d] += M[2 * TB:, :TB] @ v[:TB, d]
            out[:TB, d] += M[:TB, 2 * TB:] @ v[2 * TB:, d]
        return 2.0 ** -24 * out

    e_pt = far(FK, af) + far(FE, axc)
    return (far(FH, axc) + far(FE, af, transpose=True) + np.einsum("ikd,ik->id", J, e_pt)) / pr.beta


@pytest.mark.parametrize("states", [1, 2])
def test_a_demoted_block_enters_with_its_rounded_values_in_fp64_arithmetic(states):
    """fused log posterior, k_stream<1> (one state) and k_stream<2> (two), even and odd slot.  The gradient rows the far block feeds visibly
    (block row 2 for the state that is large on block column 0, block row 0 for the other) are compared over those rows:
      * with the oracle on the stacks that carry the fp32-rounded far blocks: 1e-12 of the rows' largest entry -- a skipped block would
        miss by >= 1e-6, a block read in another order or width by O(1);
      * with the oracle on the unrounded stacks: inside the rounding bound (_far_bound), plus the 1e-12 of the comparison above for the
        fp64 rounding both evaluations carry -- and not closer than 1e-11 somewhere: the rounding is there.
    The value is dominated by the large grid points and sees neither: it is held to 1e-12 as well."""
    exact, rounded, X = _far_block_case()
    Xb, sp, tp = _far_states(exact, X)
    eng = engine_for(exact)
    try:
        nb, nd, _ = eng.tile_formats(states)
        expect = [(d, k, bi, bj) for d, k, bi, bj, ok, _ in block_split(*fused_operators(exact.C_inv, exact.m, exact.K_inv)) if ok]
        assert nb == 84 and nd == len(expect) == 16 and all(abs(bi - bj) == 2 for _, _, bi, bj in expect)
        assert eng.stream_kernel_name(states) == f"k_stream<{states}>"
        args = (Xb[:states], sp[:states], tp[:states]) if states > 1 else (Xb[0], sp[0], tp[0])
        out = []
        for parity in (0, 1):
            eng.set_option("fused_parity", parity)
            res = eng.logpost_grad(*args, 1.0, fused=True)
            out.append(res if states > 1 else tuple(np.asarray(a)[None] for a in res))
        eng.set_option("fused_parity", 0)
        for a, b in zip(*out):
            np.testing.assert_array_equal(a, b, err_msg="even against odd slot")
    finally:
        eng.close()
    logp, gX = out[0][0], out[0][1]
    for c in range(states):
        rows = slice(2 * TB, None) if c == 0 else slice(0, TB)
        l_r, g_r, _, _ = orc.logpost_grad(Xb[c], sp[c], tp[c], 1.0, rounded)
        l_e, g_e, _, _ = orc.logpost_grad(Xb[c], sp[c], tp[c], 1.0, exact)
        scale = np.abs(g_r[rows]).max()
        to_rounded = np.abs(gX[c][rows] - g_r[rows]).max() / scale
        share = np.abs(g_r[rows] - orc.logpost_grad(Xb[c], sp[c], tp[c], 1.0, _without_far(exact))[1][rows]).max() / scale
        gap = np.abs(gX[c][rows] - g_e[rows])
        bound = _far_bound(exact, Xb[c], tp[c])[rows]
        print(f"state {c}/{states}: far blocks' share of the rows {share:.2e}; to the rounded oracle {to_rounded:.2e} (bar 1e-12); "
              f"to the unrounded one {gap.max() / scale:.2e}, largest gap / bound {np.max(gap / (bound + 1e-12 * scale)):.2f}; "
              f"value {abs(logp[c] - l_r) / abs(l_r):.2e}")
        assert share >= 1e-6
        assert to_rounded <= 1e-12
        assert (gap <= bound + 1e-12 * scale).all()
        assert gap.max() >= 1e-11 * scale
        assert abs(logp[c] - l_r) <= 1e-12 * abs(l_r)


def _without_far(pr):
    import dataclasses
    C, K = pr.C_inv.copy(), pr.K_inv.copy()
    for A in (C, K):
        A[:, 2 * TB:, :TB] = 0.0
        A[:, :TB, 2 * TB:] = 0.0
    return dataclasses.replace(pr, C_inv=C, K_inv=K)


# ---- opt-out and small grids are bit-identical -----------------------------------------------------------------------------------

@pytest.mark.parametrize("chains", [1, 2])
def test_option_off_at_a_demoting_shape_is_the_fp64_pack_however_it_was_reached(chains):
    """N = 512 with tile_demote = 0 from the start against a handle that packed WITH demotion first, then took the option and packed again
    (the option is read at the next pack; the narrow buffer and the descriptors' format bits go through the stale path): no block
    demoted, the fp64 byte count, and the same chain bit for bit."""
    off, state = _seir_engine(512, options={"tile_demote": 0})
    on, _ = _seir_engine(512)
    try:
        assert off.tile_formats(chains) == (144, 0, 144 * BLOCK_BYTES) and on.tile_formats(chains)[1] == 48
        a = _short_run(off, state, chains)
        on.set_option("tile_demote", 0)
        assert on.tile_formats(chains)[1] == 48                  # (not before the next pack)
        on.pack_resident(None)
        assert on.tile_formats(chains) == (144, 0, 144 * BLOCK_BYTES)
        _assert_runs_identical(a, _short_run(on, state, chains), f"N=512, {chains} chains")
    finally:
        off.close()
        on.close()


def _small_engine(N, band, options):
    """N = 161: the golden SEIR-3 fixture under b = 80 (two block rows, dense fused storage: 6 b + 1 >= N); N = 256: the benchmark's problem."""
    if N != 161:
        return _seir_engine(N, band, options)
    from tests.util import load_g4, problem_from_g4
    g = load_g4("seir3_N161")
    pr = problem_from_g4(g, band)
    eng = engine_for(pr, band, matrices=(g["C_inv"], g["m"], g["K_inv"]), options=options)
    return eng, orc.initial_state(g["Xhat_init"], g["sigma_sqs_init"], np.ones(pr.P), pr.LB)


@pytest.mark.parametrize("N,band", [(161, 80), (256, None)])
@pytest.mark.parametrize("chains", [1, 2])
def test_small_grids_demote_nothing_and_run_as_with_the_option_off(N, band, chains):
    runs = []
    for opt in (1, 0):
        eng, state = _small_engine(N, band, {"tile_demote": opt})
        try:
            assert eng.tile_formats(chains)[1] == 0
            runs.append(_short_run(eng, state, chains, deep=False))      # (short data: the trees need not be deep)
        finally:
            eng.close()
    _assert_runs_identical(*runs, f"N={N} b={band}, {chains} chains")


@pytest.mark.parametrize("chains", [1, 2])
def test_dense_stacks_without_decay_demote_nothing(chains):
    """Random dense stacks at N = 384 (the structureless fixture: far blocks as large as near ones): zero demoted blocks, bit-identical."""
    pr, X = fixture(384, "seir4", spd=True)
    from tests.util import STRUCTURELESS_SIG_PRE, structureless_theta
    sig0 = np.log1p(np.exp(STRUCTURELESS_SIG_PRE)) + pr.LB
    state = orc.initial_state(X, sig0, structureless_theta(pr.drift), pr.LB)
    runs = []
    for opt in (1, 0):
        eng = engine_for(pr, options={"tile_demote": opt})
        try:
            assert eng.tile_formats(chains)[:2] == (84, 0)
            runs.append(_short_run(eng, state, chains))
        finally:
            eng.close()
    _assert_runs_identical(*runs, f"structureless N=384, {chains} chains")


# ---- the sampler at a demoting shape -------------------------------------------------------------------------------------------

def test_checkpoint_of_a_demoting_pack_is_refused_under_the_other_setting():
    """The checkpoint tag mixes in the number of demoted blocks: N = 512, a checkpoint after one transition with the format on resumes on a
    handle with the format on (and continues bit for bit) and is refused, not silently continued on fp64 blocks, with the format off."""
    from magi_v2_amd.engine import MagiHipError
    engs = {opt: _seir_engine(512, options={"tile_demote": opt}) for opt in (1, 0)}
    try:
        on, state = engs[1]
        whole = _short_run(on, state, 1)
        cfg = on.default_cfg(num_results=2, num_burnin_steps=1, step_size=1e-3, max_tree_depth=4, stale_cache=0)
        on.sampler_init(cfg, *[np.asarray(v)[None] for v in state], seed=77, chain_ids=[5])
        on.sampler_run(1)
        ck = on.sampler_checkpoint()
        with pytest.raises(MagiHipError):
            engs[0][0].sampler_resume(cfg, ck, seed=77, chain_ids=[5])
        on.sampler_resume(cfg, ck, seed=77, chain_ids=[5])
        on.sampler_run(2)
        np.testing.assert_array_equal(on.sampler_samples()[0], whole[0])
    finally:
        for eng, _ in engs.values():
            eng.close()


def test_chain_at_n512_stays_within_the_fused_tolerances_and_resumes_bit_for_bit():
    """N = 512, SEIR-4, one chain, 3 NUTS transitions (trees capped at depth 5): fp32 far blocks against fp64 ones -- integers equal,
    target_log_prob to rtol 1e-9, X to 1e-8 max|X| (the bars tests/test_structureless_gpu.py holds the fused path to against the oracle);
    and with the format on, a run split 1 + 2 equals the run in one piece bit for bit (column sums per physical chunk: no slot parity in
    a demoted block's result)."""
    runs = {}
    for opt in (1, 0):
        eng, state = _seir_engine(512, options={"tile_demote": opt})
        try:
            runs[opt] = _short_run(eng, state, 1, depth=5)
            if opt:
                _assert_runs_identical(runs[1], _short_run(eng, state, 1, splits=(1, 2), depth=5), "split 1 + 2 against 3")
        finally:
            eng.close()
    (X1, s1, t1, i1, l1), (X0, s0, t0, i0, l0) = runs[1], runs[0]
    print("leapfrogs", i1[0].tolist(), "target_log_prob gap", np.abs(l1 / l0 - 1).max(), "X gap / max|X|", np.abs(X1 - X0).max() / np.abs(X0).max())
    np.testing.assert_array_equal(i1, i0)
    np.testing.assert_allclose(l1, l0, rtol=1e-9)
    np.testing.assert_allclose(X1, X0, rtol=0, atol=1e-8 * np.abs(X0).max())
