"""A re-used handle against a fresh one across every change of state.

Every other GPU comparison builds a new engine for the state it looks at (tests/util.py: engine_for); the drivers keep ONE handle alive and
move it through states -- bench.py times and profiles on the engine it sampled with and samples on, the sweeps push problem after problem
into a live handle, initial_fit stages its dense builds, update_kernel_matrices changes N, a second predict changes the chain count and the
kernel family.  The handle's device buffers only grow, several kernels rely on "entries never written stay zero", and the captured graph
holds pointers and constants by value: each test below takes one handle through a history H1 -> H2 -> ... -> S and asserts

  1. re-used == fresh, BIT FOR BIT (the raw float64): a second handle taken straight to S with the same options gives the same
     logpost_grad, logpost_grad(fused=True) in even and odd slots, and the same short NUTS and fixed-L HMC runs -- samples, every field of
     the diagnostics and of the sampler state.  Equality is what the design promises (fixed summation orders; a task table that depends on
     shape, band, options and CU count only; chains independent of their batch): a difference is a missing invalidation or memset;
  2. fresh == oracle for the log posterior at the project's bars (1e-10 three-phase, 1e-9 fused; _assert_close of
     tests/test_structureless_gpu.py).  Fresh-handle sampler parity is held by the other files.

tests/test_reuse_cpu.py proves on the oracle alone that the answer of the state BEFORE each transition differs by >= 1000 x those bars, and
that the histories pass through the storage modes and kernel families they name.  The states are structureless (every block matters) where
blocks are what could be stale.  Every negative path is a state check that returns before any launch."""
import numpy as np
import pytest

from tests.test_structureless_gpu import _assert_close
from tests.util import (REUSE_BANDS, REUSE_BATCHES, REUSE_BYTES, REUSE_DATA, REUSE_HMC, REUSE_NUTS, REUSE_SEED, REUSE_SHAPES, load_g4,
                        reuse_band_state, reuse_band_tables, reuse_block_counts, reuse_oracle_logpost, reuse_state)

pytestmark = pytest.mark.gpu

DIAG = ("step_size", "log_accept_ratio", "leapfrogs_taken", "tree_depth", "has_divergence", "reach_max_depth", "is_accepted",
        "target_log_prob", "energy", "beta_temp")
TEMP = 0.8
PAIR = ((1, "auto"), (5, "mc"))          # the batches most histories are checked on: k_stream<1>; five states on k_stream_sep<CW=8>
E_STATE = -5


def _engine(st, options=None):
    from magi_v2_amd.engine import MagiEngine
    eng = MagiEngine(0) if st.drift is None else MagiEngine(0, drift=st.drift)
    for k, v in (options or {}).items():
        eng.set_option(k, v)
    return eng


def _set_problem(eng, st):
    pr = st.pr
    eng.set_problem(pr.mu, pr.N_ds, pr.obs_idx, pr.y, pr.beta, pr.LB, st.drift if st.drift is not None else pr.drift)


def _load(eng, st):
    eng.set_matrices(*st.matrices, bandsize=st.band)
    if st.drift is not None:
        eng.set_times(st.times)
    _set_problem(eng, st)


def _refused(call):
    """An ordinary error return (MAGI_E_STATE): nothing was launched."""
    from magi_v2_amd.engine import MagiHipError
    with pytest.raises(MagiHipError) as e:
        call()
    assert e.value.code == E_STATE, str(e.value)


def _zero_states(eng, n=1):
    """States of the handle's current shape (its P that of the last problem: the refusals below come before anything is read)."""
    return np.zeros((n, eng.N, eng.D)), np.zeros((n, eng.D)), np.zeros((n, eng.P or 1))


def _run(eng, st, n, cfg_kw, seed=REUSE_SEED, steps=None):
    """A sampler run on the first n states of st (chain k: id 20 + k) -> {name: array}: samples, diagnostics, sampler state."""
    cfg = eng.default_cfg(**cfg_kw)
    eng.sampler_init(cfg, *st.states(n), seed=seed, chain_ids=list(range(20, 20 + n)))
    eng.sampler_run(cfg.num_burnin_steps + cfg.num_results if steps is None else steps)
    return _collect(eng)


def _collect(eng):
    out = dict(zip(("X", "sig_pre", "th_pre"), eng.sampler_samples()))
    d = eng.sampler_diag()
    out.update({"diag." + k: getattr(d, k) for k in DIAG})
    out.update(zip(("state.X", "state.sig_pre", "state.th_pre", "state.step_size", "state.beta_cache"), eng.sampler_state()))
    return out


def _observe(eng, st, n):
    """Everything the re-used handle is compared on: the log posterior three ways, a NUTS run, a fixed-L HMC run."""
    args = st.states(n)
    out = {}
    eng.set_option("fused_parity", 0)
    for tag, kw in (("three", {}), ("even", dict(fused=True))):
        out.update(zip((f"{tag}.L", f"{tag}.gX", f"{tag}.gs", f"{tag}.gt"), eng.logpost_grad(*args, TEMP, **kw)))
    eng.set_option("fused_parity", 1)
    out.update(zip(("odd.L", "odd.gX", "odd.gs", "odd.gt"), eng.logpost_grad(*args, TEMP, fused=True)))
    eng.set_option("fused_parity", 0)
    out.update({"nuts." + k: v for k, v in _run(eng, st, n, REUSE_NUTS).items()})
    out.update({"hmc." + k: v for k, v in _run(eng, st, n, REUSE_HMC).items()})
    assert out["nuts.diag.leapfrogs_taken"].min() >= 1 and (out["hmc.diag.leapfrogs_taken"] == REUSE_HMC["hmc_leapfrogs"]).all()
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _assert_same(got, ref, what, keys=None, sl=None):
    """Bit for bit: np.array_equal on the raw float64."""
    assert set(got) == set(ref)
    for k in (keys or sorted(ref)):
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        if sl is not None and k.split(".")[-2:-1] == ["diag"]:
            a, b = a[sl], b[sl]
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (what, k, float(np.abs(a - b).max()))


_fresh = {}


def _fresh_obs(name, n, family="auto"):
    """_observe of a handle taken straight to the state, held to the oracle (log posterior only); once per session, read-only."""
    key = (name, n, family)
    if key not in _fresh:
        st = reuse_state(name)
        eng = _engine(st, {"stream_family": family})
        try:
            _load(eng, st)
            obs = _observe(eng, st, n)
            kernel = eng.stream_kernel_name(n)
        finally:
            eng.close()
        X, sp, tp = st.states(n)
        for c in range(n):
            truth = reuse_oracle_logpost(st, X[c], sp[c], tp[c], TEMP)
            _assert_close([obs[f"three.{f}"][c] for f in ("L", "gX", "gs", "gt")], truth, 1e-10, f"{name} fresh {kernel} three-phase {c}/{n}")
            _assert_close([obs[f"even.{f}"][c] for f in ("L", "gX", "gs", "gt")], truth, 1e-9, f"{name} fresh {kernel} fused {c}/{n}")
        _fresh[key] = obs
    return _fresh[key]


def _check(eng, st, what, batches=PAIR):
    for n, family in batches:
        eng.set_option("stream_family", family)
        _assert_same(_observe(eng, st, n), _fresh_obs(st.name, n, family), f"{what}: {st.name}, {n} states, {family}")


# ---- 1: the band on resident matrices ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ["pack_resident", "set_matrices"])
def test_band_changes_on_resident_matrices(route):
    """dense -> 20 -> 0 -> 43 -> dense -> 20 at N = 384 (three block rows), by pack_resident(b) with no upload and by set_matrices(...,
    bandsize=b).  At 20 (fb = 60, wb = 1) the far tiles of the dense pack are still in the tile buffer and the far product slots of the
    last dense evaluation in tpart; at 43 (fb = 129, wb = 2) the far blocks return; three-phase storage switches between dense and banded
    rows at every step.  After every step: one state on k_stream<1>, five on k_stream_sep<CW=8>."""
    st = reuse_band_state(None)
    eng = _engine(st)
    try:
        _load(eng, st)
        _check(eng, st, route)
        for b in REUSE_BANDS[1:]:
            st = reuse_band_state(b)
            if route == "pack_resident":
                eng.pack_resident(b)                                       # (same shape: the problem stays)
                _refused(lambda: eng.sampler_run(1))
            else:
                eng.set_matrices(*st.matrices, bandsize=b)
                _set_problem(eng, st)
            _check(eng, st, f"{route} -> {b}")
    finally:
        eng.close()


# ---- 2: the shape -----------------------------------------------------------------------------------------------------------------

def test_shape_changes_under_a_live_handle():
    """N = 384 x 4 -> 41 x 4 -> 161 x 3 -> 384 x 4: the grow-only buffers hold the larger problem's contents under a smaller one and the
    other way round.  After each matrix change and before set_problem, logpost_grad, sampler_init and time_gradient return MAGI_E_STATE."""
    eng = None
    try:
        for k, name in enumerate(REUSE_SHAPES):
            st = reuse_state(name)
            if eng is None:
                eng = _engine(st)
            eng.set_matrices(*st.matrices, bandsize=None)
            if k:
                X, sp, tp = _zero_states(eng)
                _refused(lambda: eng.logpost_grad(X, sp, tp))
                _refused(lambda: eng.sampler_init(eng.default_cfg(**REUSE_NUTS), X, sp, tp, seed=1))
                _refused(lambda: eng.time_gradient(1, 3))
            _set_problem(eng, st)
            _check(eng, st, f"shape {k}")
    finally:
        eng.close()


# ---- 3: problem data and drift on unchanged matrices ------------------------------------------------------------------------------

def test_problem_data_and_drift_change_on_unchanged_matrices():
    """set_problem on a live handle, as the sweeps do: another data set of the same shape, back; the seir4 problem on the same D = 4
    matrices (P = 3 against 5: dimp changes), back.  A sampler initialised before the change must not run on."""
    first = reuse_state(REUSE_DATA[0])
    eng = _engine(first)
    try:
        _load(eng, first)
        _check(eng, first, "data 0")
        for k, name in enumerate(REUSE_DATA[1:], 1):
            st = reuse_state(name)
            _set_problem(eng, st)
            _refused(lambda: eng.sampler_run(1))
            _check(eng, st, f"data {k}")
    finally:
        eng.close()


# ---- 4: chain count and kernel family ---------------------------------------------------------------------------------------------

def test_chain_count_and_kernel_family_change_on_one_problem():
    """Batches 9 -> 2 -> 16 -> 8 -> 1 -> 3 -> 17 with set_option("stream_family", ...) on the live handle in between: k_stream_sep<16> ->
    k_stream<2> -> sep<16> -> sep<8> -> k_stream<1> -> sep<8> (forced) -> sep<16> with a ragged second group.  Chain k has state k and id
    20 + k in every batch.
    (A library built WITHOUT the two hipMemsetAsync calls of magi_ensure_chains passes this history and the others unchanged: the point
    kernels add only the product slots inside the block band and of used basis functions, all written in the same slot, and a matrix-core
    column depends on its own operand column alone while only columns in use are stored -- the zeros guard nothing a kernel reads today.
    What the comparisons do catch, tried on scratch builds: operator tiles kept across a re-pack, mu / beta kept across set_problem.)"""
    st = reuse_state("A")
    eng = _engine(st)
    try:
        _load(eng, st)
        for n, family, kernel in REUSE_BATCHES:
            eng.set_option("stream_family", family)
            assert eng.stream_kernel_name(n) == kernel
            _check(eng, st, f"batch {n}", batches=((n, family),))
    finally:
        eng.close()


# ---- 5: a sampler after a sampler -------------------------------------------------------------------------------------------------

def _fresh_run(st, n, cfg_kw, seed=REUSE_SEED, steps=None):
    eng = _engine(st)
    try:
        _load(eng, st)
        return _run(eng, st, n, cfg_kw, seed, steps)
    finally:
        eng.close()


def test_sampler_after_sampler_and_checkpoint_resumed_in_the_same_handle():
    """NUTS on 3 chains paused after 3 of 7 transitions and abandoned; fixed-L HMC on 2 chains; NUTS again with another seed and tree depth:
    each equals a fresh handle's run.  Then a checkpoint of a paused run, an HMC run in between, and the checkpoint resumed IN THE SAME
    handle: the remaining transitions are the uninterrupted run's (the existing checkpoint test resumes in a new handle only)."""
    st = reuse_state("A")
    other = dict(REUSE_NUTS, max_tree_depth=5)
    eng = _engine(st)
    try:
        _load(eng, st)
        _run(eng, st, 3, REUSE_NUTS, steps=3)
        assert list(eng.sampler_steps_done()) == [3, 3, 3]
        _assert_same(_run(eng, st, 2, REUSE_HMC), _fresh_run(st, 2, REUSE_HMC), "HMC after an abandoned NUTS run")
        _assert_same(_run(eng, st, 3, other, seed=909), _fresh_run(st, 3, other, seed=909), "NUTS after HMC")
        whole = _fresh_run(st, 3, REUSE_NUTS)
        _run(eng, st, 3, REUSE_NUTS, steps=3)
        ck = eng.sampler_checkpoint()
        assert list(ck["scalars"][:, 0]) == [3.0] * 3
        _run(eng, st, 2, REUSE_HMC)
        eng.sampler_resume(eng.default_cfg(**REUSE_NUTS), ck, seed=REUSE_SEED, chain_ids=[20, 21, 22])
        eng.sampler_run(4)
        _assert_same(_collect(eng), whole, "checkpoint resumed in the same handle", sl=(slice(None), slice(3, None)))
    finally:
        eng.close()


def test_grow_only_buffers_under_a_capacity_larger_than_the_need():
    """The buffers that grow and never shrink (csrc/magi_internal.h: magi_grow) and that no other history compares, at N = 41: the sample
    buffer and the eight diagnostics arrays sized by a NUTS run of 3 chains x (8 + 6) transitions, then REUSE_NUTS on 2 chains paused after
    3 of its 7 -- every transition not taken reads as the NaN / -1 fill over the first run's rows, as on a fresh handle paused at the same
    place (tests/test_reuse_cpu.py: the rows differ wherever they could be stale); dense_apply with 1, 8 and 1 vectors, the work-space
    slot and the pinned staging growing and then re-used under a larger capacity, each call against a fresh handle's; the first run again."""
    from tests.util import REUSE_GROW
    st = reuse_state("C41")
    total, taken = REUSE_NUTS["num_burnin_steps"] + REUSE_NUTS["num_results"], 3
    rng = np.random.default_rng(11)
    eng = _engine(st)
    try:
        _load(eng, st)
        whole = _run(eng, st, 3, REUSE_GROW)
        assert whole["diag.step_size"].shape == (3, 14) and np.isfinite(whole["X"]).all() and np.isfinite(whole["diag.energy"]).all()
        paused = _run(eng, st, 2, REUSE_NUTS, steps=taken)
        assert list(eng.sampler_steps_done()) == [taken] * 2
        _assert_same(paused, _fresh_run(st, 2, REUSE_NUTS, steps=taken), "a paused run under a larger capacity")
        assert paused["diag.energy"].shape == (2, total) and np.isfinite(paused["diag.energy"][:, :taken]).all()
        assert np.isnan(paused["diag.energy"][:, taken:]).all() and np.isnan(paused["diag.step_size"][:, taken:]).all()
        assert (paused["diag.leapfrogs_taken"][:, taken:] == -1).all() and (paused["diag.tree_depth"][:, taken:] == -1).all()
        assert all(np.isnan(paused[k]).all() for k in ("X", "sig_pre", "th_pre"))         # (three burn-in transitions: no draw stored)
        for nv in (1, 8, 1):
            V = rng.standard_normal((eng.D, eng.N, nv))
            fresh = _engine(st)
            try:
                fresh.set_matrices(*st.matrices, bandsize=None)
                for which in ("C_inv", "m", "K_inv"):
                    for tr in (False, True):
                        a, b = eng.dense_apply(which, V, transpose=tr), fresh.dense_apply(which, V, transpose=tr)
                        assert a.shape == (eng.D, eng.N, nv) and np.array_equal(_bits(a), _bits(b)), (nv, which, tr)
            finally:
                fresh.close()
        _assert_same(_run(eng, st, 3, REUSE_GROW), whole, "the first run again")
        _assert_same(whole, _fresh_run(st, 3, REUSE_GROW), "the first run against a fresh handle's")
    finally:
        eng.close()


# ---- 6: the instruments -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("instrument", ["time_gradient_same_n", "time_gradient_other_n", "sampler_profile"])
def test_instruments_leave_a_handle_that_equals_a_fresh_one(instrument):
    """What bench.py --full calls on the engine it has just sampled with, and samples on afterwards: time_gradient(n, 3) with n the last
    batch and another one, sampler_profile(8).  Afterwards the sampler calls return MAGI_E_STATE (the chain state is clobbered); then the
    log posterior and a re-initialised sampler equal a fresh handle's.  time_gradient on a group handle is refused."""
    from magi_v2_amd.engine import MagiGroup
    st, n = reuse_state("A"), 3
    eng = _engine(st)
    try:
        _load(eng, st)
        if instrument == "sampler_profile":
            cfg = eng.default_cfg(**REUSE_NUTS)
            eng.sampler_init(cfg, *st.states(n), seed=REUSE_SEED, chain_ids=[20, 21, 22])
            stream_us, point_us, lf = eng.sampler_profile(8)
            print(instrument, stream_us, point_us, lf)
            assert np.isfinite([stream_us, point_us]).all() and stream_us > 0 and point_us > 0 and 1 <= lf <= 8 * n
        else:
            _run(eng, st, n, REUSE_NUTS)
            total, phases = eng.time_gradient(n if instrument == "time_gradient_same_n" else 2, 3)
            print(instrument, total, phases)
            assert np.isfinite(total) and total > 0 and np.isfinite(phases).all() and (phases > 0).all()
        _refused(lambda: eng.sampler_run(1))
        _refused(eng.sampler_samples)
        _refused(eng.sampler_state)
        _refused(eng.sampler_summary)
        _check(eng, st, instrument, batches=((n, "auto"), (5, "mc")))
        g = MagiGroup([eng])
        try:
            _refused(lambda: g.time_gradient(1, 3))
        finally:
            g.close()
    finally:
        eng.close()


def test_profiled_build_then_unprofiled_build_and_sampler_profile():
    """build_profile on at N = 161, then off: the same matrices bit for bit, and no event left attached -- a following sampler_profile
    still reports times."""
    st = reuse_state("C161")
    g = load_g4("seir3_N161")
    eng = _engine(st)
    try:
        eng.set_option("build_profile", 1)
        profiled = eng.build_matrices(g["I"], g["phi1s"], g["phi2s"], 2.01)
        assert sum(v[2] for v in eng.build_profile().values()) > 0
        eng.set_option("build_profile", 0)
        plain = eng.build_matrices(g["I"], g["phi1s"], g["phi2s"], 2.01)
        for a, b in zip(profiled, plain):
            assert np.array_equal(_bits(a), _bits(b))
        _set_problem(eng, st)
        eng.sampler_init(eng.default_cfg(**REUSE_NUTS), *st.states(2), seed=REUSE_SEED, chain_ids=[20, 21])
        stream_us, point_us, lf = eng.sampler_profile(8)
        assert np.isfinite([stream_us, point_us]).all() and stream_us > 0 and point_us > 0 and 1 <= lf <= 16
    finally:
        eng.close()


# ---- 7: gradient_bytes ------------------------------------------------------------------------------------------------------------

def test_gradient_bytes_against_an_independent_block_count():
    """phase_bytes[4] of a VALU batch is n_tasks (128 x 128 x 8 + n x 2 x 128 x 8) -- bench.py derives its roofline's block count from it;
    n_tasks must be the number of 128 x 128 blocks that hold an entry within fb of the diagonal (lower block triangle for FH and FK, all
    blocks for FE; tests/util.py: reuse_block_counts builds the index sets in numpy): a block too many is a performance bug, a block too
    few a correctness bug.  At b = 0 the library's wb = 1 keeps off-diagonal blocks that the mask empties: only "none missing" is asserted
    there.  bytes[0..3] and [7] are the three-phase formulas (include/magi_hip.h; csrc/capi.hip names the operands) with W = N dense and
    2 b + 1 banded.  One handle throughout: the band by pack_resident, the shape by set_matrices.  Without matrices: MAGI_E_STATE."""
    eng = _engine(reuse_state("A"))
    try:
        _refused(lambda: eng.gradient_bytes(1))
        loaded = None
        for name, band in REUSE_BYTES:
            st = reuse_state(name)
            if loaded != name:
                eng.set_matrices(*st.matrices, bandsize=band)
                _set_problem(eng, st)
                loaded = name
            else:
                eng.pack_resident(band)
            eng.set_option("stream_family", "auto")
            N, D = eng.N, eng.D
            independent, library = reuse_block_counts(N, D, band)
            banded, W, _, _, _ = reuse_band_tables(N, band)
            for n in (1, 2):
                assert eng.stream_kernel_name(n) == f"k_stream<{n}>"
                b = eng.gradient_bytes(n)
                n_tasks = b[4] / (128 * 128 * 8 + n * 2 * 128 * 8)
                print(name, band, n, "blocks:", n_tasks, "independent count", independent)
                assert n_tasks == int(n_tasks)
                if band == 0:
                    assert n_tasks >= independent and n_tasks == library
                else:
                    assert n_tasks == independent
                mat, vec = D * N * W * 8.0, n * N * D * 8.0
                assert list(b[:4]) == [2 * mat + 3 * vec, mat + 2 * vec, mat + 5 * vec, 5 * vec] and b[7] == 3 * mat + 10 * vec
    finally:
        eng.close()


# ---- 8: the staged dense build ----------------------------------------------------------------------------------------------------

_whole = {}


def _staged_inputs(N):
    g = load_g4("seir3_N161")
    I = np.arange(N) * float(g["I"][1] - g["I"][0])                           # the golden grid's spacing at both sizes
    return I, np.asarray(g["phi1s"], dtype=np.float64), np.asarray(g["phi2s"], dtype=np.float64)


def _whole_build(N):
    """One build_matrices of all three components on a fresh handle; once per session, read-only."""
    if N not in _whole:
        from magi_v2_amd.engine import MagiEngine
        I, phi1, phi2 = _staged_inputs(N)
        eng = MagiEngine(0)
        try:
            _whole[N] = eng.build_matrices(I, phi1, phi2, 2.01)
        finally:
            eng.close()
    return _whole[N]


@pytest.mark.parametrize("N,first,second,serial", [(161, [1, 2], [0], 0), (161, [2, 0], [1], 0), (300, [1, 2], [0], 0), (300, [2, 0], [1], 1),
                                                   (161, [1, 2], [0], 1)])
def test_staged_dense_build_equals_one_build(N, first, second, serial):
    """initial_fit builds the observed components, works on them, builds the others and only then packs: build_dense(sel) twice --
    ascending and descending / non-contiguous, batched and build_serial -- at N = 161 and N = 300 (three Cholesky blocks), on a handle that
    held another shape before.  Unbuilt components read as exact zeros, logpost_grad is refused until pack_resident, the staged stacks
    equal one build_matrices bit for bit, dense_apply on them equals numpy (the bar of tests/test_shuffled_grid_gpu.py), a rebuilt
    component changes alone, a build at another N zeroes every component."""
    prev = reuse_state("C41")
    I, phi1, phi2 = _staged_inputs(N)
    whole = _whole_build(N)
    eng = _engine(prev, {"build_serial": serial})
    same = lambda a, b: np.array_equal(_bits(a), _bits(b))
    try:
        _load(eng, prev)
        eng.logpost_grad(*prev.states(2))
        eng.build_dense(I, 3, first, phi1[first], phi2[first])
        _refused(lambda: eng.logpost_grad(*_zero_states(eng)))
        for got, ref in zip(eng.get_dense(), whole):
            assert not got[second[0]].any()
            for d in first:
                assert same(got[d], ref[d]), d
        eng.build_dense(I, 3, second, phi1[second], phi2[second])
        _refused(lambda: eng.logpost_grad(*_zero_states(eng)))
        rng = np.random.default_rng(3)
        for nv in (1, 3, 8):
            V = rng.standard_normal((3, N, nv))
            for which, A in zip(("C_inv", "m", "K_inv"), whole):
                atol = 1e-12 * np.abs(A).max()
                np.testing.assert_allclose(eng.dense_apply(which, V), np.einsum("dij,djp->dip", A, V), rtol=1e-12, atol=atol, err_msg=which)
                np.testing.assert_allclose(eng.dense_apply(which, V, transpose=True), np.einsum("dji,djp->dip", A, V), rtol=1e-12, atol=atol,
                                           err_msg=which + "^T")
        eng.pack_resident(None)
        staged = eng.get_dense()
        for got, ref in zip(staged, whole):
            assert same(got, ref)
        eng.build_dense(I, 3, [1], 1.3 * phi1[[1]], 1.1 * phi2[[1]])
        for got, ref in zip(eng.get_dense(), whole):
            assert same(got[0], ref[0]) and same(got[2], ref[2]) and not same(got[1], ref[1])
        eng.build_dense(I[:-1], 3, [0], phi1[[0]], phi2[[0]])
        for got in eng.get_dense():
            assert got.shape == (3, N - 1, N - 1) and got[0].any() and not got[1].any() and not got[2].any()
    finally:
        eng.close()


# ---- 9: group members changed between initialisations -----------------------------------------------------------------------------

def test_group_member_changed_between_initialisations():
    """include/magi_hip.h: "a member changed later takes effect at the next magi_sampler_init".  Two N = 41 members, a group run,
    set_problem on member 1 with other data, the group initialised again: its chains equal a fresh group's, the other member's chains are
    unchanged bit for bit."""
    from magi_v2_amd.engine import MagiGroup
    a, b = reuse_state("C41"), reuse_state("C41*")
    states = [np.concatenate([x[:2], x[:2]]) for x in a.batch]
    ids = [20, 21, 20, 21]

    def group_run(g):
        g.sampler_init(g.default_cfg(**REUSE_NUTS), *states, seed=REUSE_SEED, chain_ids=ids)
        g.sampler_run(REUSE_NUTS["num_burnin_steps"] + REUSE_NUTS["num_results"])
        return _collect(g)

    def members(sts):
        engs = []
        for st in sts:
            engs.append(_engine(st))
            _load(engs[-1], st)
        return engs

    engs = members([a, a])
    g = MagiGroup(engs)
    try:
        before = group_run(g)
        _set_problem(engs[1], b)
        after = group_run(g)
    finally:
        g.close()
        for e in engs:
            e.close()
    engs = members([a, b])
    g = MagiGroup(engs)
    try:
        fresh = group_run(g)
    finally:
        g.close()
        for e in engs:
            e.close()
    _assert_same(after, fresh, "group after a member changed")
    for k in before:
        assert np.array_equal(_bits(before[k][:2]), _bits(after[k][:2])), k                 # member 0
        assert np.array_equal(_bits(before[k][:2]), _bits(before[k][2:])), k                # (the same problem and ids twice)
    assert not np.array_equal(after["X"][:2], after["X"][2:])


# ---- 10: the times on a live handle -----------------------------------------------------------------------------------------------

def test_times_change_on_a_live_handle():
    """seir_seasonal at N = 41: after a sampler run set_times(t + 0.37) at the same N -- the graph held the old pointer and constants, the
    operand mirror basis functions of the old times.  Log posterior and a re-initialised run equal a fresh handle given the shifted times
    and differ from the unshifted ones by more than 1e-3 relative."""
    st, shifted = reuse_state("T"), reuse_state("T+0.37")
    eng = _engine(st)
    try:
        _load(eng, st)
        _check(eng, st, "times")
        eng.set_times(shifted.times)
        _refused(lambda: eng.sampler_run(1))
        _check(eng, shifted, "times shifted")
    finally:
        eng.close()
    for n, family in PAIR:
        old, new = _fresh_obs("T", n, family), _fresh_obs("T+0.37", n, family)
        for tag in ("three", "even"):
            assert (np.abs(new[tag + ".L"] - old[tag + ".L"]) > 1e-3 * np.abs(old[tag + ".L"])).all()
            assert np.abs(new[tag + ".gX"] - old[tag + ".gX"]).max() > 1e-3 * np.abs(old[tag + ".gX"]).max()
