"""Every reader of certified fp32 operator blocks against truth on the graded fixture (tests/demote_reference.py): ragged grids (N = 300: a
last block of 44 rows; 513: of one), FE != FK and not symmetric, a split in which demoted and kept blocks interleave, a first neighbour
qualifies and FH is kept beside a demoted FK / FE -- so that a reader which takes another operator's narrow copy, reads a block transposed
or takes the neighbouring slot of the narrow buffer gets other numbers.  tests/test_demote_edges_cpu.py proves, on the oracle alone, that
every demoted block is visible at the bars used here by a factor 1000, the rounding itself by a factor 10, and that the oracle sits a
factor 100 below them.

  * the VALU kernels (k_stream<1>, <2>, their per-drift builds for a traced and a time-dependent drift) read the narrow copies: compared
    set by set with the oracle on the ROUNDED stacks at 1e-12 of the set's largest entry; against the unrounded stacks inside the rounding
    bound and not closer than 10 bars somewhere;
  * the matrix-core kernels (k_stream_sep<8|16>, k_stream_mc) read the rounded doubles: 2 sum_bound entrywise (the first-order error of any
    summation order) against the rounded stacks, and just as far from the unrounded ones;
  * the sampler, a problem group whose members demote different sets or nothing, one handle packed again and again, banded storage.

The sampler comparisons cannot see a demoted block (the density's far blocks weigh 1e-11 at an ordinary state): they hold the
machinery -- slots, task words, buffers that grow and shrink -- to a fresh handle bit for bit, and the chain to the oracle's."""
import numpy as np
import pytest

from oracle import magi_oracle as orc
from tests import demote_reference as dr
from tests.test_structureless_cpu import fixture
from tests.test_tile_demote_gpu import BLOCK_BYTES
from tests.util import STRUCTURELESS_SIG_PRE, engine_for, reuse_auto_kernel, structureless_theta

pytestmark = pytest.mark.gpu

DIAG = ("step_size", "log_accept_ratio", "leapfrogs_taken", "tree_depth", "has_divergence", "reach_max_depth", "is_accepted", "energy",
        "target_log_prob", "beta_temp")
NUTS = dict(num_results=2, num_burnin_steps=1, step_size=1e-3, max_tree_depth=4, stale_cache=0)     # tests/test_tile_demote_gpu.py: _short_run
SEED = 77


HIP_ATTRIBUTE_MULTIPROCESSOR_COUNT = 63                         # hipDeviceAttributeMultiprocessorCount in hip_runtime_api.h of HIP 7.2


def _compute_units():
    """Compute units of device 0 from the HIP runtime the library has loaded (torch, imported after it, brings a runtime of its own that
    finds no device), or None where the answer is not a plausible count -- another HIP's numbering of the attribute."""
    import ctypes
    try:
        with open("/proc/self/maps") as fh:                      # the runtime the library brought into this process
            path = next(line.split()[-1] for line in fh if "libamdhip64" in line)
        hip = ctypes.CDLL(path)
        n = ctypes.c_int(0)
        if hip.hipDeviceGetAttribute(ctypes.byref(n), HIP_ATTRIBUTE_MULTIPROCESSOR_COUNT, 0) != 0:
            return None
    except (OSError, AttributeError, StopIteration):
        return None
    return n.value if 8 <= n.value <= 1024 and n.value % 8 == 0 else None


def _engine(g, band=None, options=None):
    return engine_for(g.exact, band, drift=g.traced, options=options)


def _fused(eng, g, idx):
    """Fused log posterior of the states `idx` (one call), even and odd slot bit for bit equal: (logp[n], gX[n, N, D])."""
    X = np.stack([g.states[j].X for j in idx])
    sp, tp = np.repeat(g.sp[None], len(idx), axis=0), np.repeat(g.tp[None], len(idx), axis=0)
    args = (X, sp, tp) if len(idx) > 1 else (X[0], sp[0], tp[0])
    out = []
    for parity in (0, 1):
        eng.set_option("fused_parity", parity)
        res = eng.logpost_grad(*args, 1.0, fused=True)
        out.append(res if len(idx) > 1 else tuple(np.asarray(a)[None] for a in res))
    eng.set_option("fused_parity", 0)
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b, err_msg=f"states {idx}: even against odd slot")
    return np.asarray(out[0][0]), np.asarray(out[0][1])


def _check(g, j, ref, logp, gX, entrywise, what):
    """State j's gradient over its compared sets.  entrywise False: the bar is 1e-12 of the set's largest entry; True: 2 sum_bound."""
    st = g.states[j]
    worst = far = 0.0
    for (bi, e), (got, r, x, b, rb) in dr.set_views(g, st, gX, ref.gX, ref.gX_exact, ref.bound, ref.rounding):
        bar = 2.0 * b if entrywise else np.full_like(b, dr.VALU_BAR * np.abs(r).max())
        to_rounded, gap = np.abs(got - r), np.abs(got - x)
        worst, far = max(worst, (to_rounded / bar).max()), max(far, (gap / bar).max())
        assert (to_rounded <= bar).all(), (what, st.name, (bi, e), float((to_rounded / bar).max()))
        assert (gap <= rb + bar).all(), (what, st.name, (bi, e), "outside the rounding bound")
    value = abs(logp - ref.logp) / abs(ref.logp)
    print(f"{what} {st.name}: to the rounded oracle {worst:.3g} bars over {len(st.sets)} sets, to the unrounded one {far:.3g} bars; value {value:.2e}")
    assert far >= 10.0, (what, st.name, far)                     # the rounding is there: not the unrounded doubles
    assert value <= 1e-12, (what, st.name, value)


def _expect_pack(eng, g):
    nb, nd, by = eng.tile_formats(1)
    assert (nb, nd) == (len(g.split), len(g.demoted)), (nb, nd)
    if eng.stream_kernel_name(1) == "k_stream<1>":               # (not under stream_family = "mc": those kernels stream every block's doubles)
        assert by == (nb - nd) * BLOCK_BYTES + nd * BLOCK_BYTES / 2


# ---- the VALU readers ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,drift", [(N, d) for d in ("seir4", "ptrans", "seir_seasonal") for N in (300, 513)] + [(1024, "seir4")])
def test_valu_kernels_read_every_narrow_copy_as_the_oracle_has_it(N, drift):
    """Every state alone (k_stream<1>) and, below N = 1024, in pairs (k_stream<2>: each state once in either half of a pair).  N = 1024 is the
    production shape: 544 blocks + 1 on 256 compute units are three launch rounds and the task list -- over which the slots of the narrow
    buffer are numbered -- is permuted."""
    g, refs = dr.graded(N, drift), dr.references(N, drift)
    eng = _engine(g)
    try:
        _expect_pack(eng, g)
        assert eng.stream_kernel_name(1) == "k_stream<1>" and eng.stream_kernel_name(2) == "k_stream<2>"
        if N == 1024:
            cus = _compute_units()
            launched = len(g.split) + 1
            print(f"{cus} compute units, {launched} workgroups")
            if cus == 256:                                       # csrc/pack.hip: exactly three rounds, more than one workgroup in the last
                assert -(-launched // cus) == 3 and launched % cus > 1
        singles = [_fused(eng, g, [j]) for j in range(g.nb)]
        pairs = [_fused(eng, g, [j, (j + 1) % g.nb]) for j in range(g.nb)] if N < 1024 else []
    finally:
        eng.close()
    for j in range(g.nb):
        _check(g, j, refs[j], singles[j][0][0], singles[j][1][0], False, f"N={N} {drift} k_stream<1>")
    for j, (logp, gX) in enumerate(pairs):
        for c, k in enumerate((j, (j + 1) % g.nb)):
            _check(g, k, refs[k], logp[c], gX[c], False, f"N={N} {drift} k_stream<2> half {c}")


# ---- the matrix-core readers ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,drift", [(300, "seir4"), (513, "seir4"), (300, "ptrans"), (513, "ptrans")])
def test_matrix_core_kernels_multiply_the_same_rounded_operator(N, drift, stream_family):
    """Batches of 3, 8, 9 and 17 states (the fixture's states in turn): k_stream_sep<CW=8>, <CW=16> and a second chain group with a ragged
    tail; k_stream_mc for the protein-transduction drift, which is not separable.  Under the library's own rule N = 300 (84 blocks) keeps
    three states on k_stream<2>, a pair and a single-state tail, and those read the narrow copies: they are held to the VALU bar."""
    g, refs = dr.graded(N, drift), dr.references(N, drift)
    eng = _engine(g)
    try:
        _expect_pack(eng, g)
        if (N, stream_family) == (300, "auto"):
            assert eng.stream_kernel_name(3) == "k_stream<2>"
        runs = []
        for n in (3, 8, 9, 17):
            name = eng.stream_kernel_name(n)
            assert name == reuse_auto_kernel(len(g.split), n, stream_family, separable=drift != "ptrans"), (n, name)
            if not name.startswith("k_stream<"):                 # the matrix-core kernels stream every block's doubles
                assert eng.tile_formats(n)[2] == len(g.split) * BLOCK_BYTES
            idx = [(c + n) % g.nb for c in range(n)]
            runs.append((name, idx, _fused(eng, g, idx)))
    finally:
        eng.close()
    assert any(not name.startswith("k_stream<") for name, _, _ in runs)
    for name, idx, (logp, gX) in runs:
        for c in range(len(idx)):
            _check(g, idx[c], refs[idx[c]], logp[c], gX[c], not name.startswith("k_stream<"), f"N={N} {drift} {name} state {c}/{len(idx)}")


# ---- the sampler -----------------------------------------------------------------------------------------------------------------------

def _inits(pr, X):
    sig0 = np.log1p(np.exp(STRUCTURELESS_SIG_PRE)) + pr.LB
    th0 = structureless_theta(pr.drift)
    return sig0, th0, orc.initial_state(X, sig0, th0, pr.LB)


def _nuts(eng, starts, ids, splits=(3,)):
    """3 NUTS transitions from `starts` = [(X0, sig_pre0, th_pre0)] per chain: {name: array} of samples and every diagnostic."""
    cfg = eng.default_cfg(**NUTS)
    eng.sampler_init(cfg, *[np.stack([np.asarray(s[k]) for s in starts]) for k in range(3)], seed=SEED, chain_ids=list(ids))
    for n in splits:
        eng.sampler_run(n)
    out = dict(zip(("X", "sig_pre", "th_pre"), eng.sampler_samples()))
    d = eng.sampler_diag()
    out.update({k: getattr(d, k) for k in DIAG})
    assert out["leapfrogs_taken"].max() >= 7                     # (trees of depth 3 and more)
    return out


def _assert_identical(a, b, what, rows=slice(None)):
    for k in a:
        np.testing.assert_array_equal(a[k][rows], b[k], err_msg=f"{what}: {k}")


@pytest.mark.parametrize("chains", [1, 2, 3])
def test_chains_at_n300_match_the_oracle_on_the_rounded_stacks_draw_for_draw(chains):
    """N = 300, SEIR-4: k_stream<1>, k_stream<2>, and a pair with a single-chain tail (84 blocks: three chains stay on the VALU kernels).
    Integer diagnostics equal, X to 1e-8 max|X|, target_log_prob to rtol 1e-9; a run split 1 + 2 equals the run in one piece bit for bit."""
    g = dr.graded(300, "seir4")
    sig0, th0, start = _inits(g.rounded, g.X)
    ids = list(range(5, 5 + chains))
    eng = _engine(g)
    try:
        _expect_pack(eng, g)
        assert eng.stream_kernel_name(chains) == ("k_stream<1>" if chains == 1 else "k_stream<2>")
        whole = _nuts(eng, [start] * chains, ids)
        _assert_identical(whole, _nuts(eng, [start] * chains, ids, splits=(1, 2)), "split 1 + 2 against 3")
    finally:
        eng.close()
    for i, chain in enumerate(ids):
        trace = []
        oX, _, otp, _, _ = orc.sample_chain(g.rounded, g.X, sig0, th0, NUTS["num_results"], NUTS["num_burnin_steps"], seed=SEED, chain=chain,
                                            step_size=NUTS["step_size"], stale_cache=False, trace=trace, max_tree_depth=NUTS["max_tree_depth"])
        for name, field in (("leapfrogs_taken", "leapfrogs"), ("tree_depth", "depth"), ("is_accepted", "is_accepted"),
                            ("has_divergence", "has_divergence"), ("reach_max_depth", "reach_max_depth")):
            np.testing.assert_array_equal(whole[name][i], [int(getattr(r, field)) for _, r, _ in trace], err_msg=name)
        np.testing.assert_allclose(whole["target_log_prob"][i], [r.target_log_prob for _, r, _ in trace], rtol=1e-9)
        np.testing.assert_allclose(whole["X"][i], oX, rtol=0, atol=1e-8 * np.abs(oX).max())


# ---- a problem group -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per", [1, 2])
def test_group_members_with_other_demoted_sets_or_none_equal_their_own_handles(per):
    """Three members of one shape (N = 300, SEIR-4): the graded problem, the graded problem with the roles one component on (another set
    of the same size: other slots for the same indices) and a structureless density that demotes nothing -- a null narrow buffer beside two
    others.  k_stream_group<1> and <2>; every member's chains bit for bit those of its own handle."""
    from magi_v2_amd.engine import MagiGroup
    gs = [dr.graded(300, "seir4", 0), dr.graded(300, "seir4", 1)]
    assert set(gs[0].demoted) != set(gs[1].demoted) and len(gs[0].demoted) == len(gs[1].demoted)
    plain = fixture(300, "seir4", spd=True)
    members = [(g.exact, g.X) for g in gs] + [plain]
    engs = [engine_for(pr) for pr, _ in members]
    ids = [[5 + c for c in range(per)], [5 + c for c in range(per)], [40 + c for c in range(per)]]       # (ids repeat across members)
    starts = [[_inits(pr, X)[2]] * per for pr, X in members]
    grp = None
    try:
        for eng, nd in zip(engs, (len(gs[0].demoted), len(gs[1].demoted), 0)):
            assert eng.tile_formats(per)[:2] == (len(gs[0].split), nd)
        grp = MagiGroup(engs)
        assert grp.stream_kernel_name(3 * per) == f"k_stream_group<{per}>"
        got = _nuts(grp, [s for m in starts for s in m], [i for m in ids for i in m])
        own = [_nuts(eng, starts[m], ids[m]) for m, eng in enumerate(engs)]
    finally:
        if grp is not None:
            grp.close()
        for eng in engs:
            eng.close()
    assert not np.array_equal(got["X"][0], got["X"][per])        # (the same chain id in two different problems)
    for m in range(3):
        _assert_identical(got, own[m], f"member {m}, {per} chains each", slice(m * per, (m + 1) * per))


# ---- one handle, packed again and again -------------------------------------------------------------------------------------------------

def _observe(eng, g):
    out = {}
    for n in (1, 2):
        logp, gX = _fused(eng, g, list(range(n)))
        out[f"logp{n}"], out[f"gX{n}"] = logp, gX
        start = _inits(g.exact, g.X)[2]
        out.update({f"nuts{n}.{k}": v for k, v in _nuts(eng, [start] * n, range(5, 5 + n)).items()})
    return out


def test_a_handle_packed_again_equals_a_fresh_one_at_every_stage():
    """The narrow buffer only grows and the slot numbers live in the task words: 300 (19 demoted) -> 513 (82: more than before) -> 300 with
    the roles one component on (fewer, a smaller grid after a larger one) -> 300 as at first (another set at the same count) -> tile_demote
    0 (none) -> 1 (back).  At every stage the fused log posterior of one and two states and a three-transition run of one and two chains
    equal a fresh handle's bit for bit, and the format counts are the stage's own."""
    stages = [(300, 0, 1), (513, 0, 1), (300, 1, 1), (300, 0, 1), (300, 0, 0), (300, 0, 1)]
    eng = None
    try:
        for k, (N, salt, demote) in enumerate(stages):
            g = dr.graded(N, "seir4", salt)
            pr = g.exact
            if eng is None:
                eng = engine_for(pr)
            elif stages[k - 1][:2] == (N, salt):                 # the option is read at the next pack
                eng.set_option("tile_demote", demote)
                eng.pack_resident(None)
            else:
                eng.set_matrices(pr.C_inv, pr.m, pr.K_inv, bandsize=None)
                eng.set_problem(pr.mu, pr.N_ds, pr.obs_idx, pr.y, pr.beta, pr.LB, pr.drift)
            fresh = engine_for(pr, options={"tile_demote": demote})
            try:
                want_nd = len(g.demoted) if demote else 0
                for n in (1, 2):
                    assert eng.tile_formats(n) == fresh.tile_formats(n) and eng.tile_formats(n)[:2] == (len(g.split), want_nd), (k, eng.tile_formats(n))
                got, want = _observe(eng, g), _observe(fresh, g)
            finally:
                fresh.close()
            for name in want:
                np.testing.assert_array_equal(got[name], want[name], err_msg=f"stage {k} {stages[k]}: {name}")
    finally:
        if eng is not None:
            eng.close()


# ---- banded storage is left alone ------------------------------------------------------------------------------------------------------

def test_banded_fused_storage_demotes_nothing_on_the_graded_stacks():
    """N = 513 under b = 20 (6 b + 1 < N: banded fused storage, far blocks skipped): no narrow copies whatever the option says, and the
    same numbers with it on and off."""
    g = dr.graded(513, "seir4")
    out = []
    for opt in (1, 0):
        eng = _engine(g, band=20, options={"tile_demote": opt})
        try:
            assert eng.tile_formats(1)[1] == 0 and eng.tile_formats(2)[1] == 0
            out.append(_observe(eng, g))
        finally:
            eng.close()
    for name in out[0]:
        np.testing.assert_array_equal(out[0][name], out[1][name], err_msg=name)
