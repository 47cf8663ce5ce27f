"""The conditions of the graded fixture (tests/demote_reference.py), on the oracle alone.  tests/test_demote_edges_gpu.py compares the kernels
that read certified fp32 operator blocks with the oracle on that fixture; what is proved here is that those comparisons can fail:

  * the split is mixed -- demoted and kept blocks in one block row of one operator, a demoted first neighbour, FH kept beside a demoted FK --
    and has no knife-edge: every ratio is a factor 2 from the threshold, so device sums and numpy sums decide alike;
  * the `rounded` problem's stacks give the operators with exactly the demoted blocks rounded to fp32, bit for bit;
  * EVERY demoted block is visible: zeroed, transposed in place or swapped with another demoted block (the other operator of the same
    indices, the same block of another component, the neighbouring slot) it moves the gradient on a compared set of some state by
    >= 1000 x the bar applied there (VALU readers: 1e-12 of the set's largest entry; matrix-core readers: 2 sum_bound entrywise);
  * the rounding is visible: on every state a compared set has |g_rounded - g_exact| >= 10 x the bar, so a reader of unrounded doubles fails;
  * the reference is good enough: the fp64 oracle against its longdouble evaluation sits >= 100 x below every bar;
  * C^-1 and K^-1 are positive definite.

These are conditions of the fixture, not measurements of a kernel: where one fails, the fixture changes (its scales, its states), not the factor."""
import numpy as np
import pytest

from oracle import magi_oracle as orc
from tests import demote_reference as dr
from tests.test_structureless_cpu import _longdouble, logpost_grad_longdouble
from tests.test_tile_demote_cpu import RATIO, fused_operators

# (N, drift) of every comparison with the oracle in tests/test_demote_edges_gpu.py
CASES = [(300, "seir4"), (513, "seir4"), (1024, "seir4"), (300, "ptrans"), (300, "seir_seasonal"), (513, "ptrans"), (513, "seir_seasonal")]
# (N, drift, salt): the second member of the group and the stages of the re-packed handle (compared with a fresh handle, not the oracle)
ROTATED = [(300, "seir4", 1)]
VISIBLE, ROUNDING_VISIBLE, FLOOR = 1000.0, 10.0, 100.0


@pytest.mark.parametrize("N,drift,salt", [c + (0,) for c in CASES] + ROTATED)
def test_the_split_is_mixed_and_has_no_knife_edge(N, drift, salt):
    g = dr.graded(N, drift, salt)
    off = [b for b in g.split if b[2] != b[3]]
    dem, kept = [b for b in off if b[4]], [b for b in off if not b[4]]
    worst, smallest = max(b[5] for b in dem), min(b[5] for b in kept)
    print(f"N={N} {drift} salt {salt}: roles {g.roles}; {len(dem)} of {len(g.split)} stored blocks demoted, per component "
          f"{[sum(1 for b in dem if b[0] == d) for d in range(g.D)]}; worst passing ratio / 2^-29 {worst / RATIO:.3g}, smallest failing {smallest / RATIO:.3g}")
    assert worst <= RATIO / 2 and smallest >= 2 * RATIO
    rows_dem, rows_kept = {b[:3] for b in dem}, {b[:3] for b in kept}
    assert rows_dem & rows_kept                                  # (d, kind, bi): one block row of one operator holds both
    assert any(abs(b[2] - b[3]) == 1 for b in dem)
    demoted = set(g.demoted)
    assert any((d, dr.FH, bi, bj) not in demoted for d, k, bi, bj in g.demoted if k == dr.FK)
    for d in range(g.D):                                         # FK (bi, bj) is demoted exactly when FE (bi, bj) and FE (bj, bi) are
        for bi in range(g.nb):
            for bj in range(bi):
                assert ((d, dr.FK, bi, bj) in demoted) == ((d, dr.FE, bi, bj) in demoted) == ((d, dr.FE, bj, bi) in demoted)


@pytest.mark.parametrize("N,drift,salt", [c + (0,) for c in CASES] + ROTATED)
def test_the_rounded_stacks_reproduce_the_target_operators_bit_for_bit(N, drift, salt):
    g = dr.graded(N, drift, salt)
    got = fused_operators(g.rounded.C_inv, g.rounded.m, g.rounded.K_inv)
    demoted = set(g.demoted)
    for have, want in zip(got, g.target):
        np.testing.assert_array_equal(have, want)
    for d, k, bi, bj, _, _ in g.split:                            # ... which are the exact operators with the demoted blocks, and only those, rounded
        B = dr.stored_block(g, g.ops, (d, k, bi, bj))
        np.testing.assert_array_equal(dr.stored_block(g, g.target, (d, k, bi, bj)), dr.r32(B) if (d, k, bi, bj) in demoted else B)
    assert any(not np.array_equal(dr.stored_block(g, g.target, key), dr.stored_block(g, g.ops, key)) for key in g.demoted)
    for A in (g.exact.C_inv, g.exact.K_inv, g.rounded.C_inv, g.rounded.K_inv):
        assert np.array_equal(A, np.transpose(A, (0, 2, 1)))
    eig = [float(np.linalg.eigvalsh(A).min()) for A in (g.exact.C_inv, g.exact.K_inv, g.rounded.C_inv, g.rounded.K_inv)]
    print(f"N={N} {drift}: smallest eigenvalues of C^-1, K^-1 (exact, rounded) {eig}")
    assert min(eig) >= 0.5
    s = g.s                                                      # FE is neither FK nor the transpose of its mirror
    d, _, bi, bj = next(k for k in g.demoted if k[1] == dr.FE)
    assert not np.array_equal(dr.stored_block(g, g.target, (d, dr.FE, bi, bj)), dr.stored_block(g, g.target, (d, dr.FE, bj, bi)).T)
    assert set(np.unique(np.abs(s))) == {0.5, 1.0, 2.0}


def _moves(g, refs, changes):
    """(largest move / VALU bar, largest move / matrix-core bar) of a perturbation over the compared sets of every state."""
    valu = mc = 0.0
    for st, ref in zip(g.states, refs):
        dg = dr.delta_gX(g, st.X, changes)
        if not dg.any():
            continue
        for _, (d, r, b) in dr.set_views(g, st, dg, ref.gX, ref.bound):
            valu = max(valu, np.abs(d).max() / (dr.VALU_BAR * np.abs(r).max()))
            mc = max(mc, (np.abs(d) / (2.0 * b)).max())
    return valu, mc


@pytest.mark.parametrize("N,drift", CASES)
def test_every_demoted_block_is_visible_to_both_bars(N, drift):
    g, refs = dr.graded(N, drift), dr.references(N, drift)
    worst = {}
    for key in g.demoted:
        names = set()
        for name, changes in dr.perturbations(g, key):
            valu, mc = _moves(g, refs, changes)
            kind = name[:4]
            names.add(kind)
            worst[kind] = min(worst.get(kind, np.inf), valu, mc)
            assert valu >= VISIBLE and mc >= VISIBLE, (key, name, valu, mc)
        assert names == {"zero", "tran", "swap"}, (key, names)
    print(f"N={N} {drift}: {len(g.demoted)} demoted blocks; smallest move / bar over both bars: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))


def test_the_swap_partners_cover_the_other_operator_and_another_component():
    g = dr.graded(300, "seir4")
    near = next(d for d, r in enumerate(g.roles) if r.startswith("near"))
    plain = g.roles.index("plain")
    assert (near, dr.FE, 2, 0) in dr.swap_partners(g, (near, dr.FK, 2, 0)) and (near, dr.FK, 2, 0) in dr.swap_partners(g, (near, dr.FE, 2, 0))
    assert (plain, dr.FE, 0, 2) in dr.swap_partners(g, (near, dr.FE, 0, 2))
    for key in g.demoted:
        assert key not in dr.swap_partners(g, key) and set(dr.swap_partners(g, key)) <= set(g.demoted)


def test_the_operator_form_of_the_gradient_is_the_oracle_s():
    """delta_gX (the sensitivity above) is linear in operator_gX; operator_gX is orc.logpost_grad's gX to rounding."""
    g, refs = dr.graded(300, "ptrans"), dr.references(300, "ptrans")
    for st, ref in zip(g.states, refs):
        got = dr.operator_gX(g, g.target, st.X)
        for _, (a, b) in dr.set_views(g, st, got, ref.gX):
            assert np.abs(a - b).max() <= 1e-14 * np.abs(b).max()
    key = g.demoted[0]
    name, changes = dr.perturbations(g, key)[1]
    ops = [A.copy() for A in g.target]
    for d, kind, bi, bj, dB in changes:
        ops[kind][d, g.blocks[bi], g.blocks[bj]] += dB
        if kind != dr.FE:
            ops[kind][d, g.blocks[bj], g.blocks[bi]] += dB.T
    st = g.states[key[3]]
    full, delta = dr.operator_gX(g, ops, st.X) - dr.operator_gX(g, g.target, st.X), dr.delta_gX(g, st.X, changes)
    hit = np.abs(delta) > 0
    assert hit.any() and np.abs(full - delta)[hit].max() <= 1e-3 * np.abs(delta).max()


@pytest.mark.parametrize("N,drift", CASES)
def test_the_rounding_is_visible_on_every_state(N, drift):
    g, refs = dr.graded(N, drift), dr.references(N, drift)
    worst_valu = worst_mc = np.inf
    for st, ref in zip(g.states, refs):
        assert st.sets
        valu = mc = 0.0
        for _, (r, e, b, rb) in dr.set_views(g, st, ref.gX, ref.gX_exact, ref.bound, ref.rounding):
            gap = np.abs(r - e)
            assert (gap <= rb + dr.VALU_BAR * np.abs(r).max()).all()                 # (and inside its a-priori bound)
            valu = max(valu, gap.max() / (dr.VALU_BAR * np.abs(r).max()))
            mc = max(mc, (gap / (2.0 * b)).max())
        assert valu >= ROUNDING_VISIBLE and mc >= ROUNDING_VISIBLE, (st.name, valu, mc)
        worst_valu, worst_mc = min(worst_valu, valu), min(worst_mc, mc)
    print(f"N={N} {drift}: |g_rounded - g_exact| / bar, smallest over the states of the largest over their sets: VALU {worst_valu:.3g}, matrix-core {worst_mc:.3g}")


@pytest.mark.parametrize("N,drift", CASES)
def test_the_fp64_oracle_sits_below_every_bar(N, drift):
    g, refs = dr.graded(N, drift), dr.references(N, drift)
    pr_ld = _longdouble(g.rounded)
    floor_valu = floor_mc = floor_value = 0.0
    for st, ref in zip(g.states, refs):
        with dr.registered(g):
            lp, gX, _, _ = logpost_grad_longdouble(st.X, g.sp, g.tp, 1.0, pr_ld)
        floor_value = max(floor_value, abs(float(ref.logp - lp) / float(lp)))
        for _, (have, want, b) in dr.set_views(g, st, ref.gX, np.asarray(gX, dtype=np.longdouble), ref.bound):
            gap = np.abs(have - want).astype(np.float64)
            floor_valu = max(floor_valu, gap.max() / (dr.VALU_BAR * np.abs(have).max()))
            floor_mc = max(floor_mc, (gap / (2.0 * b)).max())
    print(f"N={N} {drift}: fp64 oracle against longdouble, as a fraction of the bar: VALU {floor_valu:.3g}, matrix-core {floor_mc:.3g}; "
          f"value {floor_value:.3g} (bar 1e-12)")
    assert floor_valu <= 1.0 / FLOOR and floor_mc <= 1.0 / FLOOR and floor_value <= 1e-12 / FLOOR
