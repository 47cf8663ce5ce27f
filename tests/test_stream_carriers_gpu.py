"""Carrier workgroups of the VALU streaming kernels (csrc/pack.hip: carriers; leap_stream_body.h: CARR; option stream_carriers): three block
tasks side by side in one 768-thread workgroup per compute unit, filled by bytes.  The launch shape changes no arithmetic: every comparison
here is bit for bit, option 1 (carriers wherever a CU holds exactly one) against 0 (a workgroup per block) on the SAME handle and problem --
the option is read at the next pack --, at the smallest shapes that reach every edge: the graded fixture of tests/demote_reference.py
(N = 300: three block rows, ragged, kept and demoted blocks interleaved; N = 513: five block rows, the last block one wide), banded fused
storage (no demoted block: a carrier per block, two empty slots each), a per-drift build, the benchmark's problem at N = 512.  The table the
library packs is the one tests/test_stream_carriers_cpu.py restates."""
import numpy as np
import pytest

from tests import demote_reference as dr
from tests.test_demote_edges_gpu import _compute_units, _engine, _fused
from tests.test_stream_carriers_cpu import carrier_table, carriers_by_auto, check_table
from tests.test_structureless_cpu import fixture
from tests.test_tile_demote_gpu import BLOCK_BYTES, _assert_runs_identical, _seir_engine, _short_run, _small_engine
from tests.util import engine_for

pytestmark = pytest.mark.gpu


def _pack(eng, value, band=None):
    """The option, a new pack of the resident stacks under it, the carriers it made."""
    eng.set_option("stream_carriers", value)
    eng.pack_resident(band)
    return eng.stream_carriers()


def _expect_table(eng, info):
    """(table, units) of the pack, with every block in exactly one slot and the units of its formats."""
    nb, nd, _ = eng.tile_formats(1)
    table, units = info["tasks"], info["units"]
    assert table.shape == (len(units), 3)
    used = table[table >= 0]
    assert sorted(used.tolist()) == list(range(nb))              # every task exactly once
    assert units.sum() == 2 * (nb - nd) + nd
    return table, units


# ---- the fused log posterior and its gradient ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,drift,band", [(300, "seir4", None), (513, "seir4", None), (300, "ptrans", None), (300, "seir4", 40)])
def test_fused_log_posterior_is_bit_identical_in_carriers(N, drift, band):
    """k_stream<1> on every state, k_stream<2> on every state in either half of a pair, even and odd slot (_fused evaluates both and
    holds them equal); "ptrans" runs the per-drift build of a traced drift; b = 40 at N = 300 is banded fused storage."""
    g = dr.graded(N, drift)
    eng = _engine(g, band)
    out = {}
    try:
        assert eng.stream_kernel_name(1) == "k_stream<1>" and eng.stream_kernel_name(2) == "k_stream<2>"
        formats = eng.tile_formats(1)
        for value in (0, 1, 0):                                  # (and back: the table and the launch follow the pack, not the handle's history)
            info = _pack(eng, value, band)
            assert info["on"] == bool(value)
            assert eng.tile_formats(1) == formats and eng.stream_kernel_name(1) == "k_stream<1>"
            res = [_fused(eng, g, [j]) for j in range(g.nb)] + [_fused(eng, g, [j, (j + 1) % g.nb]) for j in range(g.nb)]
            if value in out:
                for (la, ga), (lb, gb) in zip(out[value], res):
                    np.testing.assert_array_equal(la, lb)
                    np.testing.assert_array_equal(ga, gb)
            out[value] = res
            print(f"N={N} {drift} b={band} stream_carriers={value}: {len(info['units'])} carriers, units "
                  + ", ".join(f"{u}x{(info['units'] == u).sum()}" for u in np.unique(info["units"])))
    finally:
        eng.close()
    for k, ((l0, g0), (l1, g1)) in enumerate(zip(out[0], out[1])):
        np.testing.assert_array_equal(l0, l1, err_msg=f"evaluation {k}: log posterior")
        np.testing.assert_array_equal(g0, g1, err_msg=f"evaluation {k}: gradient")


def test_benchmark_problem_at_n512_is_bit_identical_in_carriers():
    """SEIR-4 on Matern operators, N = 512 (144 blocks, 48 demoted): the fused log posterior of one and two states in both slot parities; a
    chain of 3 transitions; a pause under one setting resumed under the other, both ways (the checkpoint tag does not know the option)."""
    eng, state = _seir_engine(512)
    rep = lambda v, n: np.repeat(np.asarray(v)[None], n, axis=0)
    try:
        fused, runs, cks = {}, {}, {}
        cfg = eng.default_cfg(num_results=2, num_burnin_steps=1, step_size=1e-3, max_tree_depth=4, stale_cache=0)
        for value in (0, 1):
            info = _pack(eng, value)
            assert info["on"] == bool(value) and eng.tile_formats(1) == (144, 48, (144 - 48) * BLOCK_BYTES + 48 * BLOCK_BYTES / 2)
            res = []
            for parity in (0, 1):
                eng.set_option("fused_parity", parity)
                res.append(eng.logpost_grad(*state, 1.0, fused=True))
                res.append(eng.logpost_grad(*[rep(v, 2) for v in state], 1.0, fused=True))
            eng.set_option("fused_parity", 0)
            fused[value] = res
            runs[value] = _short_run(eng, state, 1)
            eng.sampler_init(cfg, *[rep(v, 1) for v in state], seed=77, chain_ids=[5])
            eng.sampler_run(1)
            cks[value] = eng.sampler_checkpoint()
        for a, b in zip(fused[0], fused[1]):
            for x, y in zip(a, b):
                np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
        _assert_runs_identical(runs[0], runs[1], "N=512, a workgroup per block against carriers")
        for key in cks[0]:
            np.testing.assert_array_equal(cks[0][key], cks[1][key], err_msg=f"checkpoint after one transition: {key}")
        for written, resumed in ((0, 1), (1, 0)):                # (the handle is under setting 1 after the loop)
            if eng.stream_carriers()["on"] != bool(resumed):
                _pack(eng, resumed)
            eng.sampler_resume(cfg, cks[written], seed=77, chain_ids=[5])
            eng.sampler_run(2)
            np.testing.assert_array_equal(eng.sampler_samples()[0], runs[0][0], err_msg=f"paused under {written}, resumed under {resumed}")
    finally:
        eng.close()


@pytest.mark.parametrize("chains", [1, 2])
def test_deep_trees_decide_alike_in_a_carrier_launch(chains):
    """From its 32nd leaf on a tree's U-turn checks add dot products over the whole state in the decision workgroup (decide.h: kk >= 5),
    strided over the workgroup's threads and summed per wave -- the one piece of decision code that sees the 768 threads of a carrier launch
    (it runs on the first 256).  N = 512, trees capped at depth 6 with a step small enough to fill them: 63 leaves, bit for bit."""
    eng, state = _seir_engine(512)
    try:
        runs = {}
        for value in (0, 1):
            assert _pack(eng, value)["on"] == bool(value)
            runs[value] = _short_run(eng, state, chains, depth=6)
            assert runs[value][3][0].max() >= 32                 # leapfrogs_taken: the deep checks ran
        _assert_runs_identical(runs[0], runs[1], f"N=512, depth 6, {chains} chains")
    finally:
        eng.close()


# ---- the table ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [300, 513])
def test_carrier_table_is_the_packing_rule(N):
    g = dr.graded(N, "seir4")
    eng = _engine(g)
    try:
        info = _pack(eng, 1)
        table, units = _expect_table(eng, info)
        # the pack's task order at these shapes is (d, kind, bi, bj) ascending (no launch of three rounds): the split's order
        kinds = [k for _, k, _, _, _, _ in g.split]
        dem = [bool(ok) for _, _, _, _, ok, _ in g.split]
        check_table(table, units, dem)
        want_table, want_units = carrier_table(kinds, dem)
        np.testing.assert_array_equal(table, want_table)
        np.testing.assert_array_equal(units, want_units)
        auto = _pack(eng, -1)
        assert not auto["on"]                                    # one round already
        np.testing.assert_array_equal(auto["tasks"], table)      # (the table is there to be read either way)
    finally:
        eng.close()


def test_with_every_block_kept_auto_resolves_to_off():
    """The structureless fixture at N = 384: nothing demoted, a carrier per block (2 units each); auto launches none."""
    pr, _ = fixture(384, "seir4", spd=True)
    eng = engine_for(pr, options={"stream_carriers": -1})
    try:
        info = eng.stream_carriers()
        assert eng.tile_formats(1)[:2] == (84, 0)
        assert not info["on"] and info["units"].tolist() == [2] * 84 and (info["tasks"][:, 1:] == -1).all()
        assert not carriers_by_auto(84, 84, _compute_units() or 256)
    finally:
        eng.close()


def test_production_shape_runs_in_one_round_of_full_carriers():
    """N = 1024 on a 256-CU device: the library's default is a workgroup per block (carriers measured slower: profiles/r22_carriers_ab.txt);
    stream_carriers = -1 resolves to carriers -- 250 of 3 units and the last of 2 (752 units do not divide by 3) +
    the decision workgroup = 252 workgroups, one round, 192 KB per CU -- with the pinned formats, bytes and kernel names; and one fused
    evaluation is bit-identical to the 256-thread launch of 545 workgroups."""
    if _compute_units() != 256:
        pytest.skip("the carrier count is pinned for a 256-CU device")
    eng, state = _seir_engine(1024)
    try:
        assert not eng.stream_carriers()["on"]
        info = _pack(eng, -1)
        table, units = _expect_table(eng, info)
        assert info["on"] and units.tolist() == [3] * 250 + [2]
        assert eng.tile_formats(1) == (544, 336, (544 - 336) * BLOCK_BYTES + 336 * BLOCK_BYTES / 2)
        assert eng.gradient_bytes(1)[4] == eng.tile_formats(1)[2] + 2 * 128 * 8 * 544
        assert eng.stream_kernel_name(1) == "k_stream<1>" and eng.stream_kernel_name(2) == "k_stream<2>"
        on = eng.logpost_grad(*state, 1.0, fused=True)
        assert not _pack(eng, 0)["on"]
        off = eng.logpost_grad(*state, 1.0, fused=True)
        for a, b in zip(on, off):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    finally:
        eng.close()


# ---- small grids -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chains", [1, 8])
def test_small_grid_resolves_to_off_and_runs_the_parent_path(chains):
    """N = 161, b = 80 (40 blocks: every block has a CU of its own): auto launches no carriers and the chains are those of option 0."""
    runs = []
    for value in (-1, 0):
        eng, state = _small_engine(161, 80, {"stream_carriers": value})
        try:
            assert not eng.stream_carriers()["on"] and eng.stream_kernel_name(chains).startswith("k_stream<")
            runs.append(_short_run(eng, state, chains, deep=False))
        finally:
            eng.close()
    _assert_runs_identical(*runs, f"N=161 b=80, {chains} chains")
