"""What keeps tests/test_reuse_gpu.py honest, on the CPU oracle alone (case tables: tests/util.py, "one handle through many states").

That file moves ONE handle through a history of states and holds it to a fresh handle bit for bit; a handle that answered for the state it
was in BEFORE the transition (a graph, a tile, a product slot, an operand mirror, a problem constant left over) must therefore differ from
the fresh one.  Here:

  * for every pair of consecutive states of every history the oracle's log posterior AND its X-gradient of the later state differ from the
    earlier state's, evaluated at the later state's inputs, by >= 1e-6 of scale -- 1000 x the loosest bar of the GPU comparisons (1e-9
    fused; the three-phase bar 1e-10 asks for 1e-7).  Pairs that differ in N or D have no common input: their state vectors have other
    lengths, asserted as such.  A pair that differs in P only (sirw <-> seir4 on one set of D = 4 matrices) is evaluated at the later
    state's X and sigma with each problem's own theta.  This is a condition on the fixtures (seeds and bands are picked so that it holds),
    not a measurement of the kernels.  Smallest margin found: 6.4e-4 (a group member's data, C41 -> C41*; bands >= 1.9e-2, data and drift >= 0.23, times 0.67);
  * the states of a batch are pairwise >= 1e-6 apart in the same sense (smallest: 3.5e-3): a chain that read another chain's operands shows;
  * the times of test 10 move value and gradient by > 1e-3 (the one margin that is relative to the value itself);
  * the block counts of magi_gradient_bytes: the band tables restated from the comments of csrc/pack.hip agree with an independent numpy
    count of the blocks the mask leaves an entry in -- wherever equality is claimed; at b = 0 the library keeps the empty neighbours
    (wb = 1) and only "none missing" holds;
  * every history passes through the storage modes and kernel families it names (the auto rule as tests/conftest.py documents it)."""
import numpy as np
import pytest

from tests.util import (REUSE_BANDS, REUSE_BATCHES, REUSE_BYTES, REUSE_DATA, REUSE_N, REUSE_SHAPES, reuse_auto_kernel, reuse_band_state,
                        reuse_band_tables, reuse_block_counts, reuse_oracle_logpost, reuse_state)

HISTORIES = {"bands": [reuse_band_state(b).name for b in REUSE_BANDS], "shapes": list(REUSE_SHAPES), "data": list(REUSE_DATA),
             "group member": ["C41", "C41*"], "times": ["T", "T+0.37"]}
MARGIN = 1e-6
N_STATES = 5


def _gap(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def _pair_margin(prev, nxt):
    """Smallest of (value gap, X-gradient gap) over the first N_STATES inputs of the later state; None when the shapes differ."""
    if (prev.pr.D, len(prev.pr.I)) != (nxt.pr.D, len(nxt.pr.I)):
        assert prev.batch[0].shape[1:] != nxt.batch[0].shape[1:]
        return None
    X, sp, tp = nxt.states(N_STATES)
    tp_prev = tp if prev.pr.P == nxt.pr.P else prev.states(N_STATES)[2]
    worst = np.inf
    for c in range(N_STATES):
        new = reuse_oracle_logpost(nxt, X[c], sp[c], tp[c], 0.8)
        old = reuse_oracle_logpost(prev, X[c], sp[c], tp_prev[c], 0.8)
        worst = min(worst, abs(old[0] - new[0]) / abs(new[0]), _gap(old[1], new[1]))
    return worst


@pytest.mark.parametrize("history", sorted(HISTORIES))
def test_a_stale_answer_would_be_seen_after_every_transition(history):
    names = HISTORIES[history]
    margins = {}
    for a, b in zip(names[:-1], names[1:]):
        m = _pair_margin(reuse_state(a), reuse_state(b))
        if m is not None:
            margins[f"{a} -> {b}"] = m
    print(f"sensitivity of '{history}':", {k: f"{v:.3g}" for k, v in margins.items()})
    assert margins or history == "shapes"
    for pair, m in margins.items():
        assert m >= MARGIN, (pair, m)
    if history == "times":
        assert min(margins.values()) > 1e-3, margins


def test_the_states_of_a_batch_are_pairwise_apart():
    """Transition 4 keeps the problem and changes the batch: what could be stale is another chain's operands."""
    st = reuse_state("A")
    X, sp, tp = st.batch
    out = [reuse_oracle_logpost(st, X[c], sp[c], tp[c], 0.8) for c in range(len(X))]
    worst = min(min(abs(out[a][0] - out[b][0]) / abs(out[b][0]), _gap(out[a][1], out[b][1])) for a in range(len(out)) for b in range(a))
    print(f"smallest distance of two states of the batch: {worst:.3g}")
    assert worst >= MARGIN, worst


def test_a_stale_output_row_would_be_seen_under_a_capacity_larger_than_the_need():
    """The grow-only history of tests/test_reuse_gpu.py: a NUTS run of 3 chains x (8 + 6) transitions to its end, then REUSE_NUTS on 2 chains
    paused after 3 of its 4 + 3 -- the output buffers keep the first run's capacity, and the second run's rows lie over the first's.  The
    diagnostics are [chain][total]: entry f of the second run (chain f // 7, transition f % 7) lies where the first run left chain 0's
    transition f.  On the oracle: wherever the second run has a value of its own there, the first run's differs by >= MARGIN in step size,
    energy and target (the log acceptance ratio is 0 and -inf in the first two transitions of this configuration and has no scale);
    everywhere else the second run expects the NaN fill over a finite number, and its sample rows (no transition behind burn-in taken) the
    fill over the first run's draws.  The one exception is by construction: chain 0's transitions 0 .. 2 are the same chain from the same
    state under the same seed in both runs, while both still adapt -- equal, asserted as such: a stale entry there IS the right entry.
    Smallest margin found: 0.124."""
    from tests import metric_reference as M
    from tests.util import REUSE_GROW, REUSE_NUTS, REUSE_SEED
    st = reuse_state("C41")
    X, sp, tp = st.states(3)
    floats = ("step_size", "energy", "target_log_prob")

    def run(cfg, chain):
        kw = {k: v for k, v in cfg.items() if k not in ("num_results", "num_burnin_steps", "stale_cache")}
        out = M.sample_chain(st.pr, None, None, None, cfg["num_results"], cfg["num_burnin_steps"], seed=REUSE_SEED, chain=20 + chain,
                             initial=(X[chain], sp[chain], tp[chain]), stale_cache=bool(cfg["stale_cache"]), **kw)
        return out[0], out[4]["all"]

    draws, first = run(REUSE_GROW, 0)                           # (what lies under the second run's 2 x 7 entries is chain 0's alone)
    assert np.isfinite(draws).all() and all(np.isfinite(first[k]).all() and len(first[k]) == 14 for k in floats)
    total, taken = REUSE_NUTS["num_burnin_steps"] + REUSE_NUTS["num_results"], 3
    assert taken < REUSE_NUTS["num_burnin_steps"]                # no draw of the second run is stored: its sample rows are all fill
    worst = np.inf
    for c in range(2):
        second = run(REUSE_NUTS, c)[1]
        for k in range(taken):
            gaps = [abs(first[f][c * total + k] - second[f][k]) / abs(second[f][k]) for f in floats]
            if c == 0:
                assert max(gaps) == 0.0, (k, gaps)
            else:
                worst = min(worst, min(gaps))
    print(f"smallest margin of a stale diagnostics entry: {worst:.3g}")
    assert worst >= MARGIN, worst


@pytest.mark.parametrize("name,band", REUSE_BYTES)
def test_block_counts_of_the_band_tables_against_the_masked_index_sets(name, band):
    pr = reuse_state(name).pr
    N, D = len(pr.I), pr.D
    independent, library = reuse_block_counts(N, D, band)
    expected = {("A", None): (84, 84), ("A", 20): (68, 68), ("A", 43): (84, 84), ("A", 0): (36, 68), ("C161", 20): (30, 30)}[(name, band)]
    assert (independent, library) == expected
    if band != 0:
        assert independent == library
    else:
        assert independent < library                                     # wb = 1 keeps off-diagonal blocks the diagonal mask empties


def test_the_band_history_passes_through_the_storage_modes_it_names():
    got = [reuse_band_tables(REUSE_N, b) for b in REUSE_BANDS]
    # (three-phase banded?, W, fb, wb, nb): dense; 20: banded rows, fb = 60, far blocks skipped; 0: one column; 43: 6 b + 1 = 259 < 384,
    # fb = 129, wb = 2 -- the far blocks return; dense again (mat_elems reallocates at every step); 20
    assert got == [(False, 384, -1, 3, 3), (True, 41, 60, 1, 3), (True, 1, 0, 1, 3), (True, 87, 129, 2, 3), (False, 384, -1, 3, 3), (True, 41, 60, 1, 3)]
    assert len({(banded, W) for banded, W, *_ in got}) == 4 and all(a[:2] != b[:2] for a, b in zip(got[:-1], got[1:]))
    # the (2, 0) block: no entry within fb = 60 of the diagonal, one (i = 256, j = 127) within 129
    assert 2 * 128 - 127 > 60 and 2 * 128 - 127 <= 129


def test_the_batch_history_passes_through_the_kernel_families_it_names():
    n_tasks = reuse_block_counts(REUSE_N, 4, None)[1]
    assert n_tasks == 84
    names = [reuse_auto_kernel(n_tasks, n, fam) for n, fam, _ in REUSE_BATCHES]
    assert names == [k for _, _, k in REUSE_BATCHES]
    assert names == ["k_stream_sep<CW=16>", "k_stream<2>", "k_stream_sep<CW=16>", "k_stream_sep<CW=8>", "k_stream<1>", "k_stream_sep<CW=8>",
                     "k_stream_sep<CW=16>"]
    assert all(a != b for a, b in zip(names[:-1], names[1:]))            # every step changes the kernel
    # "auto" alone would leave 3 chains on the VALU kernel (84 x 2 <= 320) and takes 8 to the 8-column mirror (84 x 4 > 320)
    assert reuse_auto_kernel(n_tasks, 3, "auto") == "k_stream<2>" and reuse_auto_kernel(n_tasks, 8, "auto") == "k_stream_sep<CW=8>"
    assert [n for n, _, _ in REUSE_BATCHES][-1] % 16 == 1               # a ragged second group of the 16-column mirror
    # the other histories: one chain on k_stream<1>, five on k_stream<2> under "auto" (84 x 3 <= 320) and on the 8-column mirror under "mc"
    # -- the band history runs its five states both ways
    assert reuse_auto_kernel(84, 5, "auto") == "k_stream<2>" and reuse_auto_kernel(68, 5, "auto") == "k_stream<2>"
    assert reuse_auto_kernel(68, 5, "mc") == "k_stream_sep<CW=8>" and reuse_auto_kernel(84, 1, "mc") == "k_stream_sep<CW=8>"
    assert reuse_auto_kernel(reuse_block_counts(41, 4, None)[1], 5, "auto") == "k_stream<2>"
