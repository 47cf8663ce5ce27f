"""The packing rule of the carrier workgroups (csrc/pack.hip: carriers; option stream_carriers), restated in numpy and held to its own
invariants.  A carrier is one workgroup of up to three block tasks that share a compute unit; a block weighs 2 units of 64 KB when the
VALU streaming kernels read it as fp64 and 1 when they read its fp32 copy:

  * the blocks of FH first on both sides (a carrier of FH blocks alone needs no theta'), task order otherwise;
  * [fp64 + fp32] while both kinds last;
  * then the fp64 blocks left, one per carrier (2 units), or the fp32 blocks left, three per carrier, the last one or two in the last carrier;
  * launched under stream_carriers = -1 (auto; the library's default is 0, never) where a workgroup per block needs more than one round and the carriers fit in one: 1 + carriers <= CUs < 1 + blocks.

tests/test_stream_carriers_gpu.py compares the table the library packs with carrier_table()."""
import numpy as np
import pytest

FH, FK, FE = 0, 1, 2
TB = 128


def task_list(N, D=4, far=2):
    """[(d, kind, bi, bj)] in the pack's order (dense), and which of them a Matern-like split demotes: |bi - bj| >= far (None: nothing)."""
    nb = -(-N // TB)
    tasks = [(d, k, bi, bj) for d in range(D) for k in (FH, FK, FE) for bi in range(nb) for bj in range(nb) if k == FE or bj <= bi]
    dem = [far is not None and abs(bi - bj) >= far for _, _, bi, bj in tasks]
    return tasks, dem


def carrier_table(kinds, demoted):
    """[n_carriers, 3] task indices (-1: an empty slot) and the units of every carrier."""
    kinds, demoted = np.asarray(kinds), np.asarray(demoted, dtype=bool)
    order = [t for fh in (True, False) for t in range(len(kinds)) if (kinds[t] == FH) == fh]
    w64, w32 = [t for t in order if not demoted[t]], [t for t in order if demoted[t]]
    n_pairs = min(len(w64), len(w32))
    rows = [[w64[i], w32[i], -1] for i in range(n_pairs)]
    rows += [[t, -1, -1] for t in w64[n_pairs:]]
    rest = w32[n_pairs:]
    rows += [(rest[i:i + 3] + [-1, -1])[:3] for i in range(0, len(rest), 3)]
    table = np.array(rows, dtype=int).reshape(-1, 3)
    units = np.array([sum(1 if demoted[t] else 2 for t in row if t >= 0) for row in table], dtype=int)
    return table, units


def carriers_by_auto(n_carriers, n_tasks, cus):
    return 1 + n_carriers <= cus < 1 + n_tasks


def check_table(table, units, demoted):
    """The invariants of any carrier table: every task once; at most 3 tasks and 3 units; empty slots behind the tasks of their carrier;
    carriers short of 3 units only at the end."""
    demoted = np.asarray(demoted, dtype=bool)
    used = table[table >= 0]
    assert sorted(used.tolist()) == list(range(len(demoted)))
    assert table.shape[1] == 3 and units.max() <= 3 and units.min() >= 1
    for row, u in zip(table, units):
        live = row >= 0
        assert live[0] and not (live[1:] & ~live[:-1]).any()     # no task behind an empty slot
        assert u == sum(1 if demoted[t] else 2 for t in row[live])
    short = np.nonzero(units < 3)[0]
    assert short.size == 0 or short[0] == len(units) - short.size      # a suffix
    assert units.sum() == 2 * (~demoted).sum() + demoted.sum()


@pytest.mark.parametrize("N,far,n_tasks,n_dem,n_carriers,on", [
    (300, 2, 84, 16, 68, False),          # three block rows: 16 pairs + 52 fp64 blocks alone; one round either way
    (384, None, 84, 0, 84, False),        # nothing demoted: a carrier per block
    (513, 2, 220, 96, 124, False),        # 96 pairs + 28 fp64 blocks alone; 221 workgroups are one round already
    (1024, 2, 544, 336, 251, True),       # 208 pairs, 128 fp32 blocks left: 42 triples + one carrier of two
    (1024, None, 544, 0, 544, False),     # option tile_demote = 0 at the production shape: more carriers than CUs
])
def test_the_rule_at_the_task_counts_of_the_test_shapes(N, far, n_tasks, n_dem, n_carriers, on):
    tasks, dem = task_list(N, far=far)
    assert (len(tasks), sum(dem)) == (n_tasks, n_dem)
    table, units = carrier_table([t[1] for t in tasks], dem)
    check_table(table, units, dem)
    assert len(table) == n_carriers
    assert carriers_by_auto(len(table), n_tasks, 256) == on
    if N == 1024 and far:
        assert units.tolist() == [3] * 250 + [2] and units.sum() == 752
        # the 60 kept blocks of FH meet demoted blocks of FH: those carriers derive no theta'
        kinds = np.array([t[1] for t in tasks])
        all_fh = [(kinds[row[row >= 0]] == FH).all() for row in table]
        assert sum(all_fh) == 60 and all(all_fh[:60])


@pytest.mark.parametrize("n64,n32", [(0, 4), (0, 5), (0, 6), (1, 9), (2, 5), (3, 4), (5, 5), (7, 2), (1, 0), (0, 1)])
def test_what_finds_no_partner_goes_last(n64, n32):
    """fp32 blocks left over: 1, 2 and 0 modulo 3; fp64 blocks left over; neither."""
    rng = np.random.default_rng([22, n64, n32])
    dem = rng.permutation([False] * n64 + [True] * n32)
    kinds = rng.integers(0, 3, size=n64 + n32)
    table, units = carrier_table(kinds, dem)
    check_table(table, units, dem)
    pairs, rest32 = min(n64, n32), max(n32 - n64, 0)
    assert len(table) == pairs + (n64 - pairs) + -(-rest32 // 3)
    if rest32 % 3:
        assert units[-1] == rest32 % 3


def test_auto_eligibility_is_one_round_instead_of_several():
    assert carriers_by_auto(251, 544, 256) and carriers_by_auto(255, 256, 256)
    assert not carriers_by_auto(256, 544, 256)                # carriers + the decision workgroup do not fit
    assert not carriers_by_auto(100, 255, 256)                # a workgroup per block is one round already
    assert carriers_by_auto(251, 544, 304) and carriers_by_auto(251, 544, 252)      # two rounds become one; exactly full
    assert not carriers_by_auto(251, 544, 640)                # a device with a CU per block
