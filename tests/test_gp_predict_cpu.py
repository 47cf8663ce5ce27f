"""What the GPU tests of the GP conditioning (tests/test_gp_predict_gpu.py) rest on, proved without a GPU on tests/gp_reference.py:
the derived bar is wide enough for float64 and narrow enough to see a wrong block, a transposed operand, a wrong row; exact grid
times reproduce the draw and m (x - mu); the unclamped variance stays inside its bar; the cross blocks are the oracle's blocks.

Fixtures: N in {129, 300} on tests.util.shuffled_grid (seed 7, spacing 0.025: on the sorted grid the far blocks of Kappa^-1 would not
count), phi in {(0.7, 0.3), (0.2, 0.15)}, C^-1 = inv(Kappa) from the oracle's accurate columns, T = 130 times (127 uniform in
[min I - 0.1, max I + 0.1] plus three exact grid times), S = 5 smooth-plus-noise draws."""
import numpy as np
import pytest

from oracle import magi_oracle as orc
from tests import gp_reference as gpr
from tests.util import shuffled_grid

U = 2.0 ** -53
MU = 0.35
CASES = [(N, phi) for N in (129, 300) for phi in ((0.7, 0.3), (0.2, 0.15))]


class Fixture:
    def __init__(self, N, phi):
        Is, perm = shuffled_grid(N, 7)
        self.N, (self.phi1, self.phi2) = N, phi
        self.I = Is[perm]
        self.t_new, self.grid_idx = gpr.new_times(self.I)
        self.Kappa, self.pKappa, _ = orc.matern_block_columns_accurate(self.I, np.arange(N), self.phi1, self.phi2)
        self.C_inv = np.linalg.inv(self.Kappa)
        self.cond = np.linalg.cond(self.Kappa)
        self.Ks, self.pKs = gpr.cross_blocks(self.I, self.t_new, self.phi1, self.phi2)
        self.X = gpr.smooth_draws(self.I, 5, 1, [MU], seed=11)[:, :, 0]           # [S, N]
        self.dpp = gpr.diag_pp(self.phi1, self.phi2)
        self.bars = gpr.bars_component(self.Ks, self.pKs, self.C_inv, self.X, MU, self.phi1, self.dpp)

    def run(self, C_inv=None, dtype=np.longdouble):
        return gpr.predict_component(self.Ks, self.pKs, self.C_inv if C_inv is None else C_inv, self.X, MU, self.phi1, self.dpp, dtype)


_cache = {}


@pytest.fixture(params=CASES, ids=lambda c: f"N{c[0]}-phi{c[1][0]}-{c[1][1]}")
def fx(request):
    if request.param not in _cache:
        _cache[request.param] = Fixture(*request.param)
    return _cache[request.param]


def test_float64_products_sit_within_a_tenth_of_every_bar(fx):
    ref, f64 = fx.run(), fx.run(dtype=np.float64)
    worst = max(float((np.abs(a - b) / bar).max()) for a, b, bar in zip(f64, ref, fx.bars))
    print("float64 against longdouble, worst fraction of the bar:", worst)
    assert worst <= 0.1


def test_zeroing_any_128_block_of_c_inv_moves_both_outputs_by_1000_bars(fx):
    ref = fx.run()
    least = np.inf
    for i0 in range(0, fx.N, 128):
        for j0 in range(0, fx.N, 128):
            C = fx.C_inv.copy()
            C[i0:i0 + 128, j0:j0 + 128] = 0.0
            got = fx.run(C)
            for k in (0, 1):                      # x_new, dx_new
                least = min(least, float((np.abs(got[k] - ref[k]) / fx.bars[k]).max()))
    print("least movement over the blocks, in bars:", least)
    assert least >= 1000.0


def test_transposing_a_non_symmetric_c_inv_moves_x_new_by_1000_bars(fx):
    C = fx.C_inv * (1.0 + 1e-3 * np.random.default_rng(3).standard_normal(fx.C_inv.shape))
    bar = gpr.bars_component(fx.Ks, fx.pKs, C, fx.X, MU, fx.phi1, fx.dpp)[0]
    moved = float((np.abs(fx.run(C.T)[0] - fx.run(C)[0]) / bar).max())
    print("movement under the transpose, in bars:", moved)
    assert moved >= 1000.0


def test_rows_at_exact_grid_times_reproduce_the_draw_and_m_times_the_centred_draw(fx):
    x_new, dx_new = (np.asarray(a, dtype=np.float64) for a in fx.run(dtype=np.float64)[:2])
    _, m, _ = orc.build_matrices(fx.I.reshape(-1, 1), fx.phi1, fx.phi2)
    bound = 100.0 * fx.cond * U * np.abs(fx.X).max()
    rows = np.arange(len(fx.t_new) - 3, len(fx.t_new))
    ex = np.abs(x_new[:, rows] - fx.X[:, fx.grid_idx]).max()
    ed = np.abs(dx_new[:, rows] - ((fx.X - MU) @ m.T)[:, fx.grid_idx]).max()
    print("grid rows: |x_new - x|", ex, "bound", bound, "; |dx_new - m (x - mu)|", ed, "bound", bound * np.abs(m).max())
    assert ex <= bound
    assert ed <= bound * np.abs(m).max()


def test_unclamped_variance_stays_inside_its_bar(fx):
    for k in (2, 3):                              # var, dvar
        v, bar = np.asarray(fx.run(dtype=np.float64)[k], dtype=np.longdouble), fx.bars[k]
        print("unclamped variance: min", float(v.min()), "at grid times", [float(a) for a in v[-3:]], "bar", [float(b) for b in bar[-3:]])
        assert (v >= -bar).all()
        if k == 2:                                # (at a grid time x is known; x' is not: its variance there is the diagonal of K_d)
            assert (v[-3:] <= bar[-3:]).all()


def test_cross_blocks_of_the_grid_itself_are_the_square_blocks(fx):
    Ks, pKs = gpr.cross_blocks(fx.I, fx.I, fx.phi1, fx.phi2)
    assert np.array_equal(Ks, fx.Kappa) and np.array_equal(pKs, fx.pKappa)
    assert np.array_equal(np.diag(Ks), np.full(fx.N, fx.phi1)) and np.array_equal(np.diag(pKs), np.zeros(fx.N))
