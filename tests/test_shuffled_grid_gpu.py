"""GPU tests of the matrix build where every block of the factors counts: Matern grids in SHUFFLED order (tests/util.py: shuffled_grid).

On a sorted grid the Cholesky factor of Kappa and its triangular inverse are numerically block-bidiagonal, so a trtri level that never
ran, a remainder pass with a wrong row count, a triangular k range one block short at distance two or more, or a rank-k update that
dropped a far tile passes every sorted test (N = 2048 .. 8192 included).  Kappa(I[perm]) = P Kappa P^T has the sorted matrix's condition
number and a factor that fills in completely; tests/test_shuffled_grid_cpu.py asserts, on the oracle alone, that the truth used here has
100 x of room under each bar and that any single zeroed 128-block of T = L^-1 or of K_d's factor inverse moves a residual below to at
least 1000 x its bar.  Residuals and bars are those of tests/test_build_gpu.py::test_build_multi_block_inverse_property, unchanged.

Sizes, chosen for the control flow of potrf and trtri (csrc/build.hip):
   300   three block rows, the last ragged; trtri's only remainder pass is at level 256 (M2 = 44);
   513   a one-row last block; two full pairs at level 128, one at 256, and no pass touches the last row (it stays as potrf left it);
   700   a remainder pass at level 128 (M2 = 60), none at 256, a 512-level pass with M2 = 188;
  1100   three block columns of the default 3-panel potrf (two full, one of 332); > 2 x 384, so look-ahead can be forced."""
import numpy as np
import pytest

from tests.util import shuffled_grid

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
PHI1, PHI2, NU = np.array([0.03, 0.2]), np.array([0.3, 0.15]), 2.01
SEED = 11

DEFAULT, REMAP, PANELS1 = {}, {"gemm_remap_min": 1}, {"potrf_panels": 1}
PANELS2_LA = {"potrf_panels": 2, "potrf_lookahead_min": 256}
LA512 = {"potrf_lookahead_min": 512}
REMAP_PANELS4_LA = {"gemm_remap_min": 1, "potrf_panels": 4, "potrf_lookahead_min": 512}
BUILD_CASES = ([(N, o) for N in (300, 513, 700, 1100) for o in (DEFAULT, REMAP, PANELS1)] + [(N, PANELS2_LA) for N in (513, 700, 1100)]
               + [(1100, LA512), (1100, REMAP_PANELS4_LA)])


def case_id(case):
    N, opts = case
    return f"{N}-" + ("-".join(f"{k}={v}" for k, v in opts.items()) or "default")


def relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.fixture(scope="module")
def eng():
    from magi_v2_amd.engine import MagiEngine
    e = MagiEngine(0)
    yield e
    e.close()


def fresh_engine(opts):
    from magi_v2_amd.engine import MagiEngine
    e = MagiEngine(0)
    for name, value in opts.items():
        e.set_option(name, value)
    return e


_truth = {}


def truth(eng, N):
    """Per component of the shuffled grid of size N: the GPU's own Matern blocks (pinned to mpmath by tests/test_build_gpu.py, and under a
    shuffle by the bit-identity test below), the host's m_ref, K_ref and the two condition numbers.  Computed once and shared: read-only."""
    if N not in _truth:
        I, perm = shuffled_grid(N, SEED)
        comps = []
        for d in range(2):
            Kap, pK, Kpp = eng.matern_blocks(I[perm], PHI1[d], PHI2[d], NU)
            m_ref = np.linalg.solve(Kap, pK.T).T                      # p_Kappa Kappa^-1
            K_ref = Kpp - m_ref @ (-pK)
            K_ref = 0.5 * (K_ref + K_ref.T)
            comps.append(dict(Kap=Kap, m_ref=m_ref, K_ref=K_ref, cond=np.linalg.cond(Kap), condK=np.linalg.cond(K_ref)))
        _truth[N] = (I, perm, comps)
    return _truth[N]


def check_build(out, comps, what):
    """The three residual checks of test_build_multi_block_inverse_property and exact symmetry of both inverses; every figure is printed
    as a fraction of its bar before it is asserted."""
    C_inv, m, K_inv = out
    N = C_inv.shape[1]
    for d, t in enumerate(comps):
        cond, condK = t["cond"], t["condK"]
        rC = np.abs(C_inv[d] @ t["Kap"] - np.eye(N)).max() / (50 * cond * EPS)
        rm = relmax(m[d], t["m_ref"]) / (50 * cond * EPS)
        rK = np.abs(K_inv[d] @ t["K_ref"] - np.eye(N)).max() / (200 * cond * EPS * condK ** 0.5)
        print(f"SHUFFLED-BUILD {what} d={d} cond={cond:.4e} condK={condK:.3e} fractions of the bars: C {rC:.2e} m {rm:.2e} K {rK:.2e}")
        assert rC < 1.0 and rm < 1.0 and rK < 1.0, (what, d, rC, rm, rK)
        assert np.abs(C_inv[d] - C_inv[d].T).max() == 0.0
        assert np.abs(K_inv[d] - K_inv[d].T).max() == 0.0


@pytest.mark.parametrize("N", [200, 513, 1100])
def test_matern_blocks_commute_with_the_shuffle_bit_for_bit(eng, N):
    """k_matern is an element-wise function of (I_i, I_j) -- fabs(dt) and the sign of dt -- so the blocks of the shuffled grid are the
    sorted ones re-indexed, bit for bit; ragged 64-tiles at every size, 4 grid rows per workgroup at 200 and 513 and 16 at 1100."""
    I, perm = shuffled_grid(N, SEED)
    for d in range(2):
        so = eng.matern_blocks(I, PHI1[d], PHI2[d], NU)
        sh = eng.matern_blocks(I[perm], PHI1[d], PHI2[d], NU)
        for a, b, what in zip(sh, so, ("Kappa", "p_Kappa", "Kappa_pp")):
            np.testing.assert_array_equal(a, b[np.ix_(perm, perm)], err_msg=what)
        assert np.array_equal(np.diag(sh[0]), np.full(N, PHI1[d]))
        assert np.array_equal(np.diag(sh[1]), np.zeros(N))
        assert np.array_equal(np.diag(sh[2]), np.full(N, np.diag(so[2])[0]))
        assert np.array_equal(sh[1], -sh[1].T)


@pytest.mark.parametrize("case", BUILD_CASES, ids=case_id)
def test_build_on_a_shuffled_grid(eng, case):
    """Every code path of the build on a grid where every block of the factors counts: the XCD-aware tile order forced, 1 / 2 / 3 / 4 panels
    per potrf block column, look-ahead forced on the second stream."""
    N, opts = case
    I, perm, comps = truth(eng, N)
    e = fresh_engine(opts)
    try:
        out = e.build_matrices(I[perm], PHI1, PHI2, NU)
    finally:
        e.close()
    check_build(out, comps, case_id(case))


def test_serial_build_on_a_shuffled_grid_is_identical_to_the_batched_one(eng):
    """Option build_serial (one component after the other on one work space) at N = 700 shuffled: held to the host truth and bit-identical
    to the batched build; the profiled launch counts show that the serial path ran (tests/test_build_gpu.py)."""
    N = 700
    I, perm, comps = truth(eng, N)
    e = fresh_engine({})
    try:
        e.set_option("build_profile", 1)
        conc = e.build_matrices(I[perm], PHI1, PHI2, NU)
        conc_calls = e.build_profile()["m_K_products"][2]
        e.set_option("build_serial", 1)
        ser = e.build_matrices(I[perm], PHI1, PHI2, NU)
        ser_calls = e.build_profile()["m_K_products"][2]
    finally:
        e.set_option("build_serial", 0)
        e.set_option("build_profile", 0)
        e.close()
    assert (conc_calls, ser_calls) == (3, 3 * 2)
    check_build(ser, comps, "700-build_serial=1")
    for a, b in zip(conc, ser):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("N", [513, 700])
def test_shuffled_build_agrees_with_the_sorted_build(eng, N):
    """out_shuffled = out_sorted[perm, perm]: two elimination orders of one matrix differ by rounding only, so the far blocks that no
    sorted test sees are tied to the mpmath-pinned sorted build.  Conditioning-limited tolerance, the bars of the residual checks."""
    I, perm, comps = truth(eng, N)
    e = fresh_engine({})
    try:
        so = e.build_matrices(I, PHI1, PHI2, NU)
        sh = e.build_matrices(I[perm], PHI1, PHI2, NU)
    finally:
        e.close()
    ix = np.ix_(perm, perm)
    for d, t in enumerate(comps):
        bars = (50 * t["cond"] * EPS, 50 * t["cond"] * EPS, 200 * t["cond"] * EPS * t["condK"] ** 0.5)
        got = [relmax(sh[k][d], so[k][d][ix]) / bars[k] for k in range(3)]
        print(f"SHUFFLED-VS-SORTED N={N} d={d} fractions of the bars: C {got[0]:.2e} m {got[1]:.2e} K {got[2]:.2e}")
        assert max(got) < 1.0, (N, d, got)


def test_resident_stacks_of_a_shuffled_build(eng):
    """The device-resident stacks after a shuffled N = 700 build that never reached the host: dense_apply, plain and transposed, against the
    downloaded stacks times the same vectors (the bar of tests/test_api_gpu.py), and the download held to the host truth."""
    N = 700
    I, perm, comps = truth(eng, N)
    e = fresh_engine({})
    try:
        assert e.build_matrices(I[perm], PHI1, PHI2, NU, want_host=False) is None
        stacks = e.get_dense()
        V = np.random.default_rng(3).standard_normal((2, N, 3))
        for which, A in zip(("C_inv", "m", "K_inv"), stacks):
            atol = 1e-12 * np.abs(A).max()
            np.testing.assert_allclose(e.dense_apply(which, V), np.einsum("dij,djp->dip", A, V), rtol=1e-12, atol=atol, err_msg=which)
            np.testing.assert_allclose(e.dense_apply(which, V, transpose=True), np.einsum("dji,djp->dip", A, V), rtol=1e-12, atol=atol,
                                       err_msg=which + "^T")
    finally:
        e.close()
    check_build(stacks, comps, "700-resident")
