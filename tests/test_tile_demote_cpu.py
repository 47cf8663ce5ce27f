"""The criterion of the certified fp32 block format (csrc/pack.hip, option tile_demote), restated in numpy, on oracle-built operators.

The pack stores an off-diagonal 128 x 128 block of FH = Csym + m^T Ksym m, FK = Ksym (lower block triangle) or FE = Ksym m (every block)
a second time as fp32 when every row abs-sum is <= 2^-29 of the abs-sum of the same row of the diagonal block (bi, bi) of the same
operator and every column abs-sum <= 2^-29 of the same column of block (bj, bj): fp32 rounding (2^-24) of such a block moves an output
entry by at most 2^-53 of the diagonal block's sum of magnitudes.  Entries beyond N are zero on both sides and pass; a non-zero against
a zero reference fails.  On Matern operators the precision decays exponentially: at N = 512 (dt 0.025, four block rows) every block
with |bi - bj| >= 2 passes and no nearer one does, with more than eight orders between the two groups."""
import functools

import numpy as np

from oracle import magi_oracle as orc

TB = 128
RATIO = 2.0 ** -29


def fused_operators(C_inv, m, K_inv):
    """(FH, FK, FE) [D, N, N] as csrc/pack.hip forms them from the dense stacks."""
    Cs = 0.5 * (C_inv + np.transpose(C_inv, (0, 2, 1)))
    Ks = 0.5 * (K_inv + np.transpose(K_inv, (0, 2, 1)))
    FE = Ks @ m
    return Cs + np.transpose(m, (0, 2, 1)) @ FE, Ks, FE


def block_split(FH, FK, FE):
    """[(d, kind, bi, bj, demoted, ratio)] of every stored block; kind 0 FH, 1 FK, 2 FE.  ratio = the largest row / column abs-sum over
    its reference (0 / 0, the padding, left out; non-zero / 0 = inf); nan for the diagonal blocks, which are never candidates."""
    D, N, _ = FH.shape
    nb = -(-N // TB)
    out = []
    for d in range(D):
        for kind, A in enumerate((FH, FK, FE)):
            P = np.zeros((nb * TB, nb * TB))
            P[:N, :N] = np.abs(A[d])
            B = P.reshape(nb, TB, nb, TB)
            rows, cols = B.sum(axis=3), B.sum(axis=1)           # [bi, r, bj], [bi, bj, c]
            for bi in range(nb):
                for bj in range(nb):
                    if kind != 2 and bj > bi:
                        continue
                    if bi == bj:
                        out.append((d, kind, bi, bj, False, np.nan))
                        continue
                    rs, rref = rows[bi, :, bj], rows[bi, :, bi]
                    cs, cref = cols[bi, bj, :], cols[bj, bj, :]
                    ok = bool((rs <= RATIO * rref).all() and (cs <= RATIO * cref).all())
                    num, den = np.concatenate([rs, cs]), np.concatenate([rref, cref])
                    live = (num > 0) | (den > 0)
                    with np.errstate(divide="ignore"):
                        ratio = float((num[live] / den[live]).max()) if live.any() else 0.0
                    out.append((d, kind, bi, bj, ok, ratio))
    return out


@functools.lru_cache(maxsize=None)
def matern_seir(N):
    """The benchmark's problem at grid size N: (I, phi1s, phi2s, X_obs) of host.synthetic_seir with the initial hyper-parameters."""
    from magi_v2_amd import host
    I, X_obs, _, _ = host.synthetic_seir(N, seed=0)
    hp = host.hparams_initial(host.linear_interpolate(X_obs))
    return I, hp["phi1s"], hp["phi2s"], X_obs


def test_split_on_oracle_operators_at_n512():
    I, phi1s, phi2s, _ = matern_seir(512)
    split = block_split(*fused_operators(*orc.build_all(I, phi1s, phi2s, 2.01, bandsize=None)))
    off = [b for b in split if b[2] != b[3]]
    dem = [b for b in off if b[4]]
    kept = [b for b in off if not b[4]]
    worst, smallest = max(b[5] for b in dem), min(b[5] for b in kept)
    print(f"N=512: {len(split)} stored blocks, {len(dem)} demoted, worst passing ratio {worst:.3g}, smallest failing ratio {smallest:.3g}")
    assert len(split) == 144 and len(dem) == 48
    assert all(abs(b[2] - b[3]) >= 2 for b in dem)
    assert worst < RATIO
    assert smallest > 0.1


def test_zero_reference_and_padding():
    """A block of zeros against anything passes (padding: 0 <= 0); a single non-zero against a zero reference row fails."""
    N, D = 300, 1                                               # three block rows, the last 44 wide
    rng = np.random.default_rng(5)
    Z = np.zeros((D, N, N))
    A = Z.copy()
    for b in range(3):
        s = slice(b * TB, min((b + 1) * TB, N))
        A[0, s, s] = rng.standard_normal((s.stop - s.start,) * 2)
    A[0, 256:300, 0:128] = 2.0 ** -45 * rng.standard_normal((44, 128))
    split = {(k, bi, bj): (ok, r) for _, k, bi, bj, ok, r in block_split(A, A, A)}
    assert split[(2, 2, 0)][0] and split[(2, 0, 2)][0] and split[(2, 1, 0)][0]      # tiny, all zero, all zero
    A[0, 5, 5] = 0.0
    A[0, 5, 0:128] = 0.0                                         # row 5 of the reference block (0, 0) is now zero ...
    A[0, 5, 260] = 1e-300                                        # ... and block (0, 2) has an entry in that row
    split = {(k, bi, bj): (ok, r) for _, k, bi, bj, ok, r in block_split(A, A, A)}
    assert not split[(2, 0, 2)][0] and split[(2, 0, 2)][1] == np.inf
