"""The graded fixture of the certified fp32 block format (csrc/pack.hip, option tile_demote), oracle side only.

tests/test_tile_demote_gpu.py holds the format to truth at N = 384 with m = I, a symmetric K^-1 and one demoted index set: FE = FK, FE(0, 2) =
FE(2, 0)^T, every operator of every component demotes the same blocks -- a reader that takes FK's narrow copy for FE's, reads an FE block
transposed or takes the neighbouring slot produces the same numbers.  Here the stacks are GRADED per (stack, component, |bi - bj|), m = diag(s)
with s from {+-1, +-2, +-1/2} (FE = K diag(s) is exact, not symmetric and not FK), and N is ragged (300: the last block 44 wide; 513: 1 wide):

  role of a component      first neighbours, C and K     far blocks of C     far blocks of K      demoted (N = 300: of 12 off-diagonal blocks)
  plain                    NEAR_KEPT                     FAR                 FAR                  the far FH, FK, FE                   4
  far_k                    NEAR_KEPT                     FAR                 FAR_KEPT             nothing                              0
  far_c                    NEAR_KEPT                     FAR_KEPT            FAR                  far FK and FE; FH is kept            3
  near                     FAR                           FAR                 FAR                  every off-diagonal block             12

(roles dealt by the size of each component's drift, see roles_of; rotated by `salt`).  FAR passes the criterion with a ratio <= 2^-29 / 2 everywhere, FAR_KEPT and NEAR_KEPT
fail it by >= 2 x: no block sits where device sums and numpy sums could disagree (tests/test_demote_edges_cpu.py asserts it).

What the comparisons on the GPU need, and tests/test_demote_edges_cpu.py proves on the oracle alone: the `rounded` problem's stacks reproduce
the operators with exactly the demoted blocks rounded to fp32, bit for bit; every demoted block, zeroed, transposed in place or swapped with
another demoted block, moves the gradient on a compared set of some state by >= 1000 x the bar applied there; the rounding itself moves it by
>= 10 x the bar; the fp64 oracle sits >= 100 x below the bars.

The states: the fixture's smooth state with the grid points of ONE block column times BIG, one state per block column -- a block (bi, bj)
is fed by the state of column bj (row-type products) or bi (the column-type product FE^T f), and seen in block row bi (bj) only.  The
compared sets of a state are (block row, component) pairs: the rows of that block row in that column of the gradient.

Why these scales.  A demoted block is at most 2^-29 of its diagonal block, and a comparison in fp64 sees 1e-12: the state has to be large
where the block reads and ordinary where it writes (BIG).  A product of two large components makes f quadratic in BIG, and J^T carries
(FK f - FE xc) of one component into other components' columns of gX: a kept block of K at 0.05 or 2^-24 beside demoted ones at 2^-40
buries them there (measured: first-neighbour blocks that qualify moved the gradient by 5e-6 of a bar).  So every off-diagonal block is
small -- kept ones 2^9 x the demoted ones, a factor 6 above the threshold where the demoted ones are a factor 3 below it -- BIG is 2^15,
and the roles go by the size of each component's drift (roles_of).  sigma^2 is ~ 3 at every state: the observation term has no operator in
it and is no part of sum_bound, and at sigma^2 ~ 0.05 its own rounding was 3e-2 of that bar."""
import contextlib
import dataclasses
import functools

import numpy as np

from oracle import magi_oracle as orc
from tests.test_structureless_cpu import TRACED, fixture, register_traced
from tests.test_tile_demote_cpu import RATIO, TB, block_split, fused_operators
from tests.util import structureless_theta

FH, FK, FE = 0, 1, 2
NEAR_KEPT, FAR, FAR_KEPT = 2.0 ** -26, 2.0 ** -35, 2.0 ** -26
BIG = 2.0 ** 15
QUANTUM = 2.0 ** -72                                             # off-diagonal entries are multiples of it: C + s K s and FH - s r32(K) s are exact in fp64
SIG_PRE = 3.0                                                    # sigma^2 ~ 3: the observation term (no operator in it, none in sum_bound) and its rounding stay small
S_VALUES = (1.0, -1.0, 2.0, -2.0, 0.5, -0.5)
VALU_BAR = 1e-12                                                 # of a compared set's largest entry (tests/test_tile_demote_gpu.py)


def r32(A):
    return np.asarray(A).astype(np.float32).astype(np.float64)


def roles_of(drift_fn, X, th, salt=0):
    """The roles dealt by the size of the drift at a state times BIG: the components with the largest |f_d| (products of two large
    components) are `near` and `plain`, the smallest is `far_k` -- its kept far K blocks, 2^9 x the demoted ones, are multiplied with the
    smallest f and drown no demoted block's product in the columns of gX they share through J^T.  Three components: `near` is `far_c` too.
    `salt` rotates the roles that many components on."""
    D = X.shape[1]
    mag = np.median(np.abs(drift_fn(X * BIG, th)[0]), axis=0)
    order = np.argsort(-mag, kind="stable")
    names = ["near+far_c", "plain", "far_k"] if D == 3 else ["near", "plain"] + ["near"] * (D - 4) + ["far_c", "far_k"]
    roles = [None] * D
    for rank, d in enumerate(order):
        roles[d] = names[rank]
    return [roles[(d - salt) % D] for d in range(D)]


def _scale(stack, role, dist):
    if dist == 1:
        return FAR if role.startswith("near") else NEAR_KEPT
    if (stack == "K" and role == "far_k") or (stack == "C" and role.endswith("far_c")):
        return FAR_KEPT
    return FAR


def _blocks(N):
    nb = -(-N // TB)
    return [slice(b * TB, min((b + 1) * TB, N)) for b in range(nb)]


def _graded_stack(rng, N, stack, roles):
    """[D, N, N], symmetric: diagonal blocks G G^T / 128 + I, block (bi, bj) below the diagonal scale(stack, role, bi - bj) N(0, 1) / sqrt(128)."""
    bl = _blocks(N)
    A = np.zeros((len(roles), N, N))
    for d, role in enumerate(roles):
        for bi, ri in enumerate(bl):
            w = ri.stop - ri.start
            G = rng.standard_normal((w, w))
            A[d, ri, ri] = G @ G.T / TB + np.eye(w)
            for bj in range(bi):
                rj = bl[bj]
                O = _scale(stack, role, bi - bj) * rng.standard_normal((w, rj.stop - rj.start)) / np.sqrt(TB)
                O = np.round(O / QUANTUM) * QUANTUM
                A[d, ri, rj] = O
                A[d, rj, ri] = O.T
    return A


class Graded:
    """Everything about one graded case; build with graded(N, drift, salt).  Read-only: shared across tests."""


@functools.lru_cache(maxsize=None)
def graded(N, drift, salt=0):
    had = drift in orc.DRIFTS
    pr, X = fixture(N, drift, spd=True)
    D = pr.D
    rng = np.random.default_rng([1905, N, D, salt, sorted(("seir3", "seir4", "sirw") + TRACED).index(drift)])
    roles = roles_of(orc.DRIFTS[drift][0], X, structureless_theta(drift), salt)
    C, K = _graded_stack(rng, N, "C", roles), _graded_stack(rng, N, "K", roles)
    s = rng.choice(S_VALUES, size=(D, N))
    m = np.zeros((D, N, N))
    m[:, np.arange(N), np.arange(N)] = s
    exact = dataclasses.replace(pr, C_inv=C, m=m, K_inv=K)
    ops = fused_operators(C, m, K)
    split = block_split(*ops)
    dem = {(d, k, bi, bj) for d, k, bi, bj, ok, _ in split if ok}

    # the stacks that reproduce the operators with the demoted blocks rounded: K' = r32(K) where FK / FE are demoted, C' = FH_target - s K' s
    bl = _blocks(N)
    Cr, Kr = C.copy(), K.copy()
    target = [A.copy() for A in ops]
    for d in range(D):
        for bi, ri in enumerate(bl):
            for bj in range(bi):
                rj = bl[bj]
                k_dem, h_dem = (d, FK, bi, bj) in dem, (d, FH, bi, bj) in dem
                if not (k_dem or h_dem):
                    continue
                Kb = r32(K[d, ri, rj]) if k_dem else K[d, ri, rj]
                Hb = r32(ops[FH][d, ri, rj]) if h_dem else ops[FH][d, ri, rj]
                sKs = s[d, ri, None] * Kb * s[d, None, rj]
                Cb = Hb - sKs                                    # (exact: every term is a multiple of QUANTUM / 4 below 2^-20)
                assert np.array_equal(Cb + sKs, Hb), (d, bi, bj)
                Kr[d, ri, rj], Kr[d, rj, ri] = Kb, Kb.T
                Cr[d, ri, rj], Cr[d, rj, ri] = Cb, Cb.T
                target[FH][d, ri, rj], target[FH][d, rj, ri] = Hb, Hb.T
                target[FK][d, ri, rj], target[FK][d, rj, ri] = Kb, Kb.T
                target[FE][d, ri, rj], target[FE][d, rj, ri] = Kb * s[d, None, rj], Kb.T * s[d, None, ri]
    rounded = dataclasses.replace(pr, C_inv=Cr, m=m, K_inv=Kr)

    g = Graded()
    g.N, g.D, g.drift, g.salt, g.roles, g.s, g.nb, g.blocks = N, D, drift, salt, roles, s, len(bl), bl
    g.exact, g.rounded, g.X, g.split, g.demoted = exact, rounded, X, split, sorted(dem)
    g.ops, g.target = ops, tuple(target)
    g.sp = np.full(D, SIG_PRE)
    g.tp = np.log(np.expm1(structureless_theta(drift)))
    g.traced = register_traced(drift, N)                         # the magi_v2_amd Drift of a traced example (None: a built-in)
    g.entry = orc.DRIFTS[drift]                                  # (a traced drift's entry is bound to this grid: see registered)
    _, J, _ = g.entry[0](X, np.log1p(np.exp(g.tp)))
    g.deps = [[e for e in range(D) if np.any(J[:, d, e] != 0.0)] for d in range(D)]      # deps[d]: the columns of gX that f_d reaches through J^T
    g.states = _states(g)
    if not had:                                                  # (other tests iterate over the oracle's drift table: see registered)
        del orc.DRIFTS[drift]
    return g


@contextlib.contextmanager
def registered(g):
    """The oracle's drift table with this case's entry, for the duration only: a traced drift is no entry of the table as other tests
    expect it, and one that uses t is bound to a grid -- another test may have registered another grid since the case was built."""
    before = orc.DRIFTS.get(g.drift)
    orc.DRIFTS[g.drift] = g.entry
    try:
        yield g
    finally:
        if before is not None:
            orc.DRIFTS[g.drift] = before
        else:
            del orc.DRIFTS[g.drift]


def graded_problem(N, drift, salt=0):
    """(exact, rounded, X, split): the graded problem, the problem whose stacks carry the fp32-rounded demoted blocks, the base state and
    block_split(...) of the exact operators."""
    g = graded(N, drift, salt)
    return g.exact, g.rounded, g.X, g.split


# ---- states and compared sets ----------------------------------------------------------------------------------------------------------

@dataclasses.dataclass
class State:
    name: str
    X: np.ndarray
    sets: list                                                   # [(block row, component)]: rows of the block row, that column of gX


def _feeds(g, j):
    """(block row, column of gX) sets that a demoted block feeds from block column j."""
    sets = set()
    for d, kind, bi, bj in g.demoted:
        for src, dst in ((bj, bi), (bi, bj)):
            if src != j:
                continue
            if kind == FH:                                       # FH(bi, bj) xc_bj -> rows bi; its mirror FH(bi, bj)^T xc_bi -> rows bj
                sets.add((dst, d))
            elif kind == FK:                                     # J^T FK f, both triangles
                sets.update((dst, e) for e in g.deps[d])
            elif src == bj:                                      # J^T FE(bi, bj) xc_bj -> rows bi
                sets.update((dst, e) for e in g.deps[d])
            else:                                                # FE(bi, bj)^T f_bi -> rows bj
                sets.add((dst, d))
    return sorted(sets)


def _states(g):
    """One state per block column j: the smooth state with the grid points of block j times BIG."""
    out = []
    for j, rj in enumerate(g.blocks):
        Xj = g.X.copy()
        Xj[rj] *= BIG
        out.append(State(f"col{j}", Xj, _feeds(g, j)))
    return out


# ---- the gradient from the operators, and what a perturbed block does to it -------------------------------------------------------------

def drift_terms(g, X):
    f, J, _ = g.entry[0](X, np.log1p(np.exp(g.tp)))
    return (X - g.exact.mu[None]).T, f.T, J                      # xc [D, N], f [D, N], J[n, d', d] = df_d' / dx_d


def operator_gX(g, ops, X, temp=1.0):
    """gX of the log posterior from the single-phase operators (csrc/pack.hip):  -(temp / beta) (FH xc - FE^T f + J^T (FK f - FE xc)) + the
    observation term, in fp64 numpy."""
    pr = g.exact
    xc, f, J = drift_terms(g, X)
    a = np.einsum("dnm,dm->dn", ops[FH], xc) - np.einsum("dmn,dm->dn", ops[FE], f)
    p = np.einsum("dnm,dm->dn", ops[FK], f) - np.einsum("dnm,dm->dn", ops[FE], xc)
    sig = np.log1p(np.exp(g.sp)) + pr.LB
    cols = pr.obs_idx % g.D
    d4 = np.zeros(X.size)
    np.add.at(d4, pr.obs_idx, 2.0 * (X.reshape(-1)[pr.obs_idx] - pr.y) / sig[cols])
    return temp * (-(1.0 / pr.beta) * (a.T + np.einsum("dn,nde->ne", p, J)) - 0.5 * d4.reshape(X.shape))


def delta_gX(g, X, changes, temp=1.0):
    """The exact change of operator_gX when stored blocks change: `changes` = [(d, kind, bi, bj, new - old)].  A stored FH / FK block (bi > bj)
    stands for its mirror too."""
    xc, f, J = drift_terms(g, X)
    a, p = np.zeros_like(xc), np.zeros_like(xc)
    for d, kind, bi, bj, dB in changes:
        ri, rj = g.blocks[bi], g.blocks[bj]
        if kind == FH:
            a[d, ri] += dB @ xc[d, rj]
            a[d, rj] += dB.T @ xc[d, ri]
        elif kind == FK:
            p[d, ri] += dB @ f[d, rj]
            p[d, rj] += dB.T @ f[d, ri]
        else:
            a[d, rj] -= dB.T @ f[d, ri]
            p[d, ri] -= dB @ xc[d, rj]
    return -(temp / g.exact.beta) * (a.T + np.einsum("dn,nde->ne", p, J))


def stored_block(g, ops, key):
    d, kind, bi, bj = key
    return ops[kind][d, g.blocks[bi], g.blocks[bj]]


def padded(B):
    P = np.zeros((TB, TB))
    P[:B.shape[0], :B.shape[1]] = B
    return P


def _live(g, key, P):
    _, _, bi, bj = key
    ri, rj = g.blocks[bi], g.blocks[bj]
    return P[:ri.stop - ri.start, :rj.stop - rj.start]


def swap_partners(g, key):
    """Demoted blocks a reader could take for `key`: the other operator of the same indices (FK <-> FE), the same block of the next component
    that demotes it, and the block before it in the demoted list (the neighbouring slot of the narrow buffer)."""
    d, kind, bi, bj = key
    dem = g.demoted
    out = []
    for other in (FK, FE, FH):
        if other != kind and (d, other, bi, bj) in dem:
            out.append((d, other, bi, bj))
            break
    for k in range(1, g.D):
        if ((d + k) % g.D, kind, bi, bj) in dem:
            out.append(((d + k) % g.D, kind, bi, bj))
            break
    out.append(dem[dem.index(key) - 1])
    return [o for i, o in enumerate(out) if o != key and o not in out[:i]]


def perturbations(g, key):
    """[(name, changes)] for a demoted block: zeroed; transposed in place (as 128 x 128 storage: a ragged block loses what falls outside its
    live part); swapped with each of swap_partners (both blocks change)."""
    B = stored_block(g, g.target, key)
    out = [("zero", [key + (-B,)]), ("transpose", [key + (_live(g, key, padded(B).T) - B,)])]
    for other in swap_partners(g, key):
        Bo = stored_block(g, g.target, other)
        out.append((f"swap{other}", [key + (_live(g, key, padded(Bo)) - B,), other + (_live(g, other, padded(B)) - Bo,)]))
    return out


# ---- bars ----------------------------------------------------------------------------------------------------------------------------

def sum_bound(pr, X, th_pre):
    """A-priori, entrywise, first-order error of gX for ANY summation order of its matrix terms in fp64:
    n 2^-53 (|FH| |xc| + |FE|^T |f| + |J|^T (|FK| |f| + |FE| |xc|)) / beta over all blocks, n = N + 8.  Derived from no kernel."""
    H, K, E = (np.abs(A) for A in fused_operators(pr.C_inv, pr.m, pr.K_inv))
    f, J, _ = orc.DRIFTS[pr.drift][0](X, np.log1p(np.exp(th_pre)))
    axc, af = np.abs(X - pr.mu[None]).T, np.abs(f).T
    a = np.einsum("dnm,dm->dn", H, axc) + np.einsum("dmn,dm->dn", E, af)
    p = np.einsum("dnm,dm->dn", K, af) + np.einsum("dnm,dm->dn", E, axc)
    return (len(X) + 8) * 2.0 ** -53 * (a.T + np.einsum("dn,nde->ne", p, np.abs(J))) / pr.beta


def rounding_bound(g, X):
    """|change of gX| that rounding the demoted blocks to fp32 can cause, entry by entry: 2^-24 |B| over the demoted blocks, through the same
    expression (tests/test_tile_demote_gpu.py: _far_bound)."""
    xc, f, J = drift_terms(g, X)
    a, p = np.zeros_like(xc), np.zeros_like(xc)
    axc, af = np.abs(xc), np.abs(f)
    for key in g.demoted:
        d, kind, bi, bj = key
        B = np.abs(stored_block(g, g.ops, key))
        ri, rj = g.blocks[bi], g.blocks[bj]
        if kind == FH:
            a[d, ri] += B @ axc[d, rj]
            a[d, rj] += B.T @ axc[d, ri]
        elif kind == FK:
            p[d, ri] += B @ af[d, rj]
            p[d, rj] += B.T @ af[d, ri]
        else:
            a[d, rj] += B.T @ af[d, ri]
            p[d, ri] += B @ axc[d, rj]
    return 2.0 ** -24 * (a.T + np.einsum("dn,nde->ne", p, np.abs(J))) / g.exact.beta


# ---- the reference gradients, computed once per case and shared (read-only) -----------------------------------------------------------

@dataclasses.dataclass
class Reference:
    logp: float                                                  # the oracle on the rounded stacks
    gX: np.ndarray
    gX_exact: np.ndarray                                         # the oracle on the unrounded stacks
    bound: np.ndarray                                            # sum_bound on the rounded stacks, entrywise
    rounding: np.ndarray                                         # rounding_bound, entrywise


@functools.lru_cache(maxsize=None)
def references(N, drift, salt=0):
    """[Reference] per state of graded(N, drift, salt)."""
    g = graded(N, drift, salt)
    out = []
    with registered(g):
        for st in g.states:
            lp, gX, _, _ = orc.logpost_grad(st.X, g.sp, g.tp, 1.0, g.rounded)
            gE = orc.logpost_grad(st.X, g.sp, g.tp, 1.0, g.exact)[1]
            out.append(Reference(lp, gX, gE, sum_bound(g.rounded, st.X, g.tp), rounding_bound(g, st.X)))
    return out


def set_views(g, st, *arrays):
    """[(set, [a[rows, column] for a in arrays])] over the compared sets of a state."""
    return [((bi, e), [a[g.blocks[bi], e] for a in arrays]) for bi, e in st.sets]
