"""Dev: per-CU bytes against per-CU last end of the one-chain stream launch at N = 1024 (needs a -DMAGI_WG_TRACE build, as tools/exp_wg_trace.py:
    python -m magi_v2_amd.build --variant wgtrace -DMAGI_WG_TRACE
    MAGI_HIP_LIB=build_variants/wgtrace/libmagi_hip.so [MAGI_STREAM_CARRIERS=-1] python tools/exp_wg_trace_bytes.py OUTFILE [traces]
A block the VALU kernel reads as fp32 counts 64 KB (Matern operators at N = 1024: |bi - bj| >= 2, checked against tile_formats), every other
128 KB; under a carrier launch a CU's bytes are its carrier's units.  CU counts are pooled over the traces; the slope is a least-squares fit per
trace.  profiles/r22_wg_trace_1chain_fp32.txt and section 4 of profiles/r22_carriers_ab.txt are its output."""
import ctypes as C
import os
import sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magi_v2_amd import host
from magi_v2_amd.engine import MagiEngine

outp = sys.argv[1]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n, N = 1, 1024
lines = []
def P(s):
    print(s, flush=True)
    lines.append(s)

I, X_obs, truth, th = host.synthetic_seir(N, seed=0)
Xi = host.linear_interpolate(X_obs); hp = host.hparams_initial(Xi)
N_ds, beta, idx, y = host.observation_bookkeeping(X_obs, X_obs)
Xhat = host.cubic_smoother(I, Xi); LB = host.sigma_sqs_lower_bound(Xhat)
sp0, tp0 = host.softplus_inverse_inits(hp["sigma_sqs"], np.ones(3), LB)
eng = MagiEngine(0)
eng.build_matrices(I, hp["phi1s"], hp["phi2s"], 2.01, want_host=False)
eng.set_problem(Xi.mean(axis=0), N_ds.astype(float), idx, y, beta, LB, "seir4")
rep = lambda v: np.repeat(np.asarray(v)[None], n, axis=0)
eng.logpost_grad(rep(Xhat), rep(sp0), rep(tp0), 1.0, fused=True)
fn = eng._lib.magi_debug_wg_trace
fn.restype = C.c_int
fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]

D, nb = 4, (N + 127) // 128
tasks = [(d, k, bi, bj) for d in range(D) for k in range(3) for bi in range(nb) for bj in range(nb) if k == 2 or bj <= bi]
carr = None
if hasattr(eng, "stream_carriers"):
    info = eng.stream_carriers()
    if info["on"]:
        carr = info
if carr is None:
    C_, T_ = 256, len(tasks) + 1
    if (T_ + C_ - 1) // C_ == 3 and T_ % C_ > 1:
        r_ = T_ % C_ - 1
        heavy = [t for t in tasks if t[1] != 0]; off = [t for t in tasks if t[1] == 0 and t[2] != t[3]]; diag = [t for t in tasks if t[1] == 0 and t[2] == t[3]]
        tasks = off[:r_] + heavy[:C_ - r_] + diag[:r_] + off[r_:2 * r_] + heavy[C_ - r_:] + off[2 * r_:] + diag[r_:]
    kb = np.array([64.0 if abs(t[2] - t[3]) >= 2 else 128.0 for t in tasks])
    fmt = eng.tile_formats(1)
    P(f"# tile_formats: {fmt}; blocks read as fp32 by the rule |bi - bj| >= 2: {(kb == 64).sum()}")
    # (the order and the rule restate pack.hip: refuse to tabulate where they do not describe this pack)
    if fmt[0] != len(kb) or fmt[1] != int((kb == 64).sum()) or fmt[2] != kb.sum() * 1024:
        sys.exit(f"the restated task list ({len(kb)} blocks, {(kb == 64).sum()} of them fp32, {kb.sum():.0f} KB) is not the library's pack {fmt}")
else:
    kb = np.asarray(carr["units"], dtype=float) * 64.0
    P(f"# carrier launch: {len(kb)} carriers, units per carrier: " + ", ".join(f"{u}x{(np.asarray(carr['units']) == u).sum()}" for u in np.unique(carr["units"])))

for with_point in (0, 1):
    allr = []
    for r in range(reps):
        out = np.zeros((2, 4096, 4), dtype=np.uint64)
        eng._check(fn(eng._h, n, 20, with_point, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        allr.append(out.astype(np.int64))
    spans, pooled, slopes = [], {}, []
    for a in allr:
        tr = a[0]
        used = tr[:, 0] > 0
        nw = int(used.sum())
        t0 = tr[used, 0].min()
        e = (tr[used, 1] - t0) * 0.01
        spans.append(e.max())
        hw = tr[used, 2]
        xcc = (hw >> 32) & 0xF
        cu = (hw >> 8) & 0xF; sh = (hw >> 12) & 1; se = (hw >> 13) & 7
        key = xcc * 1000 + se * 100 + sh * 16 + cu
        if nw != len(kb):
            P(f"    ({nw} workgroups traced, {len(kb)} expected: no byte table)")
            continue
        ucu = np.unique(key)
        cb = np.array([kb[key == k].sum() for k in ucu]); ce = np.array([e[key == k].max() for k in ucu])
        for b_, e_ in zip(cb, ce):
            pooled.setdefault(b_, []).append(e_)
        if len(np.unique(cb)) > 1:
            slopes.append(np.polyfit(cb / 64.0, ce, 1)[0])
        last = (len(ucu), np.bincount(np.unique(key, return_counts=True)[1]))
    P(f"--- stream (with_point={with_point}), 1 chain, N={N}: launch span of the {reps} traces: " + ", ".join("%.2f" % s for s in spans) + " us")
    if pooled:
        P(f"    distinct CUs {last[0]}; workgroups per CU (count: CUs) " + ", ".join(f"{c}: {m}" for c, m in enumerate(last[1]) if m))
        P("    per-CU bytes | CUs (all traces) | last end: median   p90    max  (us from the launch's first workgroup)")
        for b_ in sorted(pooled):
            v = np.array(pooled[b_])
            P(f"    {b_:8.0f} KB | {len(v):6d}           | {np.median(v):15.2f} {np.percentile(v, 90):6.2f} {v.max():6.2f}")
        if slopes:
            P("    least-squares slope of per-CU last end on per-CU bytes, per trace: " + ", ".join("%.3f" % s for s in slopes) + " us per 64 KB")
eng.close()
open(outp, "w").write("\n".join(lines) + "\n")
