"""Dev: the device time stamps of a -DMAGI_STAMPS=<kernel> build (magi_v2_amd/csrc/stamps.h), as medians in ns from the workgroup's entry.
    python -m magi_v2_amd.build --variant s_<kernel> -DMAGI_STAMPS=<kernel> -DMAGI_STAMP_WG=<task or workgroup>
    MAGI_HIP_LIB=build_variants/s_<kernel>/libmagi_hip.so python tools/stamps.py <kernel> [--n N] [--chains C] [--reps R]
stream, sep: decision-free timing launches (stream: tasks of component 0 at N = 1024 are 0..35 FH, 36..99 FE, 100..135 FK);
point, decide: a running chain.  (diag prints its own stamps: any build of the matrices on the variant shows them.)"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magi_v2_amd import host  # noqa: E402
from magi_v2_amd.engine import MagiEngine  # noqa: E402

# kernel: (default chains, default repetitions, stamp labels in index order)
KERNELS = {
    "stream": (1, 20, ["entry", "theta' written (wave 0 only)", "positions arrived", "barrier 1 (theta')", "barrier 2 (operands in LDS)",
                       "row chunks done", "barrier 3", "end"]),
    "sep": (8, 12, ["entry", "task known", "operand loads issued", "ring issued", "operands in LDS", "barrier"]
            + ["step %d" % k for k in range(8)] + ["stores issued", "stores retired"]),
    "point": (1, 40, ["entry (plan + flag arrived)", "product sums in LDS", "barrier 1", "finish done", "barrier 2", "end"]),
    "decide": (1, 40, None),
}

ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
ap.add_argument("kernel", choices=sorted(KERNELS))
ap.add_argument("--n", type=int, default=1024, help="grid points")
ap.add_argument("--chains", type=int)
ap.add_argument("--reps", type=int)
a = ap.parse_args()
chains0, reps0, labels = KERNELS[a.kernel]
n, reps = a.chains or chains0, a.reps or reps0

I, X_obs, truth, th = host.synthetic_seir(a.n, seed=0)
Xi = host.linear_interpolate(X_obs); hp = host.hparams_initial(Xi)
N_ds, beta, idx, y = host.observation_bookkeeping(X_obs, X_obs)
Xhat = host.cubic_smoother(I, Xi); LB = host.sigma_sqs_lower_bound(Xhat)
sp0, tp0 = host.softplus_inverse_inits(hp["sigma_sqs"], np.ones(3), LB)
eng = MagiEngine(0)
eng.build_matrices(I, hp["phi1s"], hp["phi2s"], 2.01, want_host=False)
eng.set_problem(Xi.mean(axis=0), N_ds.astype(float), idx, y, beta, LB, "seir4")

rows = []
if a.kernel in ("stream", "sep"):
    for _ in range(reps):
        g, ph = eng.time_gradient(n, 3)
        rows.append(eng.debug_par(0)[40:40 + len(labels)].copy())
    head = "%s kernel %.2f us (timing launches, %d chains)" % (a.kernel, ph[4] * 1e3, n)
else:
    warm = 40 if a.kernel == "point" else 30
    cfg = eng.default_cfg(num_results=warm + 20, num_burnin_steps=warm, stale_cache=0)
    rep = (lambda v: v) if n == 1 else (lambda v: np.repeat(np.asarray(v)[None], n, axis=0))
    eng.sampler_init(cfg, rep(Xhat), rep(sp0), rep(tp0), seed=1)
    eng.sampler_run(warm)
    for _ in range(reps):
        eng.sampler_run(1)
        rows.append(eng.debug_par(0)[40:56 if labels is None else 40 + len(labels)].copy())
    head = "%s stamps inside the sampler (%d chains)" % (a.kernel, n)
rows = np.array(rows)
eng.close()

if labels is not None:
    u = rows.view(np.uint64).astype(np.int64)              # raw 100 MHz counter values; 0: the stamped wave / task does not pass there
    set_ = [k for k in range(len(labels)) if (u[:, k] != 0).all()]
    med = np.median((u - u[:, :1]) * 10.0, axis=0)
    print("%s; workgroup time line (ns from entry, median of %d), N = %d:" % (head, reps, a.n))
    for k in sorted(set_, key=lambda k: med[k]):
        print("  %-30s %7.0f" % (labels[k], med[k]))
    if len(set_) < len(labels):
        print("  not set in this workgroup / wave: " + ", ".join(labels[k] for k in range(len(labels)) if k not in set_))
else:
    # decision workgroup (decide.h; LDS-staged doubles): 8 entry, 2 first round issued, 0 state staged, 1 uniforms issued,
    # 3 partial sums added, 4 reduce done, 5 decision, 6 hot-path end; [11] / [12] raw counters of the stream workgroups
    d = lambda a_, b_: np.median((rows[:, b_] - rows[:, a_]) * 10.0)
    print("%s, N = %d, median of %d (ns):" % (head, a.n, reps))
    print("issue of the first round %.0f | its wait %.0f | ->1 %.0f | add partials %.0f | param entries %.0f | decide %.0f | publish %.0f | total %.0f" %
          (d(8, 2), d(2, 0), d(0, 1), d(1, 3), d(3, 4), d(4, 5), d(5, 6), d(8, 6)))
    # the slot after the last hot leaf: stream start [12] / latest stream workgroup end [11] (raw counters), decide entry [8] / hot end [6]
    # are of the slot BEFORE; report durations only
    u = rows.view(np.uint64)
    print("stream (first wg start -> last wg end) %.0f ns" % np.median((u[:, 11].astype(np.int64) - u[:, 12].astype(np.int64)) * 10.0))
    unset = [k for k in (0, 1, 2, 3, 4, 5, 6, 8, 11, 12) if (rows[:, k] == 0).any()]
    if unset:
        sys.exit("stamps never set: %s (is the library a -DMAGI_STAMPS=decide build?)" % unset)
if labels is not None and not set_:
    sys.exit("no stamp set (is the library a -DMAGI_STAMPS=%s build?)" % a.kernel)
