"""Dev: what the library self-test (magi_v2_amd/selftest.py) measures and costs on the GPU box.
    python tools/exp_selftest.py OUT.json          -> profiles/r06_selftest.json
Per drift (the three compiled-in ones on the base library, the four example drifts on their own libraries): the worst normalised error of
the drift probe per path and output, every check's worst error, and the self-test's wall time (second run of the process: the first also
loads the library's code objects).  For a 2-component and the 5-component example: the wall time of that drift's hipcc build through
jit.library_for into an empty cache on the same box -- what a user already waits for on first use."""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BUILD = ("fhn", "ptrans")


def main(out):
    from magi_v2_amd import drift, jit, selftest
    from magi_v2_amd.drift_examples import EXAMPLES
    from magi_v2_amd.engine import DRIFT_SHAPES, LIB_PATH
    res = {"selftest_version": selftest.VERSION, "drifts": {}}
    jobs = [(n, LIB_PATH, drift.builtin_drift(n)) for n in sorted(DRIFT_SHAPES)]
    for n in sorted(EXAMPLES):
        d = drift.resolve(*EXAMPLES[n])
        jobs.append((n, jit.library_for(d), d))
    for n, lib, d in jobs:
        first = selftest.run(lib, d, 0, raise_on_failure=False)
        rep = selftest.run(lib, d, 0, raise_on_failure=False)
        res["device"] = rep.device
        res["drifts"][n] = {"D": d.D, "P": d.P, "ok": rep.ok, "selftest_seconds": rep.seconds, "selftest_seconds_first_run": first.seconds,
                            "probe_worst_normalised_error": {k: v for c in rep.checks if c.name.startswith("drift.") for k, v in c.by_path.items()},
                            "checks": {c.name: {"worst": c.worst, "tolerance": c.tol, "seconds": c.seconds, "detail": c.detail} for c in rep.checks}}
        print(rep.format(), flush=True)
    with tempfile.TemporaryDirectory() as tmp:              # an empty cache: the build a first use pays
        jit.CACHE, jit._DRIFT_FREE = tmp, ()            # (every unit compiled: the objects of the base build need not be on this box)
        for n in BUILD:
            d = drift.resolve(*EXAMPLES[n])
            t0 = time.perf_counter()
            jit.library_for(d)
            res["drifts"][n]["jit_build_seconds"] = time.perf_counter() - t0
            print(n, "hipcc build", res["drifts"][n]["jit_build_seconds"], "s", flush=True)
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)
    return 0 if all(v["ok"] for v in res["drifts"].values()) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
