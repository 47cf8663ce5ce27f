"""The library self-test without a GPU: the probe's entry point is declared, bound, exported and compiled clean for gfx950; the verdict
cache (hit / miss / a failing verdict persists / two processes run the checks once); the report and the command line; the synthetic
problem; the engine refuses a drift-specialised library whose self-test fails."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from magi_v2_amd import selftest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fake_report(path, ok=True, drifts=("fhn",), device="Fake GPU", sha=None):
    worst = 3e-16 if ok else 2.0
    checks = [selftest.Check("drift.f", drifts[0], 2e-16, 1e-12, True, 0.001, "", {"path0.f": 2e-16}),
              selftest.Check("drift.jt", drifts[0], worst, 1e-12, ok, 0.001, "", {"path0.c": worst}),
              selftest.Check("gradient", drifts[0], 1e-8 if ok else 0.7, 1e-4, ok, 0.002)]
    return selftest.Report(library=path, sha256=sha or selftest.file_sha256(path), version="magi_hip 0.1.0 gfx950", device=device,
                           selftest_version=selftest.VERSION, drifts=list(drifts), checks=checks, seconds=0.01)


@pytest.fixture
def lib_file(tmp_path, monkeypatch):
    monkeypatch.delenv("MAGI_SELFTEST", raising=False)
    monkeypatch.setattr(selftest, "_memory", {})
    p = tmp_path / "libmagi_hip_user.0123456789.so"
    p.write_bytes(b"not really a library, only bytes with a digest")
    return str(p)


class Runner:
    def __init__(self, ok=True):
        self.calls, self.ok = 0, ok

    def __call__(self, path, drift, device):
        self.calls += 1
        return fake_report(path, self.ok)


def test_probe_entry_is_declared_bound_and_exported():
    from magi_v2_amd import build, engine
    hdr = open(os.path.join(ROOT, "include", "magi_hip.h")).read()
    assert re.search(r"int magi_drift_probe\(magi_handle\* h, int drift_id, int P, int path, int n,\s*const double\* x, const double\* th, "
                     r"const double\* g,\s*double\* f, double\* c, double\* t\);", hdr)
    assert "magi_drift_probe" in engine.exported_symbols()
    assert len(engine._SYMBOLS["magi_drift_probe"][1]) == 11
    build.build_lib()
    assert hasattr(engine.load_library(), "magi_drift_probe")
    assert hasattr(engine.MagiEngine, "drift_probe") and hasattr(engine.MagiEngine, "selftest")


def test_probe_unit_is_drift_dependent_and_compiles_clean_for_gfx950():
    """selftest.hip is rebuilt for every traced drift (not in jit._DRIFT_FREE), passes the EXEC-prologue guard, and tools/resource_usage.py
    shows every k_drift_probe instantiation (3 compiled-in drifts x 4 paths) without scratch or spills."""
    from magi_v2_amd import build, isa_check, jit
    if shutil.which(build.hipcc()) is None:
        pytest.skip("no hipcc")
    assert "selftest.hip" not in jit._DRIFT_FREE
    assert os.path.join(build.CSRC, "selftest.hip") in build.sources()
    build.build_lib(verbose=False)
    isa = build.isa_path(os.path.join(build.OBJDIR, "selftest.hip.o"))
    assert os.path.exists(isa) and isa_check.check_file(isa) == []
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py"), "selftest.hip"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [[c.strip() for c in line.split("|")] for line in r.stdout.splitlines() if "k_drift_probe" in line]
    assert len(rows) == 12, r.stdout
    for name, vgprs, vspill, sspill, scratch, occ, lds in rows:
        assert (vspill, sspill, scratch, lds) == ("0", "0", "0", "0"), (name, vspill, sspill, scratch, lds)


def test_verdict_is_cached_beside_the_library_and_keyed_by_bytes_device_and_version(lib_file, monkeypatch):
    run = Runner()
    dev = lambda k: "Fake GPU"
    rep = selftest.ensure(lib_file, "fhn", 0, runner=run, get_device_name=dev)
    assert run.calls == 1 and rep.ok and not rep.cached
    vpath = selftest.verdict_path(lib_file)
    assert vpath == lib_file + ".selftest.json" and os.path.exists(vpath)
    import fnmatch
    assert not fnmatch.fnmatch(os.path.basename(vpath), "libmagi_hip_user.*.so")          # (what jit._find_cached_library globs)
    assert not [f for f in os.listdir(os.path.dirname(lib_file)) if f.endswith(".tmp")]
    on_disk = json.load(open(vpath))
    assert on_disk["sha256"] == selftest.file_sha256(lib_file) and on_disk["device"] == "Fake GPU" and on_disk["selftest_version"] == selftest.VERSION
    # same process: memory; a fresh process (memory emptied): the file
    assert selftest.ensure(lib_file, "fhn", 0, runner=run, get_device_name=dev) is rep and run.calls == 1
    monkeypatch.setattr(selftest, "_memory", {})
    again = selftest.ensure(lib_file, "fhn", 0, runner=run, get_device_name=dev)
    assert run.calls == 1 and again.cached and again.ok and "(cached)" in again.format()
    # another device name
    monkeypatch.setattr(selftest, "_memory", {})
    selftest.ensure(lib_file, "fhn", 0, runner=lambda p, d, k: fake_report(p, device="Other GPU"), get_device_name=lambda k: "Other GPU")
    monkeypatch.setattr(selftest, "_memory", {})
    selftest.ensure(lib_file, "fhn", 0, runner=run, get_device_name=dev)
    assert run.calls == 2
    # another self-test version
    monkeypatch.setattr(selftest, "_memory", {})
    monkeypatch.setattr(selftest, "VERSION", selftest.VERSION + 1)
    selftest.ensure(lib_file, "fhn", 0, runner=run, get_device_name=dev)
    assert run.calls == 3
    # other bytes
    monkeypatch.setattr(selftest, "_memory", {})
    with open(lib_file, "ab") as fh:
        fh.write(b"!")
    selftest.ensure(lib_file, "fhn", 0, runner=run, get_device_name=dev)
    assert run.calls == 4
    # MAGI_SELFTEST=force ignores memory and file; MAGI_SELFTEST=0 runs and reads nothing
    monkeypatch.setenv("MAGI_SELFTEST", "force")
    assert not selftest.ensure(lib_file, "fhn", 0, runner=run, get_device_name=dev).cached and run.calls == 5
    monkeypatch.setenv("MAGI_SELFTEST", "0")
    assert selftest.ensure(lib_file, "fhn", 0, runner=run, get_device_name=dev) is None and run.calls == 5


def test_failing_verdict_persists_and_keeps_raising(lib_file, monkeypatch):
    run = Runner(ok=False)
    dev = lambda k: "Fake GPU"
    with pytest.raises(selftest.MagiSelfTestError) as e:
        selftest.ensure(lib_file, "fhn", 0, runner=run, get_device_name=dev)
    assert isinstance(e.value, RuntimeError) and not e.value.report.ok
    msg = str(e.value)
    assert "drift.jt" in msg and "gradient" in msg and "drift.f " not in msg and "2.000e+00" in msg and "1.0e-12" in msg and lib_file in msg
    monkeypatch.setattr(selftest, "_memory", {})
    good = Runner(ok=True)
    with pytest.raises(selftest.MagiSelfTestError) as e2:                                   # the stored verdict refuses; nothing is run again
        selftest.ensure(lib_file, "fhn", 0, runner=good, get_device_name=dev)
    assert good.calls == 0 and e2.value.report.cached
    assert selftest.ensure(lib_file, "fhn", 0, force=True, runner=good, get_device_name=dev).ok and good.calls == 1


def test_read_only_directory_keeps_the_verdict_in_memory(lib_file, monkeypatch):
    real_open = open

    def no_write(path, mode="r", *a, **kw):
        if "selftest" in str(path) and ("w" in mode or "a" in mode):
            raise PermissionError(13, "read-only", str(path))
        return real_open(path, mode, *a, **kw)

    monkeypatch.setattr("builtins.open", no_write)
    run = Runner()
    dev = lambda k: "Fake GPU"
    assert selftest.ensure(lib_file, "fhn", 0, runner=run, get_device_name=dev).ok
    assert selftest.ensure(lib_file, "fhn", 0, runner=run, get_device_name=dev).ok
    assert run.calls == 1 and not os.path.exists(selftest.verdict_path(lib_file))


RACER = """
import sys, time
sys.path.insert(0, sys.argv[2])
sys.path.insert(0, sys.argv[2] + "/tests")
from magi_v2_amd import selftest
from test_selftest_cpu import fake_report
def runner(path, drift, device):
    with open(sys.argv[3], "a") as fh:
        fh.write("ran\\n")
    time.sleep(1.0)
    return fake_report(path)
rep = selftest.ensure(sys.argv[1], "fhn", 0, runner=runner, get_device_name=lambda k: "Fake GPU")
print("cached" if rep.cached else "ran")
"""


def test_two_processes_racing_on_one_library_run_the_checks_once(lib_file, tmp_path):
    count = str(tmp_path / "count.txt")
    env = {k: v for k, v in os.environ.items() if k != "MAGI_SELFTEST"}
    procs = [subprocess.Popen([sys.executable, "-c", RACER, lib_file, ROOT, count], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env) for _ in range(2)]
    outs = [p.communicate(timeout=120) for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1].decode()[-800:] for o in outs]
    assert open(count).read().splitlines() == ["ran"]
    assert sorted(o[0].decode().strip().splitlines()[-1] for o in outs) == ["cached", "ran"]


def test_report_format_and_command_line_exit_status(lib_file, capsys):
    dev = lambda k: "Fake GPU"
    assert selftest.main(["--lib", lib_file, "--drift", "seir4"], runner=lambda p, d, k: fake_report(p, drifts=("seir4",)), get_device_name=dev) == 0
    out = capsys.readouterr().out
    assert lib_file in out and selftest.file_sha256(lib_file) in out and "magi_hip 0.1.0 gfx950 on Fake GPU" in out and f"self-test v{selftest.VERSION}" in out
    for name in ("drift.f", "drift.jt", "gradient"):
        assert re.search(rf"^\s+{re.escape(name)}\s+seir4\s+\S+e[-+]\d+\s+1\.0e-\d+\s+\d+\.\d+\s+ok", out, flags=re.M), (name, out)
    assert "PASSED" in out and "FAILED" not in out
    # a failing library: exit status 1, the report on stdout, the refusal on stderr; --force runs although a verdict is stored
    bad = Runner(ok=False)
    assert selftest.main(["--lib", lib_file, "--drift", "seir4", "--force"], runner=bad, get_device_name=dev) == 1 and bad.calls == 1
    cap = capsys.readouterr()
    assert re.search(r"drift\.jt\s+\S+\s+2\.000e\+00\s+1\.0e-12\s+\S+\s+FAILED", cap.out) and "FAILED in" in cap.out
    assert "drift.jt" in cap.err and "gradient" in cap.err and "not used" in cap.err
    assert selftest.main(["--lib", lib_file, "--drift", "seir4"], runner=bad, get_device_name=dev) == 1 and bad.calls == 1          # the stored verdict
    rep = fake_report(lib_file)
    assert selftest.Report.from_json(json.loads(json.dumps(rep.to_json())), cached=False) == rep


def test_synthetic_problem_is_deterministic_in_range_and_needs_no_oracle():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); from magi_v2_amd import selftest;"
            "a, b = selftest.synthetic_problem(2, 3), selftest.synthetic_problem(2, 3);"
            "assert sorted(a) == sorted(b) and all(a[k].tobytes() == b[k].tobytes() and a[k].dtype == b[k].dtype for k in a);"
            "assert not [m for m in sys.modules if m == 'oracle' or m.startswith('oracle.')]; print('ok')")
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-1500:]
    for D, P in ((2, 3), (5, 6), (4, 5)):
        pr = selftest.synthetic_problem(D, P)
        N = selftest.N_GRID
        assert N == 161 and pr["I"].shape == (N,) and np.allclose(np.diff(pr["I"]), pr["I"][1])           # uniform, more than one 128-point block
        assert pr["X0"].shape == (N, D) and 0.05 < pr["X0"].min() and pr["X0"].max() < 0.6
        assert pr["state_X"].shape == (3, N, D) and 0.05 < pr["state_X"].min() and pr["state_X"].max() < 0.6
        th = np.log1p(np.exp(np.concatenate([pr["tp0"][None], pr["state_tp"]])))
        assert 0.2 < th.min() and th.max() < 2.0
        assert pr["probe_X"].shape == (256, D) and 0.05 <= pr["probe_X"].min() and pr["probe_X"].max() <= 0.6
        assert pr["probe_th"].shape == (P,) and 0.2 <= pr["probe_th"].min() and pr["probe_th"].max() <= 2.0
        rows = np.unique(pr["obs_idx"] // D)
        assert np.array_equal(rows, np.arange(0, N, 2)) and len(pr["obs_idx"]) == 81 * D and pr["dir_X"].shape == (4, N, D)


def test_engine_refuses_a_specialised_library_whose_selftest_fails(tmp_path, monkeypatch):
    """MagiEngine(drift=<traced drift>) asks selftest.ensure before the library is loaded; a failure propagates and nothing is loaded.  A
    built-in drift never asks."""
    from magi_v2_amd import drift, engine, jit
    from magi_v2_amd.drift_examples import EXAMPLES
    d = drift.resolve(*EXAMPLES["fhn"])
    lib = str(tmp_path / "libmagi_hip_user.x.so")
    open(lib, "wb").write(b"bytes")
    asked, loaded = [], []
    monkeypatch.setattr(jit, "library_for", lambda dr, **kw: lib)
    monkeypatch.setattr(engine, "load_library", lambda path=None: loaded.append(path) or (_ for _ in ()).throw(AssertionError("loaded")))

    def refuse(path, dr, device, **kw):
        asked.append((path, dr.name, device))
        raise selftest.MagiSelfTestError(fake_report(path, ok=False, drifts=(dr.name,)))

    monkeypatch.setattr(selftest, "ensure", refuse)
    with pytest.raises(selftest.MagiSelfTestError, match="drift.jt"):
        engine.MagiEngine(0, drift=d)
    assert asked == [(lib, d.name, 0)] and loaded == []
    with pytest.raises(AssertionError, match="loaded"):                    # the base library: loaded without a question
        engine.MagiEngine(0, drift=drift.builtin_drift("seir4"))
    assert len(asked) == 1 and loaded == [None]
