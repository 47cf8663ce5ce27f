"""The library self-test on the GPU: the drift probe against the host evaluators of the trace, the self-test on the base library and on
every example drift's library, the verdict cache across processes, and -- the point of it -- libraries whose generated drift code is
wrong are refused (wrong numbers only: every deliberately wrong header below computes finite values)."""
import dataclasses
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from magi_v2_amd import drift, selftest
from magi_v2_amd.drift_examples import EXAMPLES
from magi_v2_amd.engine import DRIFT_SHAPES, MagiEngine, MagiHipError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def the_drift(name):
    return drift.builtin_drift(name) if name in DRIFT_SHAPES else drift.resolve(*EXAMPLES[name])


@pytest.mark.parametrize("name", sorted(DRIFT_SHAPES) + sorted(EXAMPLES))
def test_drift_probe_matches_the_host_evaluators_on_every_path(name):
    """256 points in the box of drift.resolve; error per point relative to the largest magnitude of that point's output vector <= 1e-12
    (+ 1e-14): the pair drift.resolve compares drift evaluations with.  The host evaluators are within 2e-15 of 30-digit sympy values there."""
    d = the_drift(name)
    pr = selftest.synthetic_problem(d.D, d.P)
    X, th, g = pr["probe_X"], pr["probe_th"], pr["probe_g"]
    f_want = np.asarray(d.f_np(None, X, th), dtype=np.float64)
    J, T = d.jac_np(X, th)
    c_want, t_want = np.einsum("nd,ndk->nk", g, J), np.einsum("nd,ndp->np", g, T)
    eng = MagiEngine(0, drift=d)

    def err(got, want):
        return float((np.abs(got - want) / (1e-12 * np.abs(want).max(axis=1, keepdims=True) + 1e-14)).max() * 1e-12)

    worst = {}
    for path in (0, 1):
        f, c, t = eng.drift_probe(d, X, th, g, path)
        worst[f"path{path}"] = {"f": err(f, f_want), "c": err(c, c_want), "t": err(t, t_want)}
    sep = selftest._separable(d)
    assert sep == (name != "ptrans")                       # V x / (K + x) with K a parameter does not separate
    if sep:
        f, c, t = eng.drift_probe(d, X, th, None, 2)
        assert c is None and t is None
        worst["path2"] = {"f": err(f, f_want)}
    else:
        with pytest.raises(MagiHipError, match="separable"):
            eng.drift_probe(d, X, th, None, 2)
    worst["path3"] = {"f": err(eng.drift_probe(d, X, th, None, 3)[0], f_want)}
    with pytest.raises(MagiHipError):
        eng.drift_probe(d, X, th, g, 4)
    eng.close()
    print("drift probe, worst normalised error:", name, worst)
    for path, by in worst.items():
        for what, e in by.items():
            assert e <= 1e-12, (name, path, what, e)


@pytest.mark.parametrize("name", ["base"] + sorted(EXAMPLES))
def test_selftest_passes_on_the_base_library_and_on_every_example_library(name):
    if name == "base":
        rep = selftest.run(None, None, 0)
        assert rep.drifts == sorted(DRIFT_SHAPES) or set(rep.drifts) == set(DRIFT_SHAPES)
    else:
        from magi_v2_amd import jit
        d = the_drift(name)
        rep = selftest.run(jit.library_for(d), d, 0)
        assert rep.drifts == [d.name]
    print(rep.format())
    assert rep.ok and not rep.cached and rep.sha256 == selftest.file_sha256(rep.library) and "gfx950" in rep.version
    names = [c.name for c in rep.checks if c.drift == rep.drifts[0]]
    want = ["drift.f", "drift.jt", "drift.runtime"] + (["drift.sep"] if name != "ptrans" else []) + ["families", "gradient", "sampler"]
    assert names == want
    fam = next(c for c in rep.checks if c.name == "families")
    assert fam.detail.split()[:2] == ["k_stream<1>", "k_stream<2>"] and fam.detail.split()[2].startswith("k_stream_sep" if name != "ptrans" else "k_stream_mc")
    smp = next(c for c in rep.checks if c.name == "sampler")
    assert "hmc x1" in smp.detail and "nuts x5" in smp.detail
    assert rep.seconds < 30.0


CHILD = ("import sys; sys.path.insert(0, sys.argv[1]);"
         "from magi_v2_amd import drift; from magi_v2_amd.drift_examples import EXAMPLES; from magi_v2_amd.engine import MagiEngine;"
         "e = MagiEngine(0, drift=drift.resolve(*EXAMPLES['lotka_volterra'])); r = e.selftest(); e.close();"
         "print('cached' if r.cached else 'ran', r.ok)")


def test_second_engine_in_a_fresh_process_hits_the_verdict_cache():
    env = dict(os.environ)
    env["MAGI_SELFTEST"] = "force"
    first = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert first.returncode == 0 and first.stdout.strip().splitlines()[-1] == "ran True", (first.stdout, first.stderr[-1500:])
    env.pop("MAGI_SELFTEST")
    second = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, timeout=300, env=env)
    assert second.returncode == 0 and second.stdout.strip().splitlines()[-1] == "cached True", (second.stdout, second.stderr[-1500:])


def wrong_drift(name, member, new_name):
    """The traced drift `name` with ONE generated line of `member` ("f", "jt", "coefs") made wrong in the header: the right-hand side of the
    first `c[k] = ...;` line of jt / `c[d][k] = ...;` line of coefs negated, the first `o[d] = ...;` line of f scaled by 1.5.  The host
    evaluators stay those of the trace; the new name gives it a cache directory of its own."""
    d = the_drift(name)
    head, body = d.header.split(f" void {member}(", 1)
    body, tail = body.split("\n    }\n", 1)
    pat = {"f": r"^(\s*o\[\d+\] = )(.*);$", "jt": r"^(\s*c\[\d+\] = )(.*);$", "coefs": r"^(\s*c\[\d+\]\[\d+\] = )((?!0\.0;).*);$"}[member]
    new_body, n = re.subn(pat, (r"\g<1>1.5*(\2);" if member == "f" else r"\1-(\2);"), body, count=1, flags=re.M)
    assert n == 1
    return dataclasses.replace(d, name=new_name, header=head + f" void {member}(" + new_body + "\n    }\n" + tail)


@pytest.mark.parametrize("name,member,fails,passes", [
    ("fhn", "jt", {"drift.jt", "gradient"}, {"drift.f"}),
    ("lotka_volterra", "coefs", {"drift.sep", "families", "sampler"}, {"drift.f", "drift.jt", "drift.runtime", "gradient"}),
    ("fhn", "f", {"drift.f"}, {"drift.jt"})])
def test_a_library_with_wrong_drift_code_is_refused(name, member, fails, passes, monkeypatch):
    """Without the self-test these libraries load and sample without complaint."""
    from magi_v2_amd import jit
    monkeypatch.delenv("MAGI_SELFTEST", raising=False)
    bad = wrong_drift(name, member, f"{name}_wrong_{member}")
    assert bad.header != the_drift(name).header
    with pytest.raises(selftest.MagiSelfTestError) as e:
        MagiEngine(0, drift=bad)
    rep = e.value.report
    print(rep.format())
    failed = {c.name for c in rep.failed()}
    assert fails <= failed and not (passes & failed), failed
    for n in fails:
        assert n in str(e.value)
    assert os.path.exists(selftest.verdict_path(jit.library_for(bad)))
    with pytest.raises(selftest.MagiSelfTestError):                      # the failing verdict is remembered and keeps refusing
        MagiEngine(0, drift=bad)
    # the switch: the same library loads when the self-test is skipped, i.e. the refusal came from the self-test
    monkeypatch.setenv("MAGI_SELFTEST", "0")
    eng = MagiEngine(0, drift=bad)
    pr = selftest.synthetic_problem(bad.D, bad.P)
    f, c, t = eng.drift_probe(bad, pr["probe_X"], pr["probe_th"], pr["probe_g"], 0)
    assert np.isfinite(f).all() and np.isfinite(c).all() and np.isfinite(t).all()
    eng.close()
