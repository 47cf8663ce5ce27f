"""CPU tests of the boundary: the C-ABI library builds, loads, and exports every symbol that
include/magi_hip.h declares (no compute calls -- there is no GPU in the build container)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "magi_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(magi_[a-z_0-9]+)\s*\(", src)))


def option_table():
    """(name, environment variable or None) of every row of the option table in csrc/capi.hip"""
    src = open(os.path.join(ROOT, "magi_v2_amd", "csrc", "capi.hip")).read()
    table = src[src.index("const OptRow kOptions[] = {"):]
    table = table[:table.index("};")]
    return sorted((n, None if e == "nullptr" else e.strip('"')) for n, e in re.findall(r'\{"([a-z_]+)",\s*("MAGI_[A-Z_]+"|nullptr)', table))


def header_options():
    """(name, environment variable or None) of every option the comment above magi_set_option in include/magi_hip.h lists"""
    src = open(os.path.join(ROOT, "include", "magi_hip.h")).read()
    doc = src[:src.index("int magi_set_option(")]
    doc = doc[doc.rindex("/*"):]
    return sorted((n, e or None) for n, e in re.findall(r'^\s*\*\s+"([a-z_]+)"\s+(?:(MAGI_[A-Z_]+)|\(none)', doc, flags=re.M))


def test_header_lists_every_option_of_the_table():
    table = option_table()
    assert len(table) >= 12 and ("slot_budget_graphs", None) in table
    assert "fit_per_component" not in [name for name, _ in table]          # (deleted with the per-component fit path)
    assert header_options() == table


def test_library_builds_and_exports_every_declared_symbol():
    from magi_v2_amd import build, engine
    build.build_lib()
    lib = engine.load_library()
    declared = header_functions()
    assert len(declared) >= 18
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/magi_hip.h but not exported"
    # and the ctypes table binds exactly the declared set
    assert sorted(engine.exported_symbols()) == declared
    assert b"gfx950" in lib.magi_version()


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from magi_v2_amd.engine import MagiEngine, MagiHipError
    with pytest.raises(MagiHipError):
        MagiEngine(0)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "magi_v2_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, f


def test_stream_kernels_spill_no_vector_register(tmp_path):
    """The decisions of the sampler ride inlined in the streaming kernels and share their register allocation.  Since the state-sized
    boundary passes moved to the point kernel no streaming kernel spills a vector register; this pins it (the
    decision path is where round 3's register-allocation heisenbug lived).  hipcc cross-compiles without a GPU."""
    import shutil
    import subprocess
    from magi_v2_amd import build
    if shutil.which(build.hipcc()) is None:
        pytest.skip("no hipcc")
    src = os.path.join(build.CSRC, "leap.hip")
    r = subprocess.run(build.compile_command(src, ["-Rpass-analysis=kernel-resource-usage"]) + ["-c", src, "-o", str(tmp_path / "leap.o")],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    seen = 0
    for b in blocks:
        name = b.split(" [")[0]
        if "k_stream" not in name:
            continue
        seen += 1
        spills = int(re.search(r"VGPRs Spill: (\d+)", b).group(1))
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        assert spills == 0, (name, spills)
        assert occ >= 3, (name, occ)
        # round 4: no scratch reservation at all (64 B/lane until then: a `LeafPlan` kept in memory by an aggregate copy, and the spill slot of a
        # callee-saved register in dual_averaging_eval -- decide.h: plan_store, the leaf function)
        assert scratch == 0, (name, scratch)
    assert seen >= 6


def test_host_side_of_the_c_abi_is_clean_under_asan_and_ubsan():
    """SURVEY section 5 (sanitizers): csrc/capi.hip compiled with -fsanitize=address,undefined for the HOST (GPU AddressSanitizer is not
    available on this pool) and driven through everything reachable without a GPU -- creation with no device, every entry point on a
    NULL handle, the out-parameter helpers (tools/sanitize_host.py; with --gpu on a GPU box it goes on through a live handle)."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sanitize_host.py")], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "sanitizer run clean" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


FAULTY_JOIN = """
_Z6kernelv:
	v_cmp_eq_u32_e32 vcc, 0, v60
	s_and_saveexec_b64 s[2:3], vcc
	s_cbranch_execz .LBB0_5
; %bb.1:
	s_getpc_b64 s[0:1]
	s_swappc_b64 s[30:31], s[0:1]
	ds_write_b64 v2, v[0:1] offset:13968
.LBB0_5:                             ; %Flow
	v_mov_b64_e32 v[100:101], v[32:33]
	v_mov_b64_e32 v[98:99], v[28:29]
	s_or_b64 exec, exec, s[2:3]
	s_endpgm
.Lfunc_end0:
"""


def test_exec_prologue_guard_flags_the_round3_miscompile_and_the_build_is_clean(tmp_path):
    """Round 3's wrong energies (one-chain SIRW kernel) were hipcc placing live-range split copies of values that are live
    in EVERY lane in front of the `s_or_b64 exec, exec, sN` of the join block behind `if (tid == 0) shs[4] = temperature(..)`: the copies
    ran for lane 0 only.  magi_v2_amd.isa_check recognises that shape in the ISA; the build keeps every unit's ISA and fails (after one
    retry without IPRA) when it appears.  Here: the checker on the faulty shape and on its repaired form, then on every unit of the
    in-tree build."""
    from magi_v2_amd import build, isa_check
    bad = tmp_path / "bad.s"
    bad.write_text(FAULTY_JOIN)
    hits = isa_check.check_file(str(bad))
    assert len(hits) == 1 and hits[0][1] == ".LBB0_5" and [i for _, i in hits[0][2]] == ["v_mov_b64_e32 v[100:101], v[32:33]", "v_mov_b64_e32 v[98:99], v[28:29]"]
    good = tmp_path / "good.s"
    lines = FAULTY_JOIN.split("\n")
    k = next(i for i, l in enumerate(lines) if "s_or_b64 exec" in l)
    lines.insert(k - 2, lines.pop(k))                          # the restore first, the copies behind it
    good.write_text("\n".join(lines))
    assert isa_check.check_file(str(good)) == []
    spill = tmp_path / "spill.s"                               # SGPR spill lanes in front of the restore are harmless (they ignore EXEC)
    spill.write_text(FAULTY_JOIN.replace("v_mov_b64_e32 v[100:101], v[32:33]", "v_readlane_b32 s2, v165, 4").replace("v_mov_b64_e32 v[98:99], v[28:29]", "v_readlane_b32 s3, v165, 5"))
    assert isa_check.check_file(str(spill)) == []
    build.build_lib(verbose=False)
    n = 0
    for src in build.sources():
        isa = build.isa_path(os.path.join(build.HERE, "build", os.path.basename(src) + ".o"))
        assert os.path.exists(isa), isa
        assert isa_check.check_file(isa) == [], isa
        n += 1
    assert n >= 7


def test_recipe_takes_no_flags_from_the_environment(monkeypatch):
    """The product and the drift-specialised builds compile with the recipe's flags alone: MAGI_EXTRA_CFLAGS (once read by both) changes
    neither their commands nor the JIT cache key; extra flags reach a build only as an argument."""
    import types
    from magi_v2_amd import build, jit
    drift = types.SimpleNamespace(D=8, P=3)

    def commands():
        return ([build.compile_command(s) for s in build.sources()],
                [build.compile_command(s, jit.drift_flags(drift, "/x/user_drift.h")) for s in build.sources()], jit._source_digest())

    monkeypatch.delenv("MAGI_EXTRA_CFLAGS", raising=False)
    plain = commands()
    monkeypatch.setenv("MAGI_EXTRA_CFLAGS", "-DMAGI_STAMPS=decide -O0")
    assert commands() == plain
    assert all("-DMAGI_STAMPS=decide" not in c for cmds in plain[:2] for cmd in cmds for c in cmd)
    assert ["-ffp-contract=on" in c for c in plain[0]] == [os.path.basename(s) != "build.hip" for s in build.sources()]
    assert jit._source_digest(["-DX"]) != plain[2]


def test_variant_build_never_targets_the_product(monkeypatch):
    from magi_v2_amd import build
    seen = []
    monkeypatch.setattr(build, "build_library", lambda units, objdir, out, **kw: seen.append((objdir, out, kw)) or out)
    out = build.build_variant("s_decide", ["-DMAGI_STAMPS=decide"])
    objdir, out_, kw = seen[0]
    assert out == out_ == os.path.join(build.VARIANTS, "s_decide", "libmagi_hip.so") and objdir == os.path.dirname(out)
    assert os.path.abspath(out) != os.path.abspath(build.LIB) and os.path.abspath(objdir) != os.path.abspath(build.OBJDIR)
    assert kw["extra"] == ["-DMAGI_STAMPS=decide"]
    for bad in ("", ".", "..", "../magi_v2_amd", "a/b"):
        with pytest.raises(ValueError):
            build.build_variant(bad, [])
    assert len(seen) == 1
