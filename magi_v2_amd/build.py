"""Build libmagi_hip.so (hipcc, gfx950) in-tree.  Used by __graft_entry__.build() and by hand:
    python -m magi_v2_amd.build [--force]
This is the library's one compile recipe: the product, the drift-specialised builds (jit.py), the host-sanitizer build
(tools/sanitize_host.py) and the dev variants all take their hipcc commands from compile_command and build through build_library.
A dev variant (device time stamps, csrc/stamps.h; tuning switches) never touches the product:
    python -m magi_v2_amd.build --variant NAME [-DFLAG ...]   ->  build_variants/NAME/libmagi_hip.so   (select with MAGI_HIP_LIB)
"""
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libmagi_hip.so")
OBJDIR = os.path.join(HERE, "build")
VARIANTS = os.path.join(os.path.dirname(HERE), "build_variants")
FLAGS_FILE = "flags.txt"          # beside the objects: the extra flags they were compiled with, one per line
BACKEND_REJECTS = b"Illegal instruction detected"          # the machine verifier's words when the code generator emits an instruction it may not
BASE_FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-Wall", "-Wno-unused-function"]


def hipcc():
    return os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def headers():
    return glob.glob(os.path.join(CSRC, "*.h")) + [os.path.join(HERE, "..", "include", "magi_hip.h")]


def compile_command(src, extra=()):
    """The hipcc command (without -c / -o / --save-temps) for one translation unit; `extra` flags go last."""
    # -ffp-contract=on: fused multiply-adds are formed per source expression (front end), not by the optimiser, so
    # every instantiation of a kernel (1, 2, 4 chains per matrix pass) rounds a chain's arithmetic identically
    contract = [] if os.path.basename(src) == "build.hip" else ["-ffp-contract=on"]     # (the matrix build keeps the default)
    return [hipcc()] + BASE_FLAGS + contract + list(extra)


def _built_flags(objdir):
    try:
        with open(os.path.join(objdir, FLAGS_FILE)) as fh:
            return fh.read()
    except OSError:
        return None


def needs_build():
    if not os.path.exists(LIB) or _built_flags(OBJDIR) != "":
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(p) > t for p in sources() + headers())


def isa_path(obj):
    """The device ISA hipcc leaves beside an object compiled with --save-temps=obj (<dir>/<stem>-hip-amdgcn-amd-amdhsa-gfx950.s)."""
    stem = os.path.basename(obj)
    stem = stem[:-2] if stem.endswith(".o") else stem           # leap.hip.o -> leap.hip
    stem = stem[:-4] if stem.endswith(".hip") else stem         # -> leap
    return os.path.join(os.path.dirname(obj), stem + "-hip-amdgcn-amd-amdhsa-gfx950.s")


def compile_checked(jobs, verbose=True):
    """jobs: [(command without -o/--save-temps, source, object)].  Compiles them in parallel keeping each unit's device ISA, runs the
    EXEC-prologue check (isa_check.py: the round-3 miscompile put live-range copies in front of a join block's EXEC restore)
    and recompiles a flagged unit with -mllvm -enable-ipra=false -- one of the switches that removed the pattern -- before giving up."""
    from . import isa_check

    def launch(cmd, src, obj, extra):
        full = cmd + extra + ["--save-temps=obj", "-c", src, "-o", obj]
        if verbose:
            print(" ".join(full), flush=True)
        return full, subprocess.Popen(full, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)

    running = [(job, launch(*job, [])) for job in jobs]
    for (cmd, src, obj), (full, p) in running:
        out, _ = p.communicate()
        retried = False
        if p.returncode != 0 and BACKEND_REJECTS in out:
            # the code generator refuses its own output (met with a traced drift that calls pow() seven times, none of them inlined:
            # "V_CMP_NE_U32_e32 0, $src_shared_base" in leap_group.hip); without interprocedural register allocation it does not
            print(f"[magi build] {os.path.basename(src)}: the code generator rejected its own output -- recompiling with -mllvm -enable-ipra=false\n"
                  + out.decode(errors="replace")[-600:], flush=True)
            full, p = launch(cmd, src, obj, ["-mllvm", "-enable-ipra=false"])
            out, _ = p.communicate()
            retried = True
        if p.returncode != 0:
            raise RuntimeError("hipcc failed: " + " ".join(full) + "\n" + out.decode(errors="replace")[-4000:])
        hits = isa_check.check_file(isa_path(obj)) if os.path.exists(isa_path(obj)) else None
        if hits is None:
            raise RuntimeError(f"no device ISA beside {obj}: the EXEC-prologue check cannot run")
        if hits and retried:
            raise RuntimeError("hipcc placed vector instructions in front of a join block's EXEC restore (DESIGN.md 4.2) in a unit that only compiles "
                               "without IPRA:\n" + isa_check.report(isa_path(obj), hits))
        if hits:
            print(f"[magi build] {os.path.basename(src)}: instructions in front of an EXEC restore -- recompiling with -mllvm -enable-ipra=false\n"
                  + isa_check.report(isa_path(obj), hits), flush=True)
            full, p = launch(cmd, src, obj, ["-mllvm", "-enable-ipra=false"])
            out, _ = p.communicate()
            if p.returncode != 0:
                raise RuntimeError("hipcc failed: " + " ".join(full) + "\n" + out.decode(errors="replace")[-4000:])
            hits = isa_check.check_file(isa_path(obj))
            if hits:
                raise RuntimeError("hipcc placed vector instructions in front of a join block's EXEC restore (they run under the narrowed mask of the "
                                   "skipped region: wrong results, DESIGN.md 4.2), with and without IPRA:\n" + isa_check.report(isa_path(obj), hits))
        stem = os.path.basename(isa_path(obj)).rsplit("-hip-", 1)[0]
        for junk in glob.glob(os.path.join(os.path.dirname(obj), stem + "-*")) + glob.glob(os.path.join(os.path.dirname(obj), stem + ".hip-*")):
            if junk != isa_path(obj):            # keep the device ISA (checked above), drop the other intermediate files of --save-temps
                os.remove(junk)


def build_library(units, objdir, out, extra=(), reuse=None, link_flags=(), force=False, verbose=True):
    """Compiles `units` (csrc/*.hip) with compile_command(unit, extra) into `objdir` through compile_checked and links them into `out`;
    reuse = {unit: object} are linked as they are.  An object is recompiled when it is older than its source or a header, or when
    `extra` is not the flag list it was compiled with (FLAGS_FILE in `objdir`)."""
    reuse = reuse or {}
    os.makedirs(objdir, exist_ok=True)
    flags = "\n".join(extra)
    stale = force or _built_flags(objdir) != flags
    objs, jobs = [], []
    for src in units:
        if src in reuse:
            objs.append(reuse[src])
            continue
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        objs.append(obj)
        if (not stale and os.path.exists(obj) and os.path.exists(isa_path(obj))
                and all(os.path.getmtime(obj) > os.path.getmtime(p) for p in [src] + headers())):
            continue
        jobs.append((compile_command(src, extra), src, obj))
    compile_checked(jobs, verbose)
    with open(os.path.join(objdir, FLAGS_FILE), "w") as fh:
        fh.write(flags)
    if jobs or not os.path.exists(out) or any(os.path.getmtime(o) > os.path.getmtime(out) for o in objs):
        cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC"] + list(link_flags) + ["-o", out] + objs + ["-Wl,-rpath,/opt/rocm/lib"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return out


def build_lib(force=False, verbose=True):
    """The product library: the recipe with no extra flags (it takes none from the environment)."""
    if not force and not needs_build():
        return LIB
    return build_library(sources(), OBJDIR, LIB, force=force, verbose=verbose)


def variant_dir(name):
    if not name or name in (".", "..") or os.sep in name or (os.altsep and os.altsep in name):
        raise ValueError(f"variant name {name!r}: one plain directory name under build_variants/")
    return os.path.join(VARIANTS, name)


def build_variant(name, extra, force=False, verbose=True):
    """Every unit compiled with `extra` into build_variants/NAME/: objects, each unit's device ISA, libmagi_hip.so.  Never the product."""
    d = variant_dir(name)
    out = os.path.join(d, "libmagi_hip.so")
    assert os.path.abspath(out) != os.path.abspath(LIB)
    return build_library(sources(), d, out, extra=extra, force=force, verbose=verbose)


if __name__ == "__main__":
    args = sys.argv[1:]
    force = "--force" in args
    args = [a for a in args if a != "--force"]
    if args[:1] == ["--variant"] and len(args) >= 2:
        print(build_variant(args[1], args[2:], force=force))
    elif not args:
        print(build_lib(force=force))
    else:
        sys.exit("usage: python -m magi_v2_amd.build [--force]  |  python -m magi_v2_amd.build [--force] --variant NAME [-DFLAG ...]")
