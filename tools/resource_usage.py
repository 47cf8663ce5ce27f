"""Dev: kernel resource usage of csrc/leap.hip (hipcc -Rpass-analysis=kernel-resource-usage) + where in the ISA the scratch accesses sit.
    python tools/resource_usage.py > profiles/r03_kernel_resource_usage.txt
    python tools/resource_usage.py selftest.hip          (another unit of csrc/: the table alone)
    python tools/resource_usage.py ode.hip chain8        (the unit compiled for a traced drift of magi_v2_amd.drift_examples)"""
import re, subprocess, sys, os, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORK = tempfile.mkdtemp(prefix="magi_ru_")          # (hipcc --save-temps writes into the working directory)
os.chdir(WORK)
sys.path.insert(0, ROOT)
from magi_v2_amd import build
unit = sys.argv[1] if len(sys.argv) > 1 else "leap.hip"
src = os.path.join(build.CSRC, unit)
extra = []
if len(sys.argv) > 2:
    from magi_v2_amd import drift, drift_examples, jit
    ex = {k: v for name in dir(drift_examples) if name.endswith("EXAMPLES") for k, v in getattr(drift_examples, name).items()}
    d = drift.resolve(*ex[sys.argv[2]])
    with open(os.path.join(WORK, "user_drift.h"), "w") as fh:
        fh.write(d.header)
    extra = jit.drift_flags(d, os.path.join(WORK, "user_drift.h"))
r = subprocess.run(build.compile_command(src, extra + ["-Rpass-analysis=kernel-resource-usage"]) + ["-c", src, "-o", os.path.join(WORK, unit[:-4] + "_ru.o"), "--save-temps"],
                   capture_output=True, text=True)
if r.returncode != 0:
    sys.exit(r.stderr[-4000:])
txt = r.stderr
blocks = re.split(r"remark: [^\n]*Function Name: ", txt)[1:]
print("# hipcc -O3 --offload-arch=gfx950 -ffp-contract=on -Rpass-analysis=kernel-resource-usage magi_v2_amd/csrc/%s%s  (ROCm 7.2)" % (unit, " for the traced drift " + sys.argv[2] if extra else ""))
print("# kernel | VGPRs | VGPR spills | SGPR spills | scratch B/lane | occupancy waves/SIMD | LDS B/block")
KEYS = ["    VGPRs", "VGPRs Spill", "SGPRs Spill", r"ScratchSize \[bytes/lane\]", r"Occupancy \[waves/SIMD\]", r"LDS Size \[bytes/block\]"]
for b in blocks:
    name = b.split(" [")[0]
    dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    dem = re.sub(r"\(anonymous namespace\)::", "", dem); dem = re.sub(r"\(DevProblem.*|\(DevChains.*|\(HIP_vector.*", "", dem); dem = dem.replace("void ", "")
    vals = []
    for k in KEYS:
        m = re.search(k + r": (\d+)", b)
        vals.append(m.group(1) if m else "?")
    print("%-28s | %4s | %3s | %3s | %4s | %2s | %6s" % tuple([dem] + vals))
if unit != "leap.hip":
    sys.exit(0)
s = open(os.path.join(WORK, "leap-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
def body(sym):
    i = s.index("\n" + sym + ":"); j = s.index(".Lfunc_end", i); return s[i:j].split("\n")
print()
print("# Scratch (ISA of the same compile; line numbers inside each kernel's body).  Round 3: the state-sized boundary passes moved from the decision workgroup to the")
print("# point kernel (leap_point.h: boundary_block) and the stream kernels stopped spilling vector registers (56-116 per kernel before, all on the decision path).")
print("# Round 4: the last 64 B per lane of scratch are gone too -- 32 B were the zero tail of a `LeafPlan p{}` kept in memory by the aggregate copy `*plan_out = p`")
print("# (decide.h: plan_store writes field by field), 16 B the spill slot of a callee-saved VGPR in dual_averaging_eval (now a leaf: its log / exp / pow expand inside it).")
for sym, what in (("_ZN12_GLOBAL__N_112k_stream_sepILi1ELi8EEEv10DevProblem9DevChains13SamplerCfgDevi", "k_stream_sep<SEIR4, 8>"),
                  ("_ZN12_GLOBAL__N_18k_streamILi1ELi1EEEv10DevProblem9DevChains13SamplerCfgDevi", "k_stream<1, SEIR4>")):
    L = body(sym)
    # the streaming body: from the first burst of tile loads (>= 4 global_load_dwordx4 within 14 lines) to 300 lines behind the last burst
    idx = [i for i, l in enumerate(L) if "global_load_dwordx4" in l]
    runs = [i for i in idx if sum(1 for m in idx if i <= m < i + 14) >= 4]
    end = runs[-1] + 300          # (the last burst is followed by its steps' arithmetic and the partial-sum stores)
    sc = [i for i, l in enumerate(L) if "scratch_" in l]
    inside = [i for i in sc if runs[0] <= i <= end]
    print("%s: %d ISA lines; streaming body (first .. last burst of tile loads + 300 lines) = lines %d..%d; %d scratch accesses in the kernel, on lines %d..%d; %d of them inside the streaming body"
          % (what, len(L), runs[0], end, len(sc), sc[0] if sc else -1, sc[-1] if sc else -1, len(inside)))
