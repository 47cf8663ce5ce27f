"""Problem groups without a GPU: the C entry point is declared and exported, the group kernels are compiled for gfx950 without spills or
scratch, and predict_many's partition rule (which models share a group, which run alone, in which order)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_create_is_declared_bound_and_exported():
    from magi_v2_amd import build, engine
    hdr = open(os.path.join(ROOT, "include", "magi_hip.h")).read()
    assert re.search(r"int magi_group_create\(magi_handle\* const\* members, int n_members, magi_handle\*\* out\);", hdr)
    assert "magi_group_create" in engine.exported_symbols()
    build.build_lib()
    assert hasattr(engine.load_library(), "magi_group_create")


def test_group_kernels_are_instantiated_without_spills_or_scratch(tmp_path):
    """k_stream_group<NC = 1, 2> and k_point_group for every compiled-in drift (seir4 among them), held to the rule the streaming kernels
    keep (tests/test_library_cpu.py): no spilled vector register, occupancy >= 3, no scratch."""
    from magi_v2_amd import build
    if shutil.which(build.hipcc()) is None:
        pytest.skip("no hipcc")
    src = os.path.join(build.CSRC, "leap_group.hip")
    r = subprocess.run(build.compile_command(src, ["-Rpass-analysis=kernel-resource-usage"]) + ["-c", src, "-o", str(tmp_path / "g.o")],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    seen = set()
    for b in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]:
        name = b.split(" [")[0].strip()
        m = re.search(r"(k_stream_group|k_point_group)ILi(\d+)E(?:Li(\d+)E)?", name)
        if not m:
            continue
        spills = int(re.search(r"VGPRs Spill: (\d+)", b).group(1))
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        assert spills == 0 and scratch == 0, (name, spills, scratch)
        if m.group(1) == "k_stream_group":
            assert occ >= 3, (name, occ)
            seen.add(("stream", int(m.group(2)), int(m.group(3))))
        else:
            seen.add(("point", int(m.group(2))))
    seir4 = 1                                   # MAGI_DRIFT_SEIR4
    assert {("stream", 1, seir4), ("stream", 2, seir4), ("point", seir4)} <= seen, seen


class _Eng:
    def __init__(self, lib, device=0, kernel="k_stream<2>"):
        self._lib, self.device, self.kernel = lib, device, kernel

    def stream_kernel_name(self, n_chains):
        return self.kernel


class _Model:
    """What group_key reads of a MAGI_v2 model."""
    def __init__(self, eng, N=161, D=4, P=3, drift="seir4", band=80):
        self.engine, self.mag_I, self.D, self.D_thetas, self.BANDSIZE = eng, N, D, P, band
        self.drift = type("Drift", (), {"name": drift})()


def test_predict_many_partition_groups_by_library_device_and_shape_in_order():
    from magi_v2_amd.api import group_key, partition_for_groups
    lib, other = object(), object()
    models = [_Model(_Eng(lib)),                                  # 0  group A
              _Model(_Eng(lib), N=321),                           # 1  alone: its N is nobody else's
              _Model(_Eng(lib)),                                  # 2  group A
              _Model(_Eng(lib, kernel="k_stream_sep<CW=16>")),    # 3  alone: its own rule picks a matrix-core kernel
              _Model(_Eng(lib), band=40),                         # 4  group B
              _Model(_Eng(other)),                                # 5  alone: another library (another traced drift)
              _Model(_Eng(lib, device=1)),                        # 6  alone: another GPU
              _Model(_Eng(lib)),                                  # 7  group A
              _Model(_Eng(lib), band=40)]                         # 8  group B
    keys = [group_key(m, 8) for m in models]
    assert keys[3] is None
    assert partition_for_groups(keys) == [[0, 2, 7], [1], [3], [4, 8], [5], [6]]
    assert partition_for_groups([]) == []
    assert partition_for_groups([None, None]) == [[0], [1]]


def test_predict_many_is_exported_by_the_package_and_the_drop_in():
    import magi_v2
    import magi_v2_amd
    assert magi_v2.predict_many is magi_v2_amd.predict_many
