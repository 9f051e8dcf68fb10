"""Register, scratch and LDS budgets of the built kernels, read from the code object inside the library (no GPU needed): a guard against the
kind of regression round 6 found twice — row addresses hoisted out of a loop and spilled (948 B of scratch in the ground-capable Cessna172Xv2
pass, 1 168 B in k_trim), which costs nothing in correctness and a great deal in time (profiles/r06_ground_launch_anatomy.txt, r06_ab_trim.txt)."""
import re

import pytest

from support import library_kernels


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return library_kernels(tmp_path_factory)


def test_every_stepping_instance_is_in_the_library(kernels):
    for kin in (0, 1, 2):
        for x in ("false", "true"):
            for env in ("false", "true"):
                assert f"fbd::k_step_duo<{kin}, {x}, {env}>" in kernels
                for gnd in ("false", "true"):
                    assert f"fbd::k_step_air<{kin}, {x}, {gnd}, {env}>" in kernels
    assert "fbf::k_step_f32" in kernels and "fbd::k_trim<false>" in kernels and "fbd::k_trim<true>" in kernels and "fbd::k_scenario<0>" in kernels


def test_stepping_instances_are_exactly_the_dispatch_matrix(kernels):
    """launch_step (csrc/fb_capi.hip) instantiates 12 k_step_duo, 24 k_step_air and the one fp32 stepper: the 37 instances whose table
    heads tests/test_gpu_dispatch_matrix.py. An instance added to or lost from the dispatcher fails here, without a GPU — and an added one
    needs a case there."""
    tf = ("false", "true")
    want = {f"fbd::k_step_duo<{kin}, {x}, {env}>" for kin in (0, 1, 2) for x in tf for env in tf}
    want |= {f"fbd::k_step_air<{kin}, {x}, {gnd}, {env}>" for kin in (0, 1, 2) for x in tf for gnd in tf for env in tf}
    want |= {"fbf::k_step_f32"}
    assert len(want) == 37
    have = {name for name in kernels if re.search(r"\bk_step_", name)}
    assert have == want, f"not in the table: {sorted(have - want)}; missing from the library: {sorted(want - have)}"


def test_budgets(kernels):
    for name, k in kernels.items():
        assert k["lds"] <= 160 * 1024, (name, k)
        m = re.match(r"fbd::k_step_duo<(\d), (true|false), (true|false)>", name)
        if m:   # two waves per SIMD: 256 registers; no scratch to speak of (a few launch-level values in the environment-row instances)
            assert k["vgpr"] <= 256, (name, k)
            assert k["scratch"] <= (48 if m.group(3) == "true" else 8), (name, k)
            continue
        m = re.match(r"fbd::k_step_air<(\d), (true|false), (true|false), (true|false)>", name)
        if m:
            x, gnd = m.group(2) == "true", m.group(3) == "true"
            limit = 0 if not x else (400 if gnd else 64)   # Cessna172Sv0: none; Xv2 ground-capable: 0.3-0.4 KB, none of it per evaluation but 1-3 reloads
            assert k["scratch"] <= limit, (name, k, limit)
            continue
        if name.startswith("fbd::k_trim"):
            assert k["scratch"] <= 512, (name, k)   # 1 168 / 1 280 B up to round 6
            continue
        assert k["scratch"] == 0, (name, k)
    assert kernels["fbd::k_step_duo<0, false, false>"]["scratch"] == 0 and kernels["fbf::k_step_f32"]["scratch"] == 0, "the headline kernels"
