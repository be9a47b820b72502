"""The builds of the step kernel that run several TTIs per launch carry the branch around the observation tail (option "lean_tail",
DESIGN.md 4.1): the shipped code object's own metadata, read the way tests/test_kernel_resources.py reads it, says that none of
them has scratch or a spilled vector register and that each stays inside the register budget of the waves per SIMD it is launched
for -- the members builds within 96 VGPRs at row widths 8 and 10, the 16-wide rows within their 4-waves budget.  (The two options need
a handle, and a handle needs a device: their defaults are asserted in tests/test_gpu_lean_tail.py.)"""
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

# every build whose loop hands step_body a "last TTI of the launch" flag: <kernel name pattern> -> VGPR limit
MULTI_TTI_BUILDS = [
    (r"ranenv_core_kernel_members<(8|10)>", 96), (r"ranenv_core_kernel_members<16>", 128),
    (r"ranenv_persist_kernel_members<(8|10)>", 96), (r"ranenv_persist_kernel_members<16>", 128),
    (r"ranenv_persist_kernel<(true|false), (8|10)>", 96), (r"ranenv_persist_kernel<(true|false), 16>", 128),
    (r"ranenv_persist_kernel_tiny<(8|10|16)>", 256),
    (r"ranenv_core_kernel<(0|4), (8|10), true>", 96), (r"ranenv_core_kernel<(0|4), 16, true>", 128),
    (r"ranenv_core_kernel_gather<(0|4), (8|10), true>", 96), (r"ranenv_core_kernel_gather<(0|4), 16, true>", 128),
    (r"ranenv_core_kernel_small<0, (8|10|16), true>", 128),
    (r"ranenv_core_kernel_mixed<(8|10), true, (true|false)>", 96), (r"ranenv_core_kernel_mixed<16, true, (true|false)>", 128),
    (r"ranenv_core_kernel_packed<8, true, (true|false)>", 128),
]


@pytest.fixture(scope="module")
def kernels():
    from intent_radio_sched_multi_slice_amd.csrc import build as hip_build
    import kernel_resources
    hip_build.build()
    return {k["name"]: k for k in kernel_resources.kernel_resources()}


@pytest.mark.parametrize("pattern,limit", MULTI_TTI_BUILDS)
def test_multi_tti_builds_keep_their_budgets(kernels, pattern, limit):
    names = [n for n in kernels if re.fullmatch(pattern, n)]
    assert names, (pattern, sorted(kernels)[:8])
    for n in names:
        k = kernels[n]
        assert k.get("private_segment_fixed_size", 0) == 0 and k.get("vgpr_spill_count", 0) == 0, (n, k)
        assert k.get("agpr_count", 0) == 0 and k["vgpr_count"] <= limit, (n, k["vgpr_count"], limit)


def test_the_headline_builds_are_there(kernels):
    for n in ("ranenv_core_kernel_members<10>", "ranenv_persist_kernel_members<10>"):
        assert n in kernels and kernels[n]["vgpr_count"] <= 96 and kernels[n]["private_segment_fixed_size"] == 0, (n, kernels.get(n))


def test_the_header_documents_both_options():
    text = open(os.path.join(REPO, "include", "ranenv.h")).read()
    assert '"lean_tail"' in text and '"last_rollout_lean_ttis"' in text and "RANENV_LEAN_TAIL" in text
