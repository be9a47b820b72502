"""The state of a launch's inner TTIs (option "lean_state") without a device: the option, its environment variable and
its counter are documented in the header and the host presets the option to 1 (a handle needs a device: the value read back from one
is asserted in tests/test_gpu_lean_state.py); the ablation value -DRANENV_DIAG=13 compiles in the two translation units that read it; and
the rebuilt library keeps the limits of tests/test_kernel_resources.py -- that file's own tests, run here as they are -- with the members
builds, which now hand seven more words per lane from TTI to TTI, inside 96 VGPRs at row widths 8 and 10."""
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "intent_radio_sched_multi_slice_amd", "csrc")
sys.path.insert(0, os.path.join(REPO, "tools"))


def test_the_header_documents_the_option_and_the_counter():
    text = open(os.path.join(REPO, "include", "ranenv.h")).read()
    assert '"lean_state"' in text and "RANENV_LEAN_STATE" in text and '"last_rollout_kept_state_ttis"' in text


def test_the_option_defaults_to_on_and_sits_in_padding():
    host = open(os.path.join(CSRC, "ranenv_host.cpp")).read()
    assert re.search(r"\bkp\.lean_state = 1;", host)
    assert re.search(r'\{"lean_state", true,', host)                 # (true: RANENV_LEAN_STATE presets it)
    internal = open(os.path.join(CSRC, "ranenv_internal.h")).read()
    assert "offsetof(KP, trf_pool) - offsetof(KP, lean_state) == 4" in internal and "offsetof(KP, lean_state) - offsetof(KP, se_rp) == 4" in internal


@pytest.mark.parametrize("source,extra", [("ranenv_step.hip", ("-DRANENV_NP=10",)), ("ranenv_host.cpp", ())])
def test_the_ablation_value_compiles(source, extra):
    from intent_radio_sched_multi_slice_amd.csrc import build as hip_build
    cmd = [hip_build.hipcc_path(), *hip_build.CFLAGS, *extra, "-DRANENV_DIAG=13", "-I", os.path.join(REPO, "include"), "-x", "hip", "-fsyntax-only",
           os.path.join(CSRC, source)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_the_rebuilt_library_keeps_the_resource_limits():
    from intent_radio_sched_multi_slice_amd.csrc import build as hip_build
    import kernel_resources
    hip_build.build()
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", os.path.join(REPO, "tests", "test_kernel_resources.py")],
                       cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    kernels = {k["name"]: k for k in kernel_resources.kernel_resources()}
    for name in ("ranenv_core_kernel_members<8>", "ranenv_core_kernel_members<10>", "ranenv_persist_kernel_members<8>", "ranenv_persist_kernel_members<10>"):
        k = kernels[name]
        assert k["vgpr_count"] <= 96 and k.get("vgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, (name, k)
    for name in ("ranenv_core_kernel_members<16>", "ranenv_persist_kernel_members<16>"):
        k = kernels[name]
        assert k["vgpr_count"] <= 128 and k.get("vgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, (name, k)
