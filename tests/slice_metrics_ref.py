"""Expected per-slice episode sums (include/ranenv.h "Per-slice episode metrics") from the CPU oracle's per-TTI outputs and the
scenario tables, and the cases tests/test_gpu_slice_metrics.py runs them on.  Shared by that file and by
tests/test_slice_metrics_cpu.py, which checks on exactly these inputs that a green device run means something.

``tti_share`` restates the ten columns in numpy from what the issue names as their sources: ``obs()["obs_intra"][:, 0:6]`` (the
three per-metric slice drifts and their declared flags, by slice index), ``obs()["reward"][1:]`` (the minimum declared drift),
``raw()`` (per-UE packet counts) and the tables (``slice_active``, ``slice_ues``).  ``slip`` plants one of four mistakes a kernel
could make; the CPU test asserts that each of them moves the expected sums by at least one count on the chosen cases.
"""
from __future__ import annotations

import numpy as np

from tests import directed_intents as di
from tests import intent_census as ic

K = 10
SLIPS = ("no_active_gate", "sorted_position", "undeclared_counted", "contiguous_ues")
PKT_KEYS = ("pkt_incoming", "pkt_throughputs", "pkt_effective_thr", "dropped_pkts")

# The directed cases of the device test (issue: the two S 5 / U 25 / Us 10 cases at B 7 and 26 TTIs, one case of two-wave envs at
# S 10 / U 100, one at the size limit S 16 / Us 16 / U 256 with its 256-thread block).  RANGE_INTENT_CASE is oracle-only: the C ABI
# refuses a table that declares a metric twice, so the device test can only hold the handle to that refusal.
CASES = {
    "ref-overfulfill-0.5": di.CASE_BY_NAME["ref-overfulfill-0.5"],
    "range-intent": di.RANGE_INTENT_CASE,
    "s10-u100": di._case("s10-u100", 10, 100, 120, 3, 10, B=5, steps=20, n_scen=5, first=17, load=1.3, policy=2, intra=1),
    "s16-u256": di._case("s16-u256", 16, 256, 96, 1, 16, B=3, steps=14, n_scen=3, first=5, load=2.0, se_scale=0.5, policy=1, intra=0,
                         **dict(di.ALL_SCALARS, overfulfill=0.1)),
}
DEVICE_CASES = ("ref-overfulfill-0.5", "s10-u100", "s16-u256")
_RUNS = {}


def run_of(name):
    """The oracle's replay of one case (tests/intent_census.replay), computed once per process."""
    if name not in _RUNS:
        _RUNS[name] = ic.replay(CASES[name])
    return _RUNS[name]


def tti_share(tabs, scen, obs, raw, slip=None):
    """[S, 10] float64: what one TTI adds for the env on scenario row ``scen``."""
    S = tabs.n_slices
    oa = np.asarray(obs["obs_intra"], dtype=np.float64).reshape(S, -1)
    dmin = np.asarray(obs["reward"], dtype=np.float64)[1:1 + S]
    out = np.zeros((S, K))
    for s in range(S):
        src = int(tabs.sorted_slices[scen, s]) if slip == "sorted_position" else s
        active = True if slip == "no_active_gate" else bool(tabs.slice_active[scen, src] != 0)
        drift, flag = oa[src, 0:3], oa[src, 3:6]
        if active:
            out[s, 0] = 1.0
            out[s, 1] = 1.0 if dmin[src] < 0 else 0.0
            for m in range(3):
                declared = True if slip == "undeclared_counted" else flag[m] > 0
                value = drift[m] if flag[m] > 0 else -2.0          # (the reference's sentinel of an undeclared metric, results/gen_results.py:886)
                out[s, 2 + m] = 1.0 if (declared and value < 0) else 0.0
            out[s, 5] = min(dmin[src], 0.0)
        if slip == "contiguous_ues":
            per = tabs.n_ues // S
            ues = np.arange(src * per, (src + 1) * per)
        else:
            ues = tabs.slice_ues[scen, src, :int(tabs.slice_nues[scen, src])]
        for k, key in enumerate(PKT_KEYS):
            out[s, 6 + k] = float(np.asarray(raw[key], dtype=np.float64)[ues].sum())
    return out


def expected_sums(run, slip=None):
    """[B, S, 10]: the sums over the run's TTIs, added in TTI order as the device adds them."""
    c, tabs = run["case"], run["tables"]
    out = np.zeros((c["B"], c["S"], K))
    for t in range(c["steps"]):
        for b, pe in enumerate(run["steps"][t][2]):
            out[b] += tti_share(tabs, int(run["scen"][b]), pe[2], pe[1], slip)
    return out
