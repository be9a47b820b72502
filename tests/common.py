"""Numpy-only helpers shared by the CPU and GPU test modules and by tools/oracle_coverage.py; what needs torch or a device is
in tests/gpu_common.py."""
from __future__ import annotations

import os

import numpy as np

from intent_radio_sched_multi_slice_amd.scenario import ScenarioTables

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name: str):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def tables_from(fx, prefix: str = "tab_") -> ScenarioTables:
    return ScenarioTables.from_arrays({k[len(prefix):]: fx[k] for k in fx.files if k.startswith(prefix)})


AGENT_CASES = ["agent_ref_mixed", "agent_ref_rr", "agent_ref_pf_nosort", "agent_ref_mt",
               "agent_scaled_mixed", "agent_scaled_pf_nosort"]
HEAD_CASES = ["heads_ref", "heads_scaled"]
TRACE_CASES = ["trace_ref_random", "trace_ref_marr", "trace_ref_mapf", "trace_scaled_mapf",
               "trace_scaled_random", "trace_plumbing"]

# float tolerance between the oracle and the reference's own outputs: both are IEEE double in
# numpy's operation order, so they agree to rounding of a handful of operations.
RTOL, ATOL = 1e-12, 1e-12
# the device against the oracle, per TTI; integers are always compared exactly
OBS_TOL = 1e-5      # observations are float32 on the device (BASELINE.json's north_star states the bar)
REW_TOL = 1e-9      # rewards are float64 on both sides
PKT_COUNTS = ("pkt_incoming", "pkt_throughputs", "pkt_effective_thr", "dropped_pkts")


# ----------------------------------------------------------------------------------------------
# synthetic batches and oracle mirrors shared by the tests
# ----------------------------------------------------------------------------------------------
def poisson_traffic_rows(tables: ScenarioTables, scen: int, rng: np.random.Generator, steps: int) -> np.ndarray:
    """[steps, U] offered bits in MultSliceTraffic.step's draw order
    (traffics/mult_slice.py:24-32: slices in index order, UEs ascending, Poisson(Mbps)*1e6)."""
    U, S = tables.n_ues, tables.n_slices
    out = np.zeros((steps, U))
    for t in range(steps):
        for s in range(S):
            if not tables.slice_has_req[scen, s]:
                continue
            n = int(tables.slice_nues[scen, s])
            ues = tables.slice_ues[scen, s, :n]
            out[t, ues] = rng.poisson(tables.slice_traffic[scen, s], n) * 1e6
    return out


def rb_major(se_ue_major):
    """[..., U, R] tiles as the device reads them: [..., R, U], contiguous."""
    return np.ascontiguousarray(np.swapaxes(se_ue_major, -1, -2))


def oracle_envs(tables, scen, dims, steps, hist_depth=10, per_element=False):
    """One pyoracle.OracleEnv per entry of ``scen``, on that scenario, not yet reset; ``dims`` = (S, U, R, G, Us)."""
    from oracle import pyoracle
    cfg = pyoracle.make_cfg(*dims, max_steps=steps, hist_depth=hist_depth)
    out = []
    for sc in scen:
        o = pyoracle.OracleEnv(cfg)
        o.set_scale_per_element(per_element)
        o.set_scenario(tables, int(sc))
        out.append(o)
    return out


def tti_metrics(oo, raw, active=None):
    """What one TTI adds to the eight running sums (include/ranenv.h), from the oracle's obs() and raw(): slices in violation =
    minimum intent drift < 0, undeclared metrics as 0 (agents/common.py:389-427: active_observations); the same for priority
    slices; the distances are the sums of those negative minima.  ``active``: slice_active in the rows' sorted order -- an
    inactive slice with UEs has a drift row, and no part in the reward; None where no such slice exists."""
    rows = oo["obs_inter"].reshape(-1, 10)
    ao, prio = rows[:, 0:3].min(axis=1), rows[:, 6]
    if active is not None:
        ao = np.where(active, ao, 0.0)
    neg, pneg = ao < 0.0, prio * ao < 0.0
    return np.array([1.0, oo["reward"][0], neg.sum(), pneg.sum(), ao[neg].sum(), ao[pneg].sum(),
                     raw["pkt_effective_thr"].sum(), raw["dropped_pkts"].sum()])
