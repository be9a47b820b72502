"""Scenario load (ranenv_build_se_stats / ranenv_rbs_needed): the inputs the CPU and the GPU tests and the fixture's generator
share, and the float64 numpy restatement of results/gen_results.py:277-497 / :1251-1451 the device is held against.

Inputs.  ``directed_tables`` builds scenario rows whose slices play fixed ROLES, rotated by one slice index per row so that a
slice index means another role in every row:

  empty       no members, a request                                   -> every figure 0 (den == 0)
  no_request  members, NO request, yet a traffic figure in the table  -> thr = 0: needs nothing
  spiky       members whose SE rows are zeros with one large value    -> std > mean: sum(mean - std) <= 0, max_needed = 0 (not R)
  starved     members at 2 % of the SE, heavy traffic                 -> avg_needed > R (stays unclipped), max_needed > R (clipped)
  loaded      members at full SE, moderate traffic
  plain       every further slice

UE ids are scattered over the slices by a hashed permutation (members on both sides of numpy's pairwise split of a 256-UE row).
``directed_tile`` is ``tests.synth.se_tile`` with the rows of the spiky and the starved UEs rewritten; a trace therefore belongs to
the scenario row whose roles shaped it (``make_case`` lays one trace per episode into the pool).

Nothing here is stored in the fixture but seeds, sizes and table indices.
"""
from __future__ import annotations

import numpy as np

from intent_radio_sched_multi_slice_amd.scenario import ScenarioTables, stable_sort_slices
from tests.synth import hash_u01, se_tile

ROLES = ("empty", "no_request", "spiky", "starved", "loaded", "plain")
EMPTY, NO_REQUEST, SPIKY, STARVED, LOADED, PLAIN = range(6)
SLIPS = ("ddof1", "clip_all", "R_where_not_positive", "ignore_has_req", "sorted_position", "divide_by_U")
BANDWIDTH_HZ = 100e6


def slice_roles(n_rows: int, S: int) -> np.ndarray:
    """[row, slice] -> role: the five directed roles first, rotated by the row number, plain behind them."""
    r = (np.arange(S)[None, :] + np.arange(n_rows)[:, None]) % S
    return np.minimum(r, PLAIN)


def directed_tables(n_rows: int, S: int, U: int, Us: int, seed: int = 0) -> ScenarioTables:
    assert S >= 5 and Us >= 3
    tabs = ScenarioTables.empty(n_rows, S, U, Us)
    roles = slice_roles(n_rows, S)
    for k in range(n_rows):
        perm = np.argsort(hash_u01(seed * 31 + k + 1, np.arange(U)), kind="stable")
        at = 0
        for s in range(S):
            role = int(roles[k, s])
            n = {EMPTY: 0, NO_REQUEST: 3, SPIKY: 2, STARVED: Us, LOADED: Us}.get(role, max(1, Us - (s % 3)))
            traffic = {EMPTY: 10.0, NO_REQUEST: 7.0, SPIKY: 5.0, STARVED: 60.0, LOADED: 20.0}.get(role, 2.0 + s)
            ues = np.sort(perm[at:at + n])
            at += n
            assert at <= U
            tabs.slice_active[k, s] = 1
            tabs.slice_has_req[k, s] = 0 if role == NO_REQUEST else 1
            tabs.slice_traffic[k, s] = traffic * (1 + k)             # (the rows differ in load: three distinct ranks)
            tabs.slice_priority[k, s] = float(s % 2)
            tabs.slice_nues[k, s] = n
            tabs.slice_ues[k, s, :n] = ues
            tabs.ue_slice[k, ues] = s
            tabs.ue_pos[k, ues] = np.arange(n)
            tabs.slice_buffer_size[k, s], tabs.slice_buffer_latency[k, s], tabs.slice_message_size[k, s] = 100, 100, 1024
            tabs.ue_pkt_size[k, ues], tabs.ue_max_pkts[k, ues], tabs.ue_max_age[k, ues] = 1024, 100, 100
        tabs.sorted_slices[k] = stable_sort_slices(tabs.slice_nues[k], tabs.slice_traffic[k], tabs.slice_has_req[k])
    return tabs


def ue_roles(tabs: ScenarioTables, row: int) -> np.ndarray:
    """[U] role of every UE of a scenario row (-1: in no slice)."""
    roles = slice_roles(tabs.n_scenarios, tabs.n_slices)[row]
    us = tabs.ue_slice[row]
    return np.where(us >= 0, roles[np.maximum(us, 0)], -1)


def directed_tile(role_of_ue: np.ndarray, seed: int, t: int, U: int, R: int) -> np.ndarray:
    """(U, R) float32: synth.se_tile with the spiky UEs' rows zero but for one RB, and the starved UEs' at 2 %."""
    se = se_tile(seed, t, U, R).copy()
    for u in np.nonzero(role_of_ue == SPIKY)[0]:
        se[u] = 0.0
        se[u, (7 * u + 3 * t) % R] = 30.0
    starved = role_of_ue == STARVED
    se[starved] = se[starved] * np.float32(0.02)
    return se


def episode_array(scenario, se_base, se_len, se_offset):
    from intent_radio_sched_multi_slice_amd import _lib
    import ctypes
    dt = [("scenario", "<i4"), ("se_len", "<i4"), ("se_base", "<i8"), ("se_offset", "<i4"), ("trf_len", "<i4"), ("trf_base", "<i8"),
          ("trf_offset", "<i4"), ("reserved", "<i4")]
    eps = np.zeros(len(scenario), dtype=dt)
    assert eps.dtype.itemsize == ctypes.sizeof(_lib.Episode)
    eps["scenario"], eps["se_base"], eps["se_len"], eps["se_offset"], eps["trf_len"] = scenario, se_base, se_len, se_offset, 1
    return eps


def make_case(S: int, U: int, Us: int, R: int, scenario, se_len, se_offset, seed: int, n_rows: int = 3):
    """Scenario rows + one trace per episode, laid end to end into a pool: -> dict(tabs, eps, pool (n_tiles, U, R) float32, sizes)."""
    tabs = directed_tables(n_rows, S, U, Us, seed=seed)
    tiles, base = [], []
    for i, (row, ln) in enumerate(zip(scenario, se_len)):
        base.append(len(tiles))
        role = ue_roles(tabs, int(row))
        tiles += [directed_tile(role, seed * 1000 + i, t, U, R) for t in range(int(ln))]
    return {"tabs": tabs, "eps": episode_array(np.asarray(scenario), np.asarray(base), np.asarray(se_len), np.asarray(se_offset)),
            "pool": np.stack(tiles), "S": S, "U": U, "Us": Us, "R": R}


# the fixture's case (tests/golden/gen_golden_rbs_needed.py): the reference's own size, scenario numbers 0..2 on rows 0..2; the second
# trace is shorter than the episode (the modulo wraps) and two start inside their trace
GOLDEN = dict(S=5, U=25, Us=5, R=135, scenario=[0, 1, 2], se_len=[24, 7, 24], se_offset=[0, 3, 5], seed=77, T=24)


def golden_case():
    g = GOLDEN
    return make_case(g["S"], g["U"], g["Us"], g["R"], g["scenario"], g["se_len"], g["se_offset"], g["seed"])


# the shapes of the device test's RBs-needed cases: (S, U, Us, R, scenario rows of the episodes, se_len, se_offset, seed, T)
DEVICE_CASES = {
    "S5_U25": (5, 25, 5, 135, [0, 1, 2, 1], [12, 5, 12, 12], [0, 3, 7, 11], 5, 12),
    "S10_U100": (10, 100, 10, 135, [2, 0, 1], [10, 4, 10], [0, 1, 6], 6, 10),
    "S16_U256": (16, 256, 16, 135, [1, 2, 0], [9, 9, 3], [4, 0, 2], 7, 9),
}


def device_case(name):
    S, U, Us, R, scen, ln, off, seed, T = DEVICE_CASES[name]
    return make_case(S, U, Us, R, scen, ln, off, seed), T


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def tile_stats(se32: np.ndarray) -> np.ndarray:
    """(..., U, R) float32 -> (..., 4, U) float64: np.mean, np.std, np.min, np.max over the RBs of the float64 values."""
    x = np.ascontiguousarray(se32, dtype=np.float32).astype(np.float64)
    return np.stack([np.mean(x, axis=-1), np.std(x, axis=-1), np.min(x, axis=-1), np.max(x, axis=-1)], axis=-2)


def trace_tiles(ep, T: int) -> np.ndarray:
    """Pool tile of every step of an episode: se_base + (se_offset + t) % se_len (include/ranenv.h)."""
    return int(ep["se_base"]) + (int(ep["se_offset"]) + np.arange(T)) % int(ep["se_len"])


def rbs_needed(tabs: ScenarioTables, row: int, se: np.ndarray, R: int, bandwidth_hz: float = BANDWIDTH_HZ, slip=None):
    """gen_results.py:361-457 (and :277-358) restated on ``se`` = np.squeeze(spectral_efficiencies): (T, U, R) float64, for scenario
    row ``row``.  -> per_step_slice (T, S, 6), per_step_network (T, 3), episode_mean (3,).  ``slip``: one of SLIPS, a planted mistake."""
    assert slip is None or slip in SLIPS
    T, U, S = se.shape[0], se.shape[1], tabs.n_slices
    mean = np.mean(se, axis=2)
    std = np.std(se, axis=2, ddof=1 if slip == "ddof1" else 0)
    lo, hi = np.min(se, axis=2), np.max(se, axis=2)
    mbps = bandwidth_hz / 1e6                       # the source's literal 100
    per_slice = np.zeros((T, S, 6))
    net = None
    for s in range(S):
        idx = int(tabs.sorted_slices[row, s]) if slip == "sorted_position" else s
        slice_ues = np.tile((tabs.ue_slice[row] == idx).astype(np.float64), (T, 1))
        den = np.sum(slice_ues, axis=1)
        div = np.full(T, float(U)) if slip == "divide_by_U" else den
        some = np.logical_not(np.isclose(den, np.zeros_like(den)))
        avg_se = np.divide(np.sum(mean * slice_ues, axis=1), div, where=some, out=np.zeros(T))
        min_se = np.divide(np.sum((mean - std) * slice_ues, axis=1), div, where=some, out=np.zeros(T))
        max_se = np.divide(np.sum((mean + std) * slice_ues, axis=1), div, where=some, out=np.zeros(T))
        has_req = bool(tabs.slice_has_req[row, idx]) or slip == "ignore_has_req"
        requested_thr = np.array([float(tabs.slice_traffic[row, idx]) if has_req else 0 for _ in range(T)])
        fill = float(R) if slip == "R_where_not_positive" else 0.0
        avg_needed = np.divide(requested_thr * den, (mbps / R) * avg_se, where=avg_se > 0, out=np.full(T, fill))
        min_needed = np.divide(requested_thr * den, (mbps / R) * max_se, where=max_se > 0, out=np.full(T, fill))
        max_needed = np.divide(requested_thr * den, (mbps / R) * min_se, where=min_se > 0, out=np.full(T, fill))
        max_needed[max_needed > R] = R
        if slip == "clip_all":
            avg_needed[avg_needed > R] = R
            min_needed[min_needed > R] = R
        per_slice[:, s, 0], per_slice[:, s, 1], per_slice[:, s, 2] = avg_needed, min_needed, max_needed
        den_rb = den * R
        for c, stat in ((3, mean), (4, lo), (5, hi)):                      # throughput_per_rb, :277-358
            per_slice[:, s, c] = np.divide(np.sum(stat * slice_ues, axis=1) * mbps, den_rb, where=some, out=np.zeros(T))
        cols = np.stack([avg_needed, min_needed, max_needed], axis=1)
        net = cols if s == 0 else net + cols                               # global_dict, :458-471
    episode_mean = np.array([np.mean(np.ascontiguousarray(net[:, c])) for c in range(3)])      # :1392-1396, per column
    return per_slice, net, episode_mean


def episode_load(case: dict, i: int, T: int, slip=None):
    """Episode i of a case, restated: the tiles of its steps, then rbs_needed on its scenario row."""
    ep = case["eps"][i]
    se = case["pool"][trace_tiles(ep, T)].astype(np.float64)
    return rbs_needed(case["tabs"], int(ep["scenario"]), se, case["R"], slip=slip)


def branch_census(case: dict, T: int) -> dict:
    """How often every branch of the rule is taken on a case's inputs, from the inputs and the statistics alone (the CPU test asserts
    every count positive: a green device run then covered them)."""
    tabs, R = case["tabs"], case["R"]
    out = {k: 0 for k in ("no_members", "members_no_request", "low_se_not_positive", "max_needed_clipped", "avg_needed_above_R",
                          "sorted_not_index")}
    for i, ep in enumerate(case["eps"]):
        row = int(ep["scenario"])
        st = tile_stats(case["pool"][trace_tiles(ep, T)])                  # (T, 4, U)
        out["sorted_not_index"] += int(np.any(tabs.sorted_slices[row] != np.arange(tabs.n_slices)))
        for s in range(tabs.n_slices):
            member = tabs.ue_slice[row] == s
            n = int(member.sum())
            if n == 0:
                out["no_members"] += T
                continue
            if not tabs.slice_has_req[row, s]:
                out["members_no_request"] += T * int(tabs.slice_traffic[row, s] > 0)
                continue
            want = float(tabs.slice_traffic[row, s]) * n
            low = (st[:, 0, member] - st[:, 1, member]).sum(axis=1) / n
            avg = st[:, 0, member].sum(axis=1) / n
            out["low_se_not_positive"] += int((low <= 0).sum())
            with np.errstate(divide="ignore", invalid="ignore"):
                out["max_needed_clipped"] += int(((low > 0) & (want / ((BANDWIDTH_HZ / 1e6 / R) * low) > R)).sum())
                out["avg_needed_above_R"] += int(((avg > 0) & (want / ((BANDWIDTH_HZ / 1e6 / R) * avg) > R)).sum())
    return out
