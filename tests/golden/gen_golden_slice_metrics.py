#!/usr/bin/env python3
"""Golden fixture of the per-slice evaluation metrics, produced by RUNNING the reference's own functions (build container
only; the reference never travels):

    python tests/golden/gen_golden_slice_metrics.py

slice_metrics.npz      results/gen_results.py calc_slice_violations(data, slice_per_metric=True) (:874-970) and
                       calc_total_throughput (:791-809) for pkt_throughputs / pkt_effective_thr / pkt_incoming, run on history
                       files of the closed loop of eval_metrics.npz (gen_golden_r3.gen_eval_metrics: the same tables, scenarios
                       [1, 4, 2], seed 401, 60 TTIs x 3 episodes of one env, MAPF + PF on the CPU oracle, written by this build's
                       history.py), for both window conventions: "live" (the 10-TTI window never cleared; the whole run with its
                       reset observations as ONE file) and "restarted" (cleared at every reset; one file per episode with its
                       reset observation in front).  Per-TTI rows only are stored:
                         {live_deque, restarted_with_reset}_intent_slice_metric   [ep, t, S, 3]  (-2: slice skipped / metric undeclared)
                         {live_deque, restarted_with_reset}_{total_network_throughput, total_network_eff_throughput,
                                                             total_network_requested_throughput}   [ep, t]  Mbit
                       At generation time the rows of every file, aggregated the way :925-964 aggregates them, are asserted to
                       reproduce the two dicts the reference returned for that file, and the traffic is asserted to be
                       eval_metrics.npz's.
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg          # noqa: E402  installs the stand-ins, imports the reference
from gen_golden import REPO, META, set_stable   # noqa: E402
from gen_golden_r3 import load_gen_results      # noqa: E402

sys.path.insert(0, REPO)
from intent_radio_sched_multi_slice_amd import history          # noqa: E402
from oracle import pyoracle                                     # noqa: E402
from tests.synth import se_tile                                 # noqa: E402

METRIC_NAMES = ("throughput", "reliability", "latency")          # gen_results.py:881-885
THROUGHPUT_KEYS = (("total_network_throughput", "pkt_throughputs"), ("total_network_eff_throughput", "pkt_effective_thr"),
                   ("total_network_requested_throughput", "pkt_incoming"))      # gen_results.py:236-259


def aggregate_rows(intent_slice_metric, names):
    """Rows [n, S, 3] of one file + the slice names per row -> the two dicts, the way gen_results.py:925-964 builds them."""
    per_type, per_metric = {}, {}
    for row, nm in zip(intent_slice_metric, names):
        for s in range(row.shape[0]):
            d = row[s].copy()
            d[d == -2] = 1
            if np.sum(d < 0):
                for k, mn in enumerate(METRIC_NAMES):
                    if d[k] < 0:
                        per_metric.setdefault(nm[s], {})
                        per_metric[nm[s]][mn] = per_metric[nm[s]].get(mn, 0) + 1
            if np.min(d) < 0:
                per_type[nm[s]] = per_type.get(nm[s], 0) + 1
    return per_type, per_metric


def main():
    grs = load_gen_results()
    S, U, R, G, Us, steps, n_ep = 5, 25, 135, 5, 5, 60, 3
    assert grs.max_number_ues_slice == Us and int(U / S) == Us
    tabs = gg.ref_tables(6, seed=10, sort=True)
    scen_ids = [1, 4, 2]
    seed = 401
    cfg = pyoracle.make_cfg(S, U, R, G, Us, max_steps=steps)
    intra = np.ones(S, dtype=np.int32)
    from traffics.mult_slice import MultSliceTraffic
    tmp = tempfile.mkdtemp()
    raw_keys = ("pkt_incoming", "pkt_throughputs", "pkt_effective_thr", "dropped_pkts", "buffer_occupancies", "buffer_latencies")

    def push(dst, raw, sched, se32, req, bua, bsa, sua, obs, rew, act):
        for k in raw_keys:
            dst[k].append(raw[k].copy())
        dst["mobility"].append(np.ones((U, 2))); dst["spectral_efficiencies"].append(se32.astype(np.float64)[None])
        dst["basestation_ue_assoc"].append(bua); dst["basestation_slice_assoc"].append(bsa); dst["slice_ue_assoc"].append(sua)
        dst["sched_decision"].append(sched); dst["reward"].append(rew); dst["slice_req"].append(req)
        dst["obs"].append(obs); dst["agent_action"].append(act)

    def per_slice(path):
        """The reference's functions on one file -> rows [n, S, 3], throughputs [n, 3]; the dicts are checked against the rows."""
        data = np.load(path, allow_pickle=True)
        _, per_type, rows, per_metric = grs.calc_slice_violations(data, slice_per_metric=True)
        names = [[(r[f"slice_{s}"] or {}).get("name") for s in range(S)] for r in data["slice_req"]]
        got_type, got_metric = aggregate_rows(rows, names)
        assert got_type == per_type and got_metric == per_metric, (path, got_type, per_type, got_metric, per_metric)
        thr = np.stack([grs.calc_total_throughput(data, key, np.arange(S)) for _, key in THROUGHPUT_KEYS], axis=1)
        return rows, thr

    def run(tag, clear_at_reset):
        core = pyoracle.OracleEnv(cfg)
        rows = {k: [] for k in history.HIST_KEYS}
        is_tti, files_with_reset, traffic_all = [], [], []
        for ep, idx in enumerate(scen_ids):
            bua, bsa, sua, req = tabs.to_reference(idx)
            if clear_at_reset:
                core.clear()
            core.set_scenario(tabs, idx)
            tgen = MultSliceTraffic(U, np.random.default_rng(seed * 100 + ep))
            core.reset(se_tile(seed + ep, 0, U, R))
            with_reset = {k: [] for k in history.HIST_KEYS}
            zero = {k: np.zeros(U) for k in raw_keys}
            o0 = core.obs()
            for dst in (rows, with_reset):
                push(dst, zero, np.zeros((1, U, R)), se_tile(seed + ep, 0, U, R), req, bua, bsa, sua,
                     {"player_0": o0["obs_inter"]}, {"player_0": float(o0["reward"][0])}, {"player_0": np.zeros(S)})
            is_tti.append(False)
            for t in range(steps):
                sc = core.policy_mapf()
                start, count, dense = core.action_format(sc, intra)
                se32 = se_tile(seed + ep, t, U, R)
                traffic = tgen.step(sua, req, t, ep)
                if t % 13 == 6:
                    traffic = traffic * 5.0
                core.step(sc, intra, se32, traffic)
                raw, oo = core.raw(), core.obs()
                for dst in (rows, with_reset):
                    push(dst, raw, dense.astype(np.float64)[None], se32, req, bua, bsa, sua, {"player_0": oo["obs_inter"]},
                         {"player_0": float(oo["reward"][0])}, {"player_0": sc})
                is_tti.append(True)
                traffic_all.append(traffic)
            files_with_reset.append(history.write_episode_npz(os.path.join(tmp, f"{tag}_ep_{ep}_with_reset.npz"), with_reset))
        whole = history.write_episode_npz(os.path.join(tmp, f"{tag}_whole_run.npz"), rows)
        set_stable(True)
        w_rows, w_thr = per_slice(whole)
        sel = np.array(is_tti)
        out = {"whole_run": (w_rows[sel].reshape(n_ep, steps, S, 3), w_thr[sel].reshape(n_ep, steps, 3))}
        per = [per_slice(f) for f in files_with_reset]
        out["with_reset"] = (np.stack([r[1:] for r, _ in per]), np.stack([t[1:] for _, t in per]))
        set_stable(False)
        return out, np.array(traffic_all).reshape(n_ep, steps, U)

    live, trf_live = run("live", False)
    rest, trf_rest = run("restarted", True)
    ev = np.load(os.path.join(HERE, "eval_metrics.npz"), allow_pickle=True)
    assert np.array_equal(trf_live, ev["traffic"]) and np.array_equal(trf_rest, ev["traffic"])      # the same closed loop
    assert [int(x) for x in ev["cfg"]] == [S, U, R, G, Us, seed, steps, n_ep] and ev["scen_ids"].tolist() == scen_ids
    out = {"cfg": np.array([S, U, R, G, Us, seed, steps, n_ep]), "scen_ids": np.array(scen_ids),
           "metric_names": np.array(json.dumps(list(METRIC_NAMES))), "meta": np.array(json.dumps(META))}
    for tag, (rows, thr) in (("live_deque", live["whole_run"]), ("restarted_with_reset", rest["with_reset"])):
        out[f"{tag}_intent_slice_metric"] = rows
        for k, (name, _) in enumerate(THROUGHPUT_KEYS):
            out[f"{tag}_{name}"] = thr[:, :, k]
    np.savez_compressed(os.path.join(HERE, "slice_metrics.npz"), **out)
    for tag in ("live_deque", "restarted_with_reset"):
        m = out[f"{tag}_intent_slice_metric"]
        d = np.where(m == -2, 1.0, m)
        print(tag, "slice-TTIs in violation", int((d.min(axis=3) < 0).sum()), "per metric", (d < 0).sum(axis=(0, 1, 2)).tolist(),
              "Mbit", [round(float(out[f"{tag}_{n}"].sum()), 3) for n, _ in THROUGHPUT_KEYS])


if __name__ == "__main__":
    main()
