#!/usr/bin/env python3
"""Golden fixture of the scenario load figures, produced by RUNNING the reference's own functions (build container only; the
reference never travels):

    python tests/golden/gen_golden_rbs_needed.py

rbs_needed.npz      results/gen_results.py plot_rbs_needed_network_scenarios (:1251-1451) for scenario numbers 0..2 and
                    slices 0..4, and plot_graph (:78-) for "rbs_needed_slice" and "throughput_per_rb" on each of the three, run on
                    history files written by this build's history.py into a temporary hist/{scenario}/{agent}_{n}/ep_{100 n}.npz.
                    The inputs are tests/se_stats_ref.py's golden_case(): S 5 / U 25 / R 135, directed scenario rows 0..2,
                    24 steps, traces of 24 / 7 / 24 tiles entered at 0 / 3 / 5; only the seeds and sizes are stored.
                      network_{avg,min,max}_needed_rbs [3, T]   global_dict of every scenario number (scenario_results)
                      total_avg_needed_rbs [3]                  np.mean of the avg row: what the scenarios are ranked by
                      chosen [3]                                max / median / min scenario_number of the summary
                      slice_avg_needed_rbs [3, S, T]            the lines of rbs_needed_slice
                      slice_{min,max}_needed_rbs [3, S, T]      its fill bounds
                      throughput_per_rb{,_min,_max} [3, S, T]   the lines and fill bounds of throughput_per_rb
                    All exact doubles, from the figures' artists and global_dict; at generation time the CSV the function writes
                    is compared with them (np.allclose: pandas prints 17 digits or fewer), and the slice columns, added over the
                    slices one after the other, are asserted to be global_dict's rows.
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg          # noqa: E402,F401  installs the stand-ins, imports the reference
from gen_golden import REPO, META   # noqa: E402
from gen_golden_r3 import load_gen_results      # noqa: E402

sys.path.insert(0, REPO)
from intent_radio_sched_multi_slice_amd import history          # noqa: E402
from tests import se_stats_ref as ssr                           # noqa: E402


def fill_bounds(poly, T):
    """(lower, upper) of a fill_between artist over x = 0..T-1: its path runs (x0, y2_0), (x, y1)..., (x_last, y2_last),
    (x, y2) backwards, and closes."""
    v = poly.get_paths()[0].vertices
    assert v.shape[0] >= 2 * T + 2, v.shape
    y1 = v[1:T + 1]
    y2 = v[T + 2:2 * T + 2][::-1]
    assert np.array_equal(y1[:, 0], np.arange(T)) and np.array_equal(y2[:, 0], np.arange(T)), "unexpected fill_between path"
    return y1[:, 1].copy(), y2[:, 1].copy()


def main():
    import matplotlib.pyplot as plt
    import pandas as pd
    grs = load_gen_results()
    g = ssr.GOLDEN
    S, U, R, T = g["S"], g["U"], g["R"], g["T"]
    case = ssr.golden_case()
    tabs = case["tabs"]
    scenario, agent = "mult_slice", "any"
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "results", scenario))
    for n, ep in enumerate(case["eps"]):
        assert int(ep["scenario"]) == n
        bua, bsa, sua, req = tabs.to_reference(n)
        rows = {k: [] for k in history.HIST_KEYS}
        for t, tile in enumerate(ssr.trace_tiles(ep, T)):
            for k in ("pkt_incoming", "pkt_throughputs", "pkt_effective_thr", "dropped_pkts", "buffer_occupancies", "buffer_latencies"):
                rows[k].append(np.zeros(U))
            rows["mobility"].append(np.ones((U, 2)))
            rows["spectral_efficiencies"].append(case["pool"][tile].astype(np.float64)[None])
            rows["basestation_ue_assoc"].append(bua); rows["basestation_slice_assoc"].append(bsa); rows["slice_ue_assoc"].append(sua)
            rows["sched_decision"].append(np.zeros((1, U, R))); rows["reward"].append({"player_0": 0.0}); rows["slice_req"].append(req)
            rows["obs"].append({"player_0": np.zeros(S * 10)}); rows["agent_action"].append({"player_0": np.zeros(S)})
        history.write_episode_npz(os.path.join(tmp, "hist", scenario, f"{agent}_{n}", f"ep_{100 * n}.npz"), rows)
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        # ---- plot_rbs_needed_network_scenarios: three lines per chosen scenario, labelled with its number -----------------------------
        plt.figure()
        grs.plot_rbs_needed_network_scenarios(scenario, agent, np.arange(S), np.arange(3))
        lines = plt.gca().lines
        assert len(lines) == 9
        chosen, net = [], {}
        for i in range(3):
            grp = lines[3 * i:3 * i + 3]
            num = int(grp[0].get_label().split()[1].rstrip(","))
            assert [ln.get_label() for ln in grp] == [f"Scenario {num}, {w}" for w in ("max", "avg", "min")]
            chosen.append(num)
            net[num] = {w: np.asarray(ln.get_ydata(), dtype=np.float64).copy() for w, ln in zip(("max", "avg", "min"), grp)}
        plt.close()
        assert sorted(chosen) == [0, 1, 2], chosen                 # three distinct loads: every scenario number is one of the three
        csv = pd.read_csv(os.path.join("results", scenario, "rbs_needed_network_scenarios.csv"))
        for key, num in zip(("max_scenario", "median_scenario", "min_scenario"), chosen):
            for w in ("max", "avg", "min"):
                assert np.allclose(csv[f"{key}_{w}"].to_numpy(), net[num][w], rtol=1e-12, atol=0), (key, w)
        # ---- plot_graph, per scenario number --------------------------------------------------------------------------------------
        sl = {k: np.zeros((3, S, T)) for k in ("slice_avg_needed_rbs", "slice_min_needed_rbs", "slice_max_needed_rbs", "throughput_per_rb",
                                               "throughput_per_rb_min", "throughput_per_rb_max")}
        for n in range(3):
            gd = {}
            plt.figure()
            grs.plot_graph("rbs_needed_slice", np.arange(S), f"{agent}_{n}", scenario, 100 * n, [f"{agent}_{n}"], gd)
            ax = plt.gca()
            assert len(ax.lines) == S and len(ax.collections) == S
            for s in range(S):
                sl["slice_avg_needed_rbs"][n, s] = ax.lines[s].get_ydata()
                sl["slice_min_needed_rbs"][n, s], sl["slice_max_needed_rbs"][n, s] = fill_bounds(ax.collections[s], T)
            plt.close()
            for w, key in (("avg", "slice_avg_needed_rbs"), ("min", "slice_min_needed_rbs"), ("max", "slice_max_needed_rbs")):
                acc = sl[key][n, 0]
                for s in range(1, S):
                    acc = acc + sl[key][n, s]
                assert np.array_equal(acc, gd[f"{w}_needed_rbs"]) and np.array_equal(acc, net[n][w]), (n, w)
            plt.figure()
            grs.plot_graph("throughput_per_rb", np.arange(S), f"{agent}_{n}", scenario, 100 * n, [f"{agent}_{n}"], {})
            ax = plt.gca()
            assert len(ax.lines) == S and len(ax.collections) == S
            for s in range(S):
                sl["throughput_per_rb"][n, s] = ax.lines[s].get_ydata()
                sl["throughput_per_rb_min"][n, s], sl["throughput_per_rb_max"][n, s] = fill_bounds(ax.collections[s], T)
            plt.close()
    finally:
        os.chdir(cwd)
    out = {"cfg": np.array([S, U, R, g["Us"], g["seed"], T]), "scenario": np.array(g["scenario"]), "se_len": np.array(g["se_len"]),
           "se_offset": np.array(g["se_offset"]), "chosen": np.array(chosen), "meta": np.array(json.dumps(META))}
    for w in ("avg", "min", "max"):
        out[f"network_{w}_needed_rbs"] = np.stack([net[n][w] for n in range(3)])
    out["total_avg_needed_rbs"] = np.array([np.mean(net[n]["avg"]) for n in range(3)])
    assert [int(np.argmax(out["total_avg_needed_rbs"])), int(np.argsort(out["total_avg_needed_rbs"])[3 // 2]),
            int(np.argmin(out["total_avg_needed_rbs"]))] == chosen
    out.update(sl)
    path = os.path.join(HERE, "rbs_needed.npz")
    np.savez_compressed(path, **out)
    print("rbs_needed.npz", os.path.getsize(path), "bytes; chosen (max, median, min)", chosen, "total_avg", out["total_avg_needed_rbs"].tolist())


if __name__ == "__main__":
    main()
