"""What the scenario load costs on the device, on the bench's configs[2] workload (B 4096, S 10 / U 100 / R 135, an HBM pool of
--traces x --trace-len tiles bound RB-quad-major; workloads.make_bench_workload).

Writes one JSON record to profiles/se_stats_probe.json (and prints it).  One job; inside a child process the blocks are
ALTERNATED (--alternations rounds), medians over all samples of a block:
  build_se_stats_ms         ranenv_build_se_stats on the whole pool (the call returns when the statistics are complete)
  sidecar_build_ms          the closest existing pass: ranenv_set_se_mode(GATHER) on the same pool (reads the pool once, writes the
                            per-tile means and a UE-major copy of the pool)
  eager_torch_ms            what a user can do today: the same four statistics in eager torch on the device, float64, in chunks of
                            --torch-chunk tiles (the RB-quad-major pool re-ordered to [tiles, U, R] first)
  rbs_needed_envs_ms        ranenv_rbs_needed for the B episode descriptors of the workload at T = --load-steps, episode means only
  rbs_needed_traces_ms      the same for one episode per trace of the pool, with the per-step rows
and, from them, pool bytes / time as a fraction of --peak-tbs (8 TB/s) for the two builds, next to tools/tile_probe.hip's 6.6 TB/s for
this access pattern.  A build rate clearly below the sidecar build's means the second walk of a tile does not come from L2.

Then the headline, each sample in a child process of its own: rollout(--steps) on this build and on the parent commit's library
(--baseline-lib, loaded through RANENV_LIB), the parent measured twice per round: `parent_vs_parent` is the spread of the two parent
series' medians, `parent_range_ms` the range of all parent samples, and `this_over_parent` beyond them would be a finding (nothing a rollout enqueues changes; the step code objects are the
parent's byte for byte).

    python tools/se_stats_probe.py [--traces 200] [--trace-len 1000] [--alternations 3] [--baseline-lib parent.so]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "se_stats_probe.json")
TILE_PROBE_TBS = 6.6          # tools/tile_probe.hip, RB-quad-major, the headline's occupancy (profiles/r05_ab_log.txt)


def _workload(args):
    import ctypes
    import torch
    from intent_radio_sched_multi_slice_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.FUNCTIONS if not hasattr(raw, n)]:      # (the parent commit's library lacks the three new functions)
        _lib.FUNCTIONS.pop(name)
    from intent_radio_sched_multi_slice_amd.workloads import make_bench_workload
    wl, _ = make_bench_workload(2, torch.device("cuda", 0), n_traces=args.traces, trace_len=args.trace_len, keep_rb_major=False)
    return torch, wl


def _wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure_load(args):
    torch, wl = _workload(args)
    env = wl.env
    assert env.se_layout == "quad"
    pool = env.bound_se_pool                                   # [tiles, ceil(R/4), U, 4]
    n, U, R = int(pool.shape[0]), env.U, env.R

    def eager():
        out = torch.empty((n, 4, U), dtype=torch.float64, device=env.device)
        for t0 in range(0, n, args.torch_chunk):
            x = pool[t0:t0 + args.torch_chunk].permute(0, 2, 1, 3).reshape(-1, U, pool.shape[1] * 4)[:, :, :R].double()
            out[t0:t0 + x.shape[0], 0] = x.mean(dim=2)
            out[t0:t0 + x.shape[0], 1] = x.std(dim=2, unbiased=False)
            out[t0:t0 + x.shape[0], 2] = x.amin(dim=2)
            out[t0:t0 + x.shape[0], 3] = x.amax(dim=2)
        return out

    def sidecars():
        env.set_se_mode("gather")
        env.set_se_mode("stream")

    import numpy as np
    traces = env._episode_array(args.traces, np.arange(args.traces) % env.n_scenarios, np.arange(args.traces) * args.trace_len,
                                args.trace_len, 0, 0, 1, 0)
    blocks = {"build_se_stats": lambda: env.se_tile_stats(rebuild=True), "sidecar_build": sidecars, "eager_torch": eager,
              "rbs_needed_envs": lambda: env.scenario_load(env.episodes, args.load_steps),
              "rbs_needed_traces": lambda: env.scenario_load(traces, args.load_steps, per_step=True)}
    for fn in blocks.values():                                 # warm-up: first launches, the allocations
        fn()
    same = bool(torch.allclose(env.se_tile_stats(), eager(), rtol=1e-12, atol=0))      # (torch's summation order is its own)
    series = {k: [] for k in blocks}
    for _ in range(args.alternations):
        for k, fn in blocks.items():
            series[k].append(_wall(torch, fn))
    load = env.scenario_load(traces, args.load_steps)["episode_mean"][:, 0].cpu().numpy()
    info = {"ms": series, "device": torch.cuda.get_device_name(0), "tiles": n, "pool_bytes": int(pool.numel()) * 4,
            "stats_bytes": n * 4 * U * 8, "eager_allclose_1e-12": same, "episodes_envs": int(env.B), "episodes_traces": args.traces,
            "traces_needing_more_than_R": int((load > R).sum())}
    env.close()
    return info


def measure_rollout(args):
    torch, wl = _workload(args)
    env = wl.env
    env.reset()
    env.rollout(8)
    out = [_wall(torch, lambda: env.rollout(args.steps)) for _ in range(args.reps)]
    info = {"ms": out, "persistent": env.get_option("last_rollout_persistent"), "launches": env.get_option("last_rollout_launches")}
    env.close()
    return info


def _child(block, args, lib):
    env = dict(os.environ)
    if lib:
        env["RANENV_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", block]
    for k in ("traces", "trace_len", "alternations", "steps", "reps", "load_steps", "torch_chunk"):
        cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
    res = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=900)
    print(f"[se_stats_probe] {block} ({'parent' if lib else 'this build'}) done", file=sys.stderr, flush=True)
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traces", type=int, default=200)
    ap.add_argument("--trace-len", type=int, default=1000)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--load-steps", type=int, default=1000)
    ap.add_argument("--torch-chunk", type=int, default=10000)
    ap.add_argument("--peak-tbs", type=float, default=8.0)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--child", default=None, choices=("load", "rollout"))
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure_load(args) if args.child == "load" else measure_rollout(args)))
        return
    # every measurement in a child: the parent of them all never opens the GPU
    load = _child("load", args, None)
    med = {k: statistics.median(v) for k, v in load["ms"].items()}
    tbs = {k: load["pool_bytes"] / (med[k] * 1e-3) / 1e12 for k in ("build_se_stats", "sidecar_build", "eager_torch")}
    record = {"probe": "se_stats", "config": "configs[2]: B 4096, S 10 / U 100 / R 135, quad layout", "traces": args.traces,
              "trace_len": args.trace_len, "alternations": args.alternations, "device": load["device"], "tiles": load["tiles"],
              "pool_bytes": load["pool_bytes"], "stats_bytes": load["stats_bytes"], "samples_ms": load["ms"],
              **{k + "_ms": v for k, v in med.items()},
              "pool_tb_per_s": tbs, "fraction_of_peak": {k: v / args.peak_tbs for k, v in tbs.items()}, "peak_tb_per_s": args.peak_tbs,
              "tile_probe_tb_per_s": TILE_PROBE_TBS, "build_over_sidecar_build": med["build_se_stats"] / med["sidecar_build"],
              "build_over_eager_torch": med["build_se_stats"] / med["eager_torch"], "eager_allclose_1e-12": load["eager_allclose_1e-12"],
              "load_steps": args.load_steps, "episodes_envs": load["episodes_envs"], "episodes_traces": load["episodes_traces"],
              "traces_needing_more_than_R": load["traces_needing_more_than_R"]}
    series = {"this": [], "parent_a": [], "parent_b": []}
    for _ in range(args.alternations):
        if args.baseline_lib:
            series["parent_a"] += _child("rollout", args, args.baseline_lib)["ms"]
        r = _child("rollout", args, None)
        series["this"] += r["ms"]
        record["rollout_schedule"] = {"persistent": r["persistent"], "launches": r["launches"]}
        if args.baseline_lib:
            series["parent_b"] += _child("rollout", args, args.baseline_lib)["ms"]
    roll = {"steps": args.steps, "samples_ms": series, "this_ms": statistics.median(series["this"])}
    if args.baseline_lib:
        pa, pb = statistics.median(series["parent_a"]), statistics.median(series["parent_b"])
        parent = statistics.median(series["parent_a"] + series["parent_b"])
        spread = abs(pa / pb - 1.0)
        both = series["parent_a"] + series["parent_b"]
        roll.update({"parent_ms": parent, "parent_vs_parent": spread, "this_over_parent": roll["this_ms"] / parent,
                     "within_parent_spread": abs(roll["this_ms"] / parent - 1.0) <= spread,
                     # ... and against the parent's run-to-run range: where this build's median and samples lie among the parent's samples
                     "parent_range_ms": [min(both), max(both)], "this_range_ms": [min(series["this"]), max(series["this"])],
                     "this_median_within_parent_range": min(both) <= roll["this_ms"] <= max(both)})
    record["rollout"] = roll
    line = json.dumps(record)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
