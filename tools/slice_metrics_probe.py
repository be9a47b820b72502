"""What the per-slice episode metrics cost on the device: rollout(K) under MAPF + PF at the two sizes of the DESIGN 4.p tables
(B 4096 S 10 / U 100 and B 16 384 S 5 / U 25, workloads.make_mult_slice_workload).

Writes one JSON record to profiles/slice_metrics_probe.json (and prints it).  Per size, every block in a child process of its own,
the blocks ALTERNATED inside one job (--alternations rounds), medians over all samples of a block:
  eight_sums_this_ms       (1) rollout(K) with the eight per-env sums only (ranenv_enable_metrics), this build
  eight_sums_parent_ms     (1) the same with the parent commit's library (--baseline-lib, loaded through RANENV_LIB), measured twice
                           per round: `parent_vs_parent` is the spread of the two parent series (ratio of their medians), and
                           `this_over_parent` beyond that spread is reported as a finding (`untaxed_within_spread`)
  slice_metrics_ms         (2) rollout(K) with slice metrics on: one TTI per launch + one small launch per TTI
  step_loop_readback_ms    (3) what it replaces: a step() loop that copies the four raw views, reward and obs_intra to the host
                           every TTI
and the ratios (2)/(1) and (2)/(3).  No threshold is attached to (2).

    python tools/slice_metrics_probe.py [--steps 200] [--reps 3] [--alternations 3] [--baseline-lib parent.so]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SIZES = {"B4096_S10_U100": dict(batch=4096, n_slices=10, n_ues=100, n_rbs=135, rbs_per_rbg=1, max_ues_slice=10),
         "B16384_S5_U25": dict(batch=16384, n_slices=5, n_ues=25, n_rbs=135, rbs_per_rbg=5, max_ues_slice=10)}
OUT = os.path.join(REPO, "profiles", "slice_metrics_probe.json")
RAW = ("pkt_incoming", "pkt_throughputs", "pkt_effective_thr", "dropped_pkts")


def measure(block, size, steps, reps):
    """One block at one size -> the list of its samples in ms."""
    import ctypes
    import torch
    from intent_radio_sched_multi_slice_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.FUNCTIONS if not hasattr(raw, n)]:      # (the parent commit's library lacks the two new functions)
        _lib.FUNCTIONS.pop(name)
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    wl = make_mult_slice_workload(device=torch.device("cuda", 0), policy=_lib.POLICY_MAPF, intra=_lib.INTRA_PF, n_scenarios=64, n_traces=64,
                                  trace_len=256, max_steps=100000, **SIZES[size])
    env = wl.env
    env.enable_metrics(0)
    if block == "slice":
        env.enable_slice_metrics()
    v = env.views()

    def step_loop(n=steps):
        for _ in range(n):
            env.step()
            for k in RAW:
                v[k].cpu()
            env.reward.cpu()
            env.obs_intra.cpu()

    fn = step_loop if block == "step_loop" else (lambda: env.rollout(steps))
    env.reset()
    step_loop(4) if block == "step_loop" else env.rollout(8)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1))
    info = {"ms": out, "device": torch.cuda.get_device_name(0)}
    if block != "step_loop":
        info["persistent"] = env.get_option("last_rollout_persistent")
        info["launches"] = env.get_option("last_rollout_launches")
    env.close()
    return info


def _child(block, size, steps, reps, lib):
    env = dict(os.environ)
    if lib:
        env["RANENV_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", block, "--size", size, "--steps", str(steps), "--reps", str(reps)]
    res = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=600)
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--child", default=None, choices=("eight", "slice", "step_loop"))
    ap.add_argument("--size", default=None, choices=sorted(SIZES))
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.child, args.size, args.steps, args.reps)))
        return
    # every measurement in a process of its own: the parent of them all never opens the GPU
    record = {"probe": "slice_metrics", "steps": args.steps, "reps": args.reps, "alternations": args.alternations, "sizes": {}}
    for size in SIZES:
        series = {"this": [], "parent_a": [], "parent_b": [], "slice": [], "step_loop": []}
        sched = {}
        for _ in range(args.alternations):
            if args.baseline_lib:
                series["parent_a"] += _child("eight", size, args.steps, args.reps, args.baseline_lib)["ms"]
            r = _child("eight", size, args.steps, args.reps, None)
            series["this"] += r["ms"]
            sched["eight_sums"] = {"persistent": r["persistent"], "launches": r["launches"]}
            record["device"] = r["device"]
            if args.baseline_lib:
                series["parent_b"] += _child("eight", size, args.steps, args.reps, args.baseline_lib)["ms"]
            r = _child("slice", size, args.steps, args.reps, None)
            series["slice"] += r["ms"]
            sched["slice_metrics"] = {"persistent": r["persistent"], "launches": r["launches"]}
            series["step_loop"] += _child("step_loop", size, args.steps, 1, None)["ms"]
        med = {k: statistics.median(x) for k, x in series.items() if x}
        B = SIZES[size]["batch"]
        case = {"samples_ms": series, "schedule": sched, "eight_sums_this_ms": med["this"], "slice_metrics_ms": med["slice"],
                "step_loop_readback_ms": med["step_loop"], "slice_over_eight_sums": med["slice"] / med["this"],
                "slice_over_step_loop": med["slice"] / med["step_loop"],
                "slice_extra_us_per_tti": (med["slice"] - med["this"]) * 1e3 / args.steps,
                "env_steps_per_s": {k: B * args.steps / (med[k] * 1e-3) for k in ("this", "slice", "step_loop")}}
        if args.baseline_lib:
            parent = statistics.median(series["parent_a"] + series["parent_b"])
            spread = abs(med["parent_a"] / med["parent_b"] - 1.0)
            case.update({"eight_sums_parent_ms": parent, "parent_vs_parent": spread, "this_over_parent": med["this"] / parent,
                         "untaxed_within_spread": abs(med["this"] / parent - 1.0) <= spread})
        record["sizes"][size] = case
    line = json.dumps(record)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
