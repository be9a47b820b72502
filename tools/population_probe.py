"""What a population costs: rollout(K) and collect(K) under one net set against G = 8 and G = 64 member copies of the same shape
(ranenv_set_population / _population_policy / _population_value), members of equal size; two batch sizes x two nets.

Writes profiles/population_probe.json (and prints it as one line): per case and call, the MEDIAN over --blocks blocks, the blocks
alternating single / G8 / G64 within one process:
  single_*_ms / g8_*_ms / g64_*_ms     rollout and collect, K TTIs each; collect with option collect_split -1 (the library's rule)
  over_single                          the ratios

With --baseline-lib PATH (the parent commit's libranenv_hip.so) the single-net rollout(K) is also timed with that library in
processes of its own, ALTERNATING with this library's (--alternations each): `rollout_vs_baseline` is held against `baseline_spread`,
the parent library's own run-to-run spread in this job.

    python tools/population_probe.py [--steps 200] [--blocks 3] [--baseline-lib parent.so]
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
NETS = {"64x64": [64, 64], "512x3": [512, 512, 512]}
KINDS = {"single": 1, "g8": 8, "g64": 64}
NEW_EXPORTS = ("ranenv_set_population", "ranenv_get_population", "ranenv_set_population_policy", "ranenv_set_population_value",
               "ranenv_set_population_member", "ranenv_population_tiles")
OUT = os.path.join(REPO, "profiles", "population_probe.json")


def _mlp(torch, dims, seed):
    torch.manual_seed(seed)
    mods = []
    for i in range(len(dims) - 1):
        mods.append(torch.nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods)


def _time(torch, fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def measure(steps, blocks, what):
    """One process's figures: {case: {name: median ms}}.  what: "all", "single-rollout" (a library without the population exports can
    run it: the binding's table is trimmed to what the library has)."""
    import torch
    from intent_radio_sched_multi_slice_amd import _lib
    if what == "single-rollout":
        import ctypes
        raw = ctypes.CDLL(_lib.LIB_PATH)
        for name in NEW_EXPORTS:
            if not hasattr(raw, name):
                _lib.FUNCTIONS.pop(name, None)
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    dev = torch.device("cuda", 0)
    out = {}
    for size, kw in SIZES.items():
        wl = make_mult_slice_workload(device=dev, policy=_lib.POLICY_MAPF, intra=_lib.INTRA_PF, n_scenarios=64, n_traces=64, trace_len=256,
                                      max_steps=100000, **kw)
        env = wl.env
        S, W, B = env.S, env.W, env.B
        for net, widths in NETS.items():
            # (the copies are G references to one net: the library copies each into its own slot, which is what costs)
            inter, v_inter = _mlp(torch, [10 * S] + widths + [2 * S], 1), _mlp(torch, [10 * S] + widths + [1], 3)
            intra, v_intra = _mlp(torch, [W] + widths + [3], 10), _mlp(torch, [W] + widths + [1], 40)
            runs = {}

            def block(kind):
                G = KINDS[kind]
                if G == 1:
                    env.set_policy_network(inter, intra, stochastic=True, seed=1)
                else:
                    env.set_population()
                    env.set_population(sizes=[B // G] * G)
                    env.set_policy_network([inter] * G, [intra] * G, stochastic=True, seed=1)
                env.reset()
                env.rollout(8)                   # warm-up (first launches, queues)
                torch.cuda.synchronize()
                runs.setdefault(f"{kind}_rollout_ms", []).append(_time(torch, lambda: env.rollout(steps)))
                if what == "single-rollout":
                    return
                if G == 1:
                    env.set_value_network(v_inter, v_intra)
                else:
                    env.set_value_network([v_inter] * G, [v_intra] * G)
                env.collect(8)
                torch.cuda.synchronize()
                runs.setdefault(f"{kind}_collect_ms", []).append(_time(torch, lambda: env.collect(steps)))
            for _ in range(blocks):
                for kind in {"all": tuple(KINDS), "single-rollout": ("single",)}[what]:
                    block(kind)
            case = {name: statistics.median(v) for name, v in runs.items()}
            case["runs"] = runs
            out[f"{size}/{net}"] = case
            env._keep.pop("trajectories", None)
            env.set_policy(_lib.POLICY_MAPF, _lib.INTRA_PF)
        env.close()
        del wl, env
        torch.cuda.empty_cache()
    out["device"] = torch.cuda.get_device_name(0)
    return out


def _child(steps, blocks, lib, what):
    env = dict(os.environ)
    if lib:
        env["RANENV_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--steps", str(steps), "--blocks", str(blocks)]
    res = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=900)
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.steps, args.blocks, args.child)))
        return
    # every measurement in a process of its own (the parent of them all never opens the GPU): the libraries in turn
    base, new = [], []
    for _ in range(args.alternations if args.baseline_lib else 1):
        if args.baseline_lib:
            base.append(_child(args.steps, args.blocks, args.baseline_lib, "single-rollout"))
        new.append(_child(args.steps, args.blocks, None, "all"))
    cases = {}
    for key in [k for k in new[0] if k != "device"]:
        names = [n for n in new[0][key] if n != "runs"]
        c = {n: statistics.median(r[key][n] for r in new) for n in names}
        c["process_runs"] = {n: [r[key][n] for r in new] for n in names}
        c["over_single"] = {f"{kind}_{call}": c[f"{kind}_{call}_ms"] / c[f"single_{call}_ms"] for kind in ("g8", "g64") for call in ("rollout", "collect")}
        if base:
            runs = [r[key]["single_rollout_ms"] for r in base]
            c["baseline_rollout_ms"] = runs
            c["baseline_spread"] = max(runs) / min(runs) - 1.0
            c["rollout_vs_baseline"] = c["single_rollout_ms"] / statistics.median(runs)
        cases[key] = c
    line = json.dumps({"probe": "population", "steps": args.steps, "blocks": args.blocks, "alternations": len(new),
                       "device": new[0]["device"], "cases": cases})
    with open(OUT, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
