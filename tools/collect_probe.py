"""What recording a PPO batch costs: rollout(K) against collect(K) under the same actors (RANENV_POLICY_NETWORK), critics of the
actors' hidden widths, everything recorded; the four cases of the DESIGN 4.p table (two sizes x two nets, inter + intra nets).

Prints one JSON line: per case
  rollout_ms / collect_ms        best of --reps, K TTIs each
  policy_us_per_tti              (network rollout - MAPF rollout with one-TTI launches) / K: the actors' share of a TTI
  collect_extra_us_per_tti       (collect - rollout) / K: critics + record + GAE, to be held against policy_us_per_tti
  record_bytes_per_env_step      what the record writes per env and TTI
  collect_env_steps_per_s

With --baseline-lib PATH (a libranenv_hip.so built from the parent commit) the same rollouts are also timed with that library in
child processes of their own, ALTERNATING with this library's (--alternations times each, same box, same job): only such figures
compare, boxes differ by up to 12 %.  `baseline_rollout_ms` / `rollout_ms_runs` then list every alternation's figure; their spread is
the margin of everything above.

    python tools/collect_probe.py [--steps 200] [--reps 3] [--baseline-lib parent.so] [--alternations 2]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SIZES = {"B4096_S10_U100": dict(batch=4096, n_slices=10, n_ues=100, n_rbs=135, rbs_per_rbg=1, max_ues_slice=10),
         "B16384_S5_U25": dict(batch=16384, n_slices=5, n_ues=25, n_rbs=135, rbs_per_rbg=5, max_ues_slice=10)}
NETS = {"64x64": [64, 64], "512x3": [512, 512, 512]}
NEW_EXPORTS = ("ranenv_set_value_network", "ranenv_collect", "ranenv_gae")


def _mlp(torch, dims, seed):
    torch.manual_seed(seed)
    mods = []
    for i in range(len(dims) - 1):
        mods.append(torch.nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods)


def _time(torch, env, fn, reps):
    env.reset()
    env.rollout(8)                       # warm-up (first launches, queues)
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1)
        best = ms if best is None else min(best, ms)
    return best


def measure(steps, reps, with_collect):
    """One process's figures: {case: {...}}.  with_collect False: the rollouts alone (also what a library without the collect
    exports can run: the binding's table is trimmed to what it has)."""
    import torch
    from intent_radio_sched_multi_slice_amd import _lib
    if not with_collect:
        import ctypes
        raw = ctypes.CDLL(_lib.LIB_PATH)
        for name in NEW_EXPORTS:
            if not hasattr(raw, name):
                _lib.FUNCTIONS.pop(name, None)
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    dev = torch.device("cuda", 0)
    out = {}
    for size, kw in SIZES.items():
        B = kw["batch"]
        wl = make_mult_slice_workload(device=dev, policy=_lib.POLICY_MAPF, intra=_lib.INTRA_PF, n_scenarios=64, n_traces=64, trace_len=256,
                                      max_steps=100000, **kw)
        env = wl.env
        S, Us = env.S, env.Us
        env.set_option("fuse", 1)
        mapf1_ms = _time(torch, env, lambda: env.rollout(steps), reps)
        env.set_option("fuse", 0)
        for net, widths in NETS.items():
            env.set_policy_network(_mlp(torch, [10 * S] + widths + [2 * S], 1), _mlp(torch, [2 * Us + 9] + widths + [3], 2), stochastic=True, seed=1)
            case = {"mapf_one_tti_launches_ms": mapf1_ms, "rollout_ms": _time(torch, env, lambda: env.rollout(steps), reps)}
            case["policy_us_per_tti"] = (case["rollout_ms"] - mapf1_ms) * 1e3 / steps
            if with_collect:
                env.set_value_network(_mlp(torch, [10 * S] + widths + [1], 3), _mlp(torch, [2 * Us + 9] + widths + [1], 4))
                rec = env.collect(steps)                      # (allocates the record)
                for name, v in (("fused", 0), ("split", 1)):          # the critic behind the actor in one launch / in a launch of its own
                    env.set_option("collect_split", v)
                    case[f"collect_{name}_ms"] = _time(torch, env, lambda: env.collect(steps), reps)
                env.set_option("collect_split", -1)                   # the library's own choice
                case["collect_ms"] = _time(torch, env, lambda: env.collect(steps), reps)
                case["collect_extra_us_per_tti"] = (case["collect_ms"] - case["rollout_ms"]) * 1e3 / steps
                case["collect_env_steps_per_s"] = B * steps / (case["collect_ms"] * 1e-3)
                case["rollout_env_steps_per_s"] = B * steps / (case["rollout_ms"] * 1e-3)
                case["record_bytes_per_env_step"] = sum(t[:steps].numel() * t.element_size() for t in rec.values()) // (B * steps)
                case["algorithmic_bytes_per_env_step"] = env.algorithmic_bytes_per_env_step()
                del rec
                env._keep.pop("trajectories", None)
            out[f"{size}/{net}"] = case
            env.set_policy(_lib.POLICY_MAPF, _lib.INTRA_PF)
        env.close()
        del wl, env
        torch.cuda.empty_cache()
    out["device"] = torch.cuda.get_device_name(0)
    return out


def _child(steps, reps, lib, with_collect):
    env = dict(os.environ)
    if lib:
        env["RANENV_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(steps), "--reps", str(reps)] + ([] if with_collect else ["--rollout-only"])
    res = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=900)
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--rollout-only", action="store_true")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.steps, args.reps, not args.rollout_only)))
        return
    if not args.baseline_lib:
        res = measure(args.steps, args.reps, True)
        print(json.dumps({"probe": "collect", "steps": args.steps, "device": res.pop("device"), "cases": res}))
        return
    # every measurement in a process of its own (the parent of them all never opens the GPU), baseline and this library in turn
    base, new = [], []
    for _ in range(args.alternations):
        base.append(_child(args.steps, args.reps, args.baseline_lib, False))
        new.append(_child(args.steps, args.reps, None, True))
    cases = {}
    for key in [k for k in new[0] if k != "device"]:
        best = min(new, key=lambda r: r[key]["collect_ms"])[key]
        c = dict(best)
        c["rollout_ms_runs"] = [r[key]["rollout_ms"] for r in new]
        c["collect_ms_runs"] = [r[key]["collect_ms"] for r in new]
        c["baseline_rollout_ms"] = [r[key]["rollout_ms"] for r in base]
        c["baseline_policy_us_per_tti"] = [r[key]["policy_us_per_tti"] for r in base]
        b = min(c["baseline_rollout_ms"])
        c["baseline_spread"] = max(c["baseline_rollout_ms"]) / b - 1.0
        c["rollout_vs_baseline"] = min(c["rollout_ms_runs"]) / b
        c["collect_minus_baseline_us_per_tti"] = (min(c["collect_ms_runs"]) - b) * 1e3 / args.steps
        cases[key] = c
    print(json.dumps({"probe": "collect", "steps": args.steps, "alternations": args.alternations, "device": new[0]["device"], "cases": cases}))


if __name__ == "__main__":
    main()
