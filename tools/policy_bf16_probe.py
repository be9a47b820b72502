"""What running the policy nets in bf16 buys (set_policy_network(precision="bf16"), RANENV_NET_BF16), and that the f32 path did not
pay for it: rollout(K) under f32 and bf16 nets over the four rows of DESIGN 4.p's table (two sizes x two nets), inter net only and
inter + intra nets, and collect(K) under either precision.

Writes one JSON document (default profiles/policy_bf16_probe.json) and prints it: per case
  rollout_ms {f32, bf16}         every alternation's figure (best of --reps each): the two precisions are re-bound and timed in turn,
                                 --alternations times, in one process on one device
  median_ms, env_steps_per_s     of those; bf16_speedup = median f32 / median bf16
  policy_us_per_tti              (median - the MAPF rollout with the same one-TTI launches) / K: the nets' share of a TTI
  collect_ms {f32, bf16}         collect(K), actors and critics of one precision, measured once (inter + intra cases)

With --baseline-lib PATH (a libranenv_hip.so built from the parent commit) this build's f32 rollouts are also timed against that
library, each in child processes of their own, alternating (--alternations times each, the order within a pair taking turns, same device, same job):
`baseline_rollout_ms` and `f32_rollout_ms_child` list both series, `baseline_spread` is the parent's own max / min - 1, and the f32
path counts as unchanged when `f32_vs_baseline` (median / median) lies inside that spread.

    python tools/policy_bf16_probe.py [--steps 200] [--reps 3] [--alternations 3] [--baseline-lib parent.so] [-o out.json]
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


def measure(steps, reps, alternations, precisions, with_collect):
    """One process's figures: a list of cases.  ``precisions`` ("f32",) is what a library of the parent commit can run."""
    import torch
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    dev = torch.device("cuda", 0)
    cases = []
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
            inter, intra = _mlp(torch, [10 * S] + widths + [2 * S], 1), _mlp(torch, [2 * Us + 9] + widths + [3], 2)
            for with_intra in (False, True):
                runs = {p: [] for p in precisions}
                for _ in range(alternations):
                    for p in precisions:
                        env.set_policy_network(inter, intra if with_intra else None, stochastic=True, seed=1, fixed_intra=_lib.INTRA_PF,
                                               **({} if p == "f32" else {"precision": p}))
                        runs[p].append(_time(torch, env, lambda: env.rollout(steps), reps))
                med = {p: statistics.median(v) for p, v in runs.items()}
                case = {"size": size, "net": net, "intra_net": with_intra, "mapf_one_tti_launches_ms": mapf1_ms, "rollout_ms": runs,
                        "median_ms": med, "env_steps_per_s": {p: B * steps / (m * 1e-3) for p, m in med.items()},
                        "policy_us_per_tti": {p: (m - mapf1_ms) * 1e3 / steps for p, m in med.items()}}
                if "bf16" in med:
                    case["bf16_speedup"] = med["f32"] / med["bf16"]
                    case["bf16_policy_speedup"] = (med["f32"] - mapf1_ms) / max(med["bf16"] - mapf1_ms, 1e-9)
                if with_collect and with_intra:
                    case["collect_ms"] = {}
                    for p in precisions:
                        env.set_policy_network(inter, intra, stochastic=True, seed=1, fixed_intra=_lib.INTRA_PF, precision=p)
                        env.set_value_network(_mlp(torch, [10 * S] + widths + [1], 3), _mlp(torch, [2 * Us + 9] + widths + [1], 4), precision=p)
                        env.collect(steps)                        # (allocates the record)
                        case["collect_ms"][p] = _time(torch, env, lambda: env.collect(steps), reps)
                    env._keep.pop("trajectories", None)
                cases.append(case)
                env.set_policy(_lib.POLICY_MAPF, _lib.INTRA_PF)
        env.close()
        del wl, env
        torch.cuda.empty_cache()
    return {"device": torch.cuda.get_device_name(0), "cases": cases}


def _child(steps, reps, lib):
    env = dict(os.environ)
    if lib:
        env["RANENV_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(steps), "--reps", str(reps)]
    res = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=600)
    return json.loads(res.stdout.strip().splitlines()[-1])["cases"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("-o", "--output", default=os.path.join(REPO, "profiles", "policy_bf16_probe.json"))
    ap.add_argument("--child", action="store_true", help="(internal) one process's f32 rollouts, one alternation, as JSON on stdout")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.steps, args.reps, 1, ("f32",), False)))
        return
    doc = {"probe": "policy_bf16", "steps": args.steps, "reps": args.reps, "alternations": args.alternations}
    if args.baseline_lib:       # first, while this process has not opened the GPU: each measurement in a process of its own
        base, new = [], []
        for k in range(args.alternations):
            for lib in ((args.baseline_lib, None) if k % 2 == 0 else (None, args.baseline_lib)):      # (who goes first takes turns)
                (base if lib else new).append(_child(args.steps, args.reps, lib))
            print(f"alternation {k + 1} of {args.alternations} against the baseline library done", file=sys.stderr, flush=True)
    res = measure(args.steps, args.reps, args.alternations, ("f32", "bf16"), True)
    doc["device"] = res["device"]
    doc["cases"] = res["cases"]
    if args.baseline_lib:
        for k, case in enumerate(doc["cases"]):
            b = [r[k]["rollout_ms"]["f32"][0] for r in base]
            n = [r[k]["rollout_ms"]["f32"][0] for r in new]
            case["baseline_rollout_ms"], case["f32_rollout_ms_child"] = b, n
            case["baseline_spread"] = max(b) / min(b) - 1.0
            case["f32_vs_baseline"] = statistics.median(n) / statistics.median(b)
    text = json.dumps(doc, indent=1)
    with open(args.output, "w") as f:
        f.write(text + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
