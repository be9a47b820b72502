"""Throughput of rollouts under trained-policy nets on the device (RANENV_POLICY_NETWORK), next to the MAPF rollout.

Prints one JSON line: per case (batch size x net x with / without an intra net)
  env_steps_per_s      of rollout(K) under the network policy (nets + step, one TTI per launch)
  policy_us_per_tti    (network rollout - MAPF rollout with option fuse = 1, the same one-TTI launches without the nets) / K:
                       the nets' share of a TTI, by difference
  policy_tflops        FLOPs of the nets per TTI (2 x rows x sum of in x out) / policy_us_per_tti, and its share of the 157 TF
                       FP32-matrix peak
  mapf_env_steps_per_s the MAPF rollout with the library's own schedule (fused launches), for context

    python tools/policy_rollout_probe.py [--steps 200] [--reps 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from intent_radio_sched_multi_slice_amd import _lib  # noqa: E402
from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload  # noqa: E402

PEAK_TF = 157.3
SIZES = {"B4096_S10_U100": dict(batch=4096, n_slices=10, n_ues=100, n_rbs=135, rbs_per_rbg=1, max_ues_slice=10),
         "B16384_S5_U25": dict(batch=16384, n_slices=5, n_ues=25, n_rbs=135, rbs_per_rbg=5, max_ues_slice=10)}
NETS = {"64x64": [64, 64], "512x3": [512, 512, 512]}


def _mlp(dims, seed):
    torch.manual_seed(seed)
    mods = []
    for i in range(len(dims) - 1):
        mods.append(torch.nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods)


def _flops(rows, dims):
    return 2.0 * rows * sum(a * b for a, b in zip(dims[:-1], dims[1:]))


def _time(env, steps, reps):
    env.reset()
    env.rollout(8)                       # warm-up (first launches, queues)
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        env.rollout(steps)
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1)
        best = ms if best is None else min(best, ms)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"probe": "policy_rollout", "steps": args.steps, "peak_fp32_matrix_tflops": PEAK_TF, "cases": []}
    for size, kw in SIZES.items():
        B = kw["batch"]
        wl = make_mult_slice_workload(device=dev, policy=_lib.POLICY_MAPF, intra=_lib.INTRA_PF, n_scenarios=64, n_traces=64, trace_len=256,
                                      max_steps=100000, **kw)
        env = wl.env
        S, Us = env.S, env.Us
        mapf_ms = _time(env, args.steps, args.reps)
        env.set_option("fuse", 1)
        mapf1_ms = _time(env, args.steps, args.reps)
        env.set_option("fuse", 0)
        out["cases"].append({"size": size, "policy": "MAPF", "env_steps_per_s": B * args.steps / (mapf_ms * 1e-3),
                             "one_tti_launches_env_steps_per_s": B * args.steps / (mapf1_ms * 1e-3)})
        for net, widths in NETS.items():
            for with_intra in (False, True):
                inter = _mlp([10 * S] + widths + [2 * S], 1)
                intra = _mlp([2 * Us + 9] + widths + [3], 2) if with_intra else None
                env.set_policy_network(inter, intra, fixed_intra=_lib.INTRA_PF)
                ms = _time(env, args.steps, args.reps)
                flops = _flops(B, [10 * S] + widths + [2 * S]) + (_flops(B * S, [2 * Us + 9] + widths + [3]) if with_intra else 0.0)
                pol_us = max(ms - mapf1_ms, 0.0) * 1e3 / args.steps
                out["cases"].append({
                    "size": size, "net": net, "intra_net": with_intra,
                    "env_steps_per_s": B * args.steps / (ms * 1e-3),
                    "vs_mapf_rollout": (mapf_ms / ms),
                    "policy_gflop_per_tti": flops * 1e-9,
                    "policy_us_per_tti": pol_us,
                    "policy_tflops": (flops / (pol_us * 1e-6) * 1e-12) if pol_us > 0 else None,
                    "policy_frac_of_peak": (flops / (pol_us * 1e-6) * 1e-12 / PEAK_TF) if pol_us > 0 else None})
                env.set_policy(_lib.POLICY_MAPF, _lib.INTRA_PF)
        env.close()
        del wl
        torch.cuda.empty_cache()
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
