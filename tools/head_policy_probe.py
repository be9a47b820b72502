"""What the learned baselines cost on the device: rollout(K) and collect_head(K) under head actors (RANENV_POLICY_HEAD_NETWORK) in
SB3's shapes -- [64, 64] tanh PPO ("gauss_clip") and [256, 256] relu SAC ("gauss_tanh") -- at the two sizes of the DESIGN 4.p table.

Writes one JSON record to profiles/head_policy_probe.json (and prints it): per size
  mapf_heads_one_tti_ms           MAPF rollout with the head outputs bound, one TTI per launch: the same launches without an actor
  ibsched_inter_64x64_ms / _us    the IBSched inter-only [64, 64] actor in the same setting, and its cost per TTI over MAPF
  per net: rollout_ms             best of --reps, K TTIs
           actor_us_per_tti       (rollout - mapf_heads_one_tti) / K: the head actor's share of a TTI
           collect_ms, collect_extra_us_per_tti   collect_head(K) with everything recorded ("gauss_clip" nets only: SAC does not
                                  collect; for the SAC shape a gauss_clip actor of the same hidden widths is collected as well)
           host_paced_ms          the loop this replaces: a torch MLP on head_obs, clamp / tanh, env.step(scores) per TTI (what
                                  HeadVecEnv does, minus its copies to the host), and host_paced_over_rollout
With --baseline-lib PATH (a libranenv_hip.so built from the parent commit) rollout(K) under MAPF and under the IBSched [64, 64]
nets is also timed with that library and with this one in child processes of their own, ALTERNATING (--alternations times each):
`untaxed` lists every figure, each library's own run-to-run spread and the ratio of the best figures.

    python tools/head_policy_probe.py [--steps 200] [--reps 3] [--baseline-lib parent.so] [--alternations 2]
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
# name -> (hidden widths, activation, dist)
NETS = {"ppo_64x64": ([64, 64], "tanh", "gauss_clip"), "sac_256x256": ([256, 256], "relu", "gauss_tanh"),
        "ppo_256x256": ([256, 256], "relu", "gauss_clip")}
OUT = os.path.join(REPO, "profiles", "head_policy_probe.json")


def _mlp(torch, dims, act, seed):
    torch.manual_seed(seed)
    mods = []
    for i in range(len(dims) - 1):
        mods.append(torch.nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            mods.append(torch.nn.Tanh() if act == "tanh" else torch.nn.ReLU())
    return torch.nn.Sequential(*mods)


def _time(torch, env, fn, reps, warm=None):
    env.reset()
    (warm or (lambda: env.rollout(8)))()     # warm-up (first launches, queues)
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


def _workload(torch, _lib, kw):
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    return make_mult_slice_workload(device=torch.device("cuda", 0), policy=_lib.POLICY_MAPF, intra=_lib.INTRA_RR, n_scenarios=64, n_traces=64,
                                    trace_len=256, max_steps=100000, **kw)


def measure(steps, reps):
    import torch
    from intent_radio_sched_multi_slice_amd import _lib
    out = {}
    for size, kw in SIZES.items():
        B = kw["batch"]
        wl = _workload(torch, _lib, kw)
        env = wl.env
        S = env.S
        env.enable_heads()
        env.set_option("fuse", 1)
        mapf = _time(torch, env, lambda: env.rollout(steps), reps)
        env.set_option("fuse", 0)
        env.set_policy_network(_mlp(torch, [10 * S, 64, 64, 2 * S], "tanh", 1), None, stochastic=True, seed=1, fixed_intra=_lib.INTRA_RR)
        ib = _time(torch, env, lambda: env.rollout(steps), reps)
        case = {"mapf_heads_one_tti_ms": mapf, "ibsched_inter_64x64_ms": ib, "ibsched_inter_64x64_us_per_tti": (ib - mapf) * 1e3 / steps, "nets": {}}
        for name, (widths, act, dist) in NETS.items():
            clip = dist == "gauss_clip"
            actor = _mlp(torch, [10 * S] + widths + [S if clip else 2 * S], act, 2).to(env.device)
            log_std = torch.full((S,), -0.5) if clip else None
            env.set_head_policy_network(actor, dist, log_std, stochastic=True, seed=1, allow_sorted=True)
            c = {"rollout_ms": _time(torch, env, lambda: env.rollout(steps), reps)}
            c["actor_us_per_tti"] = (c["rollout_ms"] - mapf) * 1e3 / steps
            c["rollout_env_steps_per_s"] = B * steps / (c["rollout_ms"] * 1e-3)
            c["actor_over_ibsched_inter_64x64"] = c["actor_us_per_tti"] / max(case["ibsched_inter_64x64_us_per_tti"], 1e-9)
            if clip:
                env.set_head_value_network(_mlp(torch, [10 * S] + widths + [1], act, 3))
                rec = env.collect_head(steps)                 # (allocates the record)
                c["collect_ms"] = _time(torch, env, lambda: env.collect_head(steps), reps)
                c["collect_extra_us_per_tti"] = (c["collect_ms"] - c["rollout_ms"]) * 1e3 / steps
                c["collect_env_steps_per_s"] = B * steps / (c["collect_ms"] * 1e-3)
                c["record_bytes_per_env_step"] = sum(t[:steps].numel() * t.element_size() for t in rec.values()) // (B * steps)
                del rec
                env._keep.pop("head_trajectories", None)
            # the host-paced loop: the same actor as a torch module, one env.step() per TTI
            env.set_policy(_lib.POLICY_EXTERNAL, _lib.INTRA_RR)

            def host_loop(n=steps):
                with torch.no_grad():
                    for _ in range(n):
                        o = actor(env.head_obs)
                        a = o.clamp(-1.0, 1.0) if clip else torch.tanh(o[:, :S])
                        env.step(a.to(torch.float64))
            c["host_paced_ms"] = _time(torch, env, host_loop, reps, warm=lambda: host_loop(8))
            c["host_paced_env_steps_per_s"] = B * steps / (c["host_paced_ms"] * 1e-3)
            c["host_paced_over_rollout"] = c["host_paced_ms"] / c["rollout_ms"]
            case["nets"][name] = c
        out[size] = case
        env.close()
        del wl, env
        torch.cuda.empty_cache()
    out["device"] = torch.cuda.get_device_name(0)
    return out


def measure_existing(steps, reps):
    """rollout(K) under MAPF and under the IBSched [64, 64] nets, paths that exist in the parent commit's library too."""
    import ctypes
    import torch
    from intent_radio_sched_multi_slice_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.FUNCTIONS if not hasattr(raw, n)]:
        _lib.FUNCTIONS.pop(name)
    _lib.ABI_VERSION = raw.ranenv_abi_version()          # (the structs both versions share have not changed)
    out = {}
    for size, kw in SIZES.items():
        wl = _workload(torch, _lib, kw)
        env = wl.env
        S, Us = env.S, env.Us
        out[f"{size}/mapf"] = _time(torch, env, lambda: env.rollout(steps), reps)
        env.set_policy_network(_mlp(torch, [10 * S, 64, 64, 2 * S], "tanh", 1), _mlp(torch, [2 * Us + 9, 64, 64, 3], "tanh", 2), stochastic=True, seed=1)
        out[f"{size}/ibsched_64x64"] = _time(torch, env, lambda: env.rollout(steps), reps)
        env.close()
        del wl, env
        torch.cuda.empty_cache()
    return out


def _child(steps, reps, lib):
    env = dict(os.environ)
    if lib:
        env["RANENV_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child-existing", "--steps", str(steps), "--reps", str(reps)]
    res = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=600)
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--child-existing", action="store_true")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.steps, args.reps)))
        return
    if args.child_existing:
        print(json.dumps(measure_existing(args.steps, args.reps)))
        return
    # every measurement in a process of its own: the parent of them all never opens the GPU
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps), "--reps", str(args.reps)]
    res = json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=1000).stdout.strip().splitlines()[-1])
    record = {"probe": "head_policy", "steps": args.steps, "reps": args.reps, "device": res.pop("device"), "sizes": res}
    if args.baseline_lib:
        base, new = [], []
        for _ in range(args.alternations):
            base.append(_child(args.steps, args.reps, args.baseline_lib))
            new.append(_child(args.steps, args.reps, None))
        untaxed = {}
        for key in new[0]:
            b, n = [r[key] for r in base], [r[key] for r in new]
            untaxed[key] = {"baseline_ms": b, "this_ms": n, "baseline_spread": max(b) / min(b) - 1.0, "this_spread": max(n) / min(n) - 1.0,
                            "this_over_baseline": min(n) / min(b)}
            untaxed[key]["within_spread_plus_1pct"] = untaxed[key]["this_over_baseline"] <= 1.0 + untaxed[key]["baseline_spread"] + 0.01
        record["alternations"] = args.alternations
        record["untaxed"] = untaxed
    line = json.dumps(record)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
