"""What the reference's IBSchedSB3 (agents/sb3_sched.py: an SB3 actor on IBSched's own player_0 observation) costs on the device:
rollout(K), collect_head(K) and collect_replay(K) under RANENV_POLICY_HEAD_NETWORK with the head policy source "inter", beside the
head source, at the two sizes of the DESIGN 4.p table, under SB3's shapes -- [64, 64] tanh PPO ("gauss_clip") and [256, 256] relu SAC
("gauss_tanh").

Writes one JSON record to profiles/inter_head_probe.json (and prints it).  Per size and net, each call timed under the variants
  a_inter         source "inter", no head outputs bound: no head kernel behind the steps
  b_inter_heads   source "inter", head outputs bound: the head kernel runs and nobody reads its rows
  c_head          source "head": the SchedTWC / SchedColORAN path
  e_host_paced    (rollout only) the loop this replaces: a torch MLP on obs_inter, clamp / tanh, env.step(scores) per TTI -- what
                  adapters.InterVecEnv does, minus its copies to the host
collect_head is timed for the "gauss_clip" net only (SAC does not collect).  The variants run in BLOCKS that alternate (--alternations
times a, b, c, e in turn), each figure the best of --reps inside its block; reported are every block's figure, their median, the
block-to-block spread (max / min - 1) and the ratios a / c and b / c of the medians.
With --baseline-lib PATH (a libranenv_hip.so built from the parent commit): (d) rollout(K) under the head source and under MAPF, paths
the parent's library has too, timed with that library and with this one in child processes of their own, alternating; `untaxed` lists
every figure, each library's own run-to-run spread and the ratio of the medians.  What to hold the numbers against: (a) enqueues one
launch fewer per TTI than (c) and should not be slower than (c) beyond the parent-against-parent spread of the same job; (c) and the
MAPF rollout must stay within that spread of the parent's library, because nothing they enqueue changes.

    python tools/inter_head_probe.py [--steps 200] [--reps 3] [--alternations 3] [--baseline-lib parent.so]
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
# name -> (hidden widths, activation, dist)
NETS = {"ppo_64x64": ([64, 64], "tanh", "gauss_clip"), "sac_256x256": ([256, 256], "relu", "gauss_tanh")}
OUT = os.path.join(REPO, "profiles", "inter_head_probe.json")
RING_SLOTS = 8            # (a call of K TTIs needs K slots: the ring is bound with max(K, RING_SLOTS))


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


def _summary(blocks):
    return {"blocks_ms": blocks, "median_ms": statistics.median(blocks), "spread": max(blocks) / min(blocks) - 1.0}


def measure(steps, reps, alternations):
    import torch
    from intent_radio_sched_multi_slice_amd import _lib
    out = {}
    for size, kw in SIZES.items():
        B = kw["batch"]
        # two envs of one workload shape: without and with head outputs (binding them is not undone here)
        bare, heads = _workload(torch, _lib, kw).env, _workload(torch, _lib, kw).env
        heads.enable_heads()
        S = bare.S
        case = {}
        for name, (widths, act, dist) in NETS.items():
            clip = dist == "gauss_clip"
            actor = _mlp(torch, [10 * S] + widths + [S if clip else 2 * S], act, 2).to(bare.device)
            critic = _mlp(torch, [10 * S] + widths + [1], act, 3) if clip else None
            log_std = torch.full((S,), -0.5) if clip else None

            def bind(env, observation):
                env.set_head_policy_network(actor, dist, log_std, stochastic=True, seed=1, allow_sorted=True, observation=observation)
                if critic is not None:
                    env.set_head_value_network(critic)
                env.bind_replay(max(steps, RING_SLOTS))          # (after the source: changing it unbinds a ring)

            def host_loop(n=steps):
                with torch.no_grad():
                    for _ in range(n):
                        o = actor(bare.obs_inter)
                        a = o.clamp(-1.0, 1.0) if clip else torch.tanh(o[:, :S])
                        bare.step(a.to(torch.float64))

            variants = {"a_inter": (bare, "inter"), "b_inter_heads": (heads, "inter"), "c_head": (heads, "head")}
            calls = {"rollout": lambda env: env.rollout(steps), "collect_replay": lambda env: env.collect_replay(steps)}
            if clip:
                calls["collect_head"] = lambda env: env.collect_head(steps)
            figures = {c: {v: [] for v in variants} for c in calls}
            figures["rollout"]["e_host_paced"] = []
            for _ in range(alternations):
                for v, (env, observation) in variants.items():
                    bind(env, observation)
                    for c, fn in calls.items():
                        figures[c][v].append(_time(torch, env, lambda: fn(env), reps, warm=lambda: fn(env)))
                    env._keep.pop("head_trajectories", None)
                    env._keep.pop("inter_head_trajectories", None)
                bare.set_policy(_lib.POLICY_EXTERNAL, _lib.INTRA_RR)
                figures["rollout"]["e_host_paced"].append(_time(torch, bare, host_loop, reps, warm=lambda: host_loop(8)))
            net = {}
            for c, per in figures.items():
                net[c] = {v: _summary(b) for v, b in per.items()}
                med = {v: net[c][v]["median_ms"] for v in per}
                net[c]["a_over_c"] = med["a_inter"] / med["c_head"]
                net[c]["b_over_c"] = med["b_inter_heads"] / med["c_head"]
                net[c]["a_env_steps_per_s"] = B * steps / (med["a_inter"] * 1e-3)
                if "e_host_paced" in med:
                    net[c]["host_paced_over_a"] = med["e_host_paced"] / med["a_inter"]
                    net[c]["host_paced_env_steps_per_s"] = B * steps / (med["e_host_paced"] * 1e-3)
            case[name] = net
        out[size] = case
        for env in (bare, heads):
            env.close()
        del bare, heads
        torch.cuda.empty_cache()
    out["device"] = torch.cuda.get_device_name(0)
    return out


def measure_existing(steps, reps):
    """rollout(K) under MAPF and under a head-source [64, 64] actor: paths that exist in the parent commit's library too."""
    import ctypes
    import torch
    from intent_radio_sched_multi_slice_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in _lib.FUNCTIONS if not hasattr(raw, n)]
    for name in missing:
        _lib.FUNCTIONS.pop(name)
    _lib.ABI_VERSION = raw.ranenv_abi_version()          # (the structs both versions share have not changed)
    out = {}
    for size, kw in SIZES.items():
        wl = _workload(torch, _lib, kw)
        env = wl.env
        S = env.S
        out[f"{size}/mapf"] = _time(torch, env, lambda: env.rollout(steps), reps)
        env.enable_heads()
        if "ranenv_set_head_policy_source" in missing:       # the parent's library: the head source is all there is
            env._lib.ranenv_set_head_policy_source = lambda h, source: 0
        env.set_head_policy_network(_mlp(torch, [10 * S, 64, 64, S], "tanh", 2), "gauss_clip", torch.full((S,), -0.5), stochastic=True, seed=1,
                                    allow_sorted=True)
        out[f"{size}/head_source_64x64"] = _time(torch, env, lambda: env.rollout(steps), reps)
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
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--child-existing", action="store_true")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.steps, args.reps, args.alternations)))
        return
    if args.child_existing:
        print(json.dumps(measure_existing(args.steps, args.reps)))
        return
    # every measurement in a process of its own: the parent of them all never opens the GPU
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps), "--reps", str(args.reps), "--alternations",
           str(args.alternations)]
    res = json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=1100).stdout.strip().splitlines()[-1])
    record = {"probe": "inter_head", "steps": args.steps, "reps": args.reps, "alternations": args.alternations, "device": res.pop("device"),
              "sizes": res}
    if args.baseline_lib:
        base, new = [], []
        for _ in range(args.alternations):
            base.append(_child(args.steps, args.reps, args.baseline_lib))
            new.append(_child(args.steps, args.reps, None))
        untaxed = {}
        for key in new[0]:
            b, n = [r[key] for r in base], [r[key] for r in new]
            untaxed[key] = {"baseline_ms": b, "this_ms": n, "baseline_spread": max(b) / min(b) - 1.0, "this_spread": max(n) / min(n) - 1.0,
                            "this_over_baseline": statistics.median(n) / statistics.median(b)}
            untaxed[key]["within_baseline_spread"] = untaxed[key]["this_over_baseline"] <= 1.0 + untaxed[key]["baseline_spread"]
        record["untaxed"] = untaxed
    line = json.dumps(record)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
