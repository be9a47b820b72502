"""What a MIXED population costs (ranenv_set_population_policy_mixed / _value_mixed, per-member gamma / lambda): rollout(K) and
collect(K) at the two sizes the other probes use, four comparisons, the variants of each alternating block by block in one process
and the MEDIAN over --blocks blocks reported.

  (a) one net set ([64, 64]) on this build against the parent commit's library (--baseline-lib), each in processes of its own,
      alternating: `vs_baseline` is held against `baseline_spread`, the parent library's own run-to-run spread in this job.
  (b) G = 8 and G = 64 copies of one [64, 64] set and of one [512] x 3 set through the uniform path and through the mixed path:
      `mixed_over_uniform` is the cost of the descriptor table.
  (c) the reference's five architectures (agents/ray_agent.py:61-67) spread evenly over G = 10 and G = 60 members in one mixed batch
      against the SUM of five uniform-population passes, one per architecture with G / 5 members on a handle of B // 5 envs -- what a
      user had to do before: `mixed_over_split`.
  (d) the mixed batch of (c) collected with per-member gamma / lambda against scalars: `pairs_over_scalars`.

Writes profiles/mixed_population_probe.json (and prints it as one line).

    python tools/mixed_population_probe.py [--steps 200] [--blocks 3] [--baseline-lib parent.so]
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
ARCHS = [[64, 64], [256, 256], [400, 300], [256, 256, 256], [512, 512, 512]]      # agents/ray_agent.py:61-67
GAMMA = [0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.98, 0.99, 0.995, 0.999, 0.9999]           # :112-126
LAMBDA = [0.8, 0.9, 0.92, 0.95, 0.98, 0.99, 1.0]                                   # :128
NEW_EXPORTS = ("ranenv_set_population_policy_mixed", "ranenv_set_population_value_mixed", "ranenv_get_population_net", "ranenv_packed_net_floats",
               "ranenv_set_population_gae", "ranenv_gae_population")
OUT = os.path.join(REPO, "profiles", "mixed_population_probe.json")


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


def _sizes(n, parts):
    """n envs over `parts` members as evenly as integers allow"""
    edges = [n * k // parts for k in range(parts + 1)]
    return [b - a for a, b in zip(edges[:-1], edges[1:])]


def measure(steps, blocks, what):
    """One process's figures: {case: {name: median ms, "runs": ...}}.  what "single": variant (a)'s side alone (a library without the
    new exports can run it: the binding's table is trimmed to what the library has), "all": (a)'s side, (b), (c) and (d)."""
    import torch
    from intent_radio_sched_multi_slice_amd import _lib
    if what == "single":
        import ctypes
        raw = ctypes.CDLL(_lib.LIB_PATH)
        for name in NEW_EXPORTS:
            if not hasattr(raw, name):
                _lib.FUNCTIONS.pop(name, None)
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    dev = torch.device("cuda", 0)
    out = {}

    def nets_of(env, widths, seed):
        S, W = env.S, env.W
        return (_mlp(torch, [10 * S] + widths + [2 * S], seed), _mlp(torch, [W] + widths + [3], seed + 1),
                _mlp(torch, [10 * S] + widths + [1], seed + 2), _mlp(torch, [W] + widths + [1], seed + 3))

    def timed(env, runs, name, bind, **collect_kw):
        """bind, warm up, time rollout(steps) and collect(steps)"""
        bind(env)
        env.reset()
        env.rollout(8)
        env.collect(8, **collect_kw)
        torch.cuda.synchronize()
        runs.setdefault(name + "_rollout_ms", []).append(_time(torch, lambda: env.rollout(steps)))
        runs.setdefault(name + "_collect_ms", []).append(_time(torch, lambda: env.collect(steps, **collect_kw)))

    def one(nets):
        def bind(env):
            env.set_population()
            env.set_policy_network(nets[0], nets[1], stochastic=True, seed=1)
            env.set_value_network(nets[2], nets[3])
        return bind

    def population(lists, sizes, mixed):
        def bind(env):
            env.set_population()
            env.set_population(sizes=sizes)
            env.set_policy_network(lists[0], lists[1], stochastic=True, seed=1, mixed=mixed)
            env.set_value_network(lists[2], lists[3], mixed=mixed)
        return bind

    def finish(key, runs):
        case = {name: statistics.median(v) for name, v in runs.items()}
        case["runs"] = runs
        out[key] = case

    for size, kw in SIZES.items():
        mk = lambda **over: make_mult_slice_workload(device=dev, policy=_lib.POLICY_MAPF, intra=_lib.INTRA_PF, n_scenarios=64, n_traces=64,  # noqa: E731
                                                     trace_len=256, max_steps=100000, **{**kw, **over})
        wl = mk()
        env = wl.env
        B = env.B
        # (a) one net set
        runs, single = {}, nets_of(env, NETS["64x64"], 1)
        for _ in range(blocks):
            timed(env, runs, "single", one(single))
        finish(f"{size}/a", runs)
        if what == "single":
            env.close()
            continue
        # (b) copies of one set: the uniform path against the mixed path
        for net, widths in NETS.items():
            runs, nets = {}, nets_of(env, widths, 1)
            for _ in range(blocks):
                for G in (8, 64):
                    lists = tuple([x] * G for x in nets)
                    for mixed in (False, True):
                        timed(env, runs, f"g{G}_{'mixed' if mixed else 'uniform'}", population(lists, _sizes(B, G), mixed))
            finish(f"{size}/b/{net}", runs)
        # (c) five architectures in one mixed batch against five uniform passes on B // 5 envs; (d) per-member gamma / lambda
        wl5 = mk(batch=B // 5)
        env5 = wl5.env
        arch_nets = [nets_of(env, widths, 10 + 10 * a) for a, widths in enumerate(ARCHS)]
        for G in (10, 60):
            runs, per = {}, G // 5
            member_arch = [m // per for m in range(G)]                      # architecture-major: the members of one architecture are neighbours
            arch_envs = _sizes(B, 5)
            sizes = [s for a in range(5) for s in _sizes(arch_envs[a], per)]
            lists = tuple([arch_nets[a][r] for a in member_arch] for r in range(4))
            gamma, lam = [GAMMA[m % len(GAMMA)] for m in range(G)], [LAMBDA[m % len(LAMBDA)] for m in range(G)]
            for _ in range(blocks):
                timed(env, runs, "mixed", population(lists, sizes, True))
                timed(env, runs, "mixed_pairs", population(lists, sizes, True), gamma=gamma, lam=lam)
                for a in range(5):
                    timed(env5, runs, f"split_arch{a}", population(tuple([x] * per for x in arch_nets[a]), _sizes(B // 5, per), False))
            for call in ("rollout", "collect"):
                runs[f"split_{call}_ms"] = [sum(runs[f"split_arch{a}_{call}_ms"][k] for a in range(5)) for k in range(blocks)]
            finish(f"{size}/c/g{G}", runs)
            env._keep.pop("trajectories", None)
        env5.close()
        env.close()
        del wl, env, wl5, env5
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
            base.append(_child(args.steps, args.blocks, args.baseline_lib, "single"))
        new.append(_child(args.steps, args.blocks, None, "all"))
    cases = {}
    for key in [k for k in new[0] if k != "device"]:
        names = [n for n in new[0][key] if n != "runs" and not n.startswith("split_arch")]
        c = {n: statistics.median(r[key][n] for r in new) for n in names}
        c["process_runs"] = {n: [r[key][n] for r in new] for n in names}
        kind = key.split("/")[1]
        for call in ("rollout", "collect"):
            if kind == "a" and base:
                runs = [r[key][f"single_{call}_ms"] for r in base]
                c[f"baseline_{call}_ms"] = runs
                c[f"baseline_{call}_spread"] = max(runs) / min(runs) - 1.0
                c[f"{call}_vs_baseline"] = c[f"single_{call}_ms"] / statistics.median(runs)
            if kind == "b":
                c.setdefault("mixed_over_uniform", {}).update({f"g{G}_{call}": c[f"g{G}_mixed_{call}_ms"] / c[f"g{G}_uniform_{call}_ms"] for G in (8, 64)})
            if kind == "c":
                c.setdefault("mixed_over_split", {})[call] = c[f"mixed_{call}_ms"] / c[f"split_{call}_ms"]
                c.setdefault("pairs_over_scalars", {})[call] = c[f"mixed_pairs_{call}_ms"] / c[f"mixed_{call}_ms"]
        cases[key] = c
    line = json.dumps({"probe": "mixed_population", "steps": args.steps, "blocks": args.blocks, "alternations": len(new),
                       "device": new[0]["device"], "cases": cases})
    with open(OUT, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
