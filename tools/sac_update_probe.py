"""What the device SAC update costs per gradient step, against the eager-torch step it replaces -- and that nothing else moved.

  update           `env.sac_update` per step for [256, 256] relu nets at S 5 and S 10, minibatch 256 (SB3's) and 4096, against the
                   eager-torch step of examples/train_sac_on_device.py on the same rows (`env.sac_targets` on the device, then the three
                   losses, three torch.optim.Adam and the polyak loop in torch).  One child process per (S, minibatch); inside it blocks
                   of --steps steps alternate device / torch, --reps times; medians of the per-step wall time.
  rollout, replay  `rollout(200)` and `collect_replay(200)` at B 4096, S 10, U 100 with this library and, with --baseline-lib (the parent
                   commit's libranenv_hip.so, loaded through RANENV_LIB), with the parent's: each sample in a child of its own, the parent
                   measured twice per round.  `parent_vs_parent` is the spread of the two parent series' medians and
                   `within_parent_spread` whether this build's median lies inside it -- a strict flag: two medians of 15 and more
                   samples each agree to 1e-4 while single runs of the parent differ by 0.5 % --; `parent_run_medians_ms` is the range of
                   the parent's per-process medians, `this_median_within_parent_runs` whether this build's median lies inside that, and
                   `this_median_within_parent_range` whether it lies among the parent's samples (the kernels those calls launch are the
                   parent's instruction for instruction: tools/isa_compare.py).

    python tools/sac_update_probe.py [--steps 20] [--reps 5] [--alternations 3] [--baseline-lib parent.so] [--out FILE]

Writes one JSON line to profiles/sac_update_probe.json (and prints it).
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

SIZES = {5: dict(n_slices=5, n_ues=25, n_rbs=135, rbs_per_rbg=5, max_ues_slice=10), 10: dict(n_slices=10, n_ues=100, n_rbs=135, rbs_per_rbg=1, max_ues_slice=10)}
OUT = os.path.join(REPO, "profiles", "sac_update_probe.json")
GAMMA, TAU, LR = 0.99, 0.005, 3e-4


def _mlp(n_in, n_out, width=256):
    import torch
    return torch.nn.Sequential(torch.nn.Linear(n_in, width), torch.nn.ReLU(), torch.nn.Linear(width, width), torch.nn.ReLU(), torch.nn.Linear(width, n_out))


def _env(S, batch, heads=True):
    import ctypes
    import numpy as np
    import torch
    from intent_radio_sched_multi_slice_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.FUNCTIONS if not hasattr(raw, n)]:      # (the parent commit's library lacks the new functions)
        _lib.FUNCTIONS.pop(name)
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    wl = make_mult_slice_workload(batch, torch.device("cuda", 0), policy=_lib.POLICY_MAPF, intra=_lib.INTRA_RR, n_scenarios=64, n_traces=64,
                                  trace_len=256, max_steps=100000, **SIZES[S])
    env = wl.env
    if heads:
        wl.tables.sorted_slices[...] = np.arange(S, dtype=np.int32)
        env.load_scenarios(wl.tables)
        env.enable_heads(np.ones_like(wl.tables.slice_active, dtype=np.int32))
    return env


def measure_update(S, minibatch, steps, reps):
    """Blocks of `steps` gradient steps, device and eager torch alternated -> per-step milliseconds of each block"""
    import copy
    import math
    import torch
    dev = torch.device("cuda", 0)
    env = _env(S, 64)
    torch.manual_seed(0)
    actor, q1, q2 = _mlp(10 * S, 2 * S).to(dev), _mlp(11 * S, 1).to(dev), _mlp(11 * S, 1).to(dev)
    env.set_head_policy_network(actor, "gauss_tanh", stochastic=True, seed=1)
    env.set_sac_critics(q1, q2)
    env.sac_bind(ent_coef="auto", slabs=32)
    n = steps * minibatch
    g = torch.Generator(device=dev).manual_seed(1)
    batch = {"obs": torch.rand((n, 10 * S), generator=g, device=dev), "next_obs": torch.rand((n, 10 * S), generator=g, device=dev),
             "action": torch.rand((n, S), generator=g, device=dev) * 2 - 1, "reward": torch.randn(n, generator=g, device=dev),
             "done": (torch.rand(n, generator=g, device=dev) < 0.05).to(torch.uint8)}
    # the eager-torch learner of examples/train_sac_on_device.py
    q1_t, q2_t = copy.deepcopy(q1), copy.deepcopy(q2)
    log_alpha = torch.zeros((), device=dev, requires_grad=True)
    opt_actor, opt_q, opt_alpha = (torch.optim.Adam(p, lr=LR) for p in (actor.parameters(), list(q1.parameters()) + list(q2.parameters()), [log_alpha]))
    half_ln_2pi = 0.5 * math.log(2.0 * math.pi)

    def torch_steps():
        for k in range(steps):
            r = slice(k * minibatch, (k + 1) * minibatch)
            obs, act = batch["obs"][r], batch["action"][r]
            alpha = float(log_alpha.exp())
            target = env.sac_targets(batch["next_obs"][r], batch["reward"][r], batch["done"][r], gamma=GAMMA, ent_coef=alpha, stochastic=True, seed=13,
                                     draw=k, outputs=("target",))["target"]
            xa = torch.cat([obs, act], dim=1)
            loss_q = 0.5 * ((q1(xa)[:, 0] - target).pow(2).mean() + (q2(xa)[:, 0] - target).pow(2).mean())
            opt_q.zero_grad(set_to_none=True)
            loss_q.backward()
            opt_q.step()
            out = actor(obs)
            mu, ls = out[:, :S], out[:, S:].clamp(-20.0, 2.0)
            z = torch.randn_like(mu)
            a = torch.tanh(mu + torch.exp(ls) * z)
            logp = (-0.5 * z * z - ls - half_ln_2pi).sum(-1) - torch.log(1.0 - a * a + 1e-6).sum(-1)
            loss_alpha = -(log_alpha * (logp.detach() - float(S))).mean()
            opt_alpha.zero_grad(set_to_none=True)
            loss_alpha.backward()
            opt_alpha.step()
            xa = torch.cat([obs, a], dim=1)
            loss_pi = (alpha * logp - torch.minimum(q1(xa)[:, 0], q2(xa)[:, 0])).mean()
            opt_actor.zero_grad(set_to_none=True)
            loss_pi.backward()
            opt_actor.step()
            with torch.no_grad():
                for net, tgt in ((q1, q1_t), (q2, q2_t)):
                    for p, pt in zip(net.parameters(), tgt.parameters()):
                        pt.mul_(1.0 - TAU).add_(p, alpha=TAU)

    def device_steps():
        env.sac_update(batch, steps, minibatch=minibatch, lr=LR, gamma=GAMMA, tau=TAU, seed=13, draw=0)

    out = {"device": [], "torch": []}
    for name, fn in (("device", device_steps), ("torch", torch_steps)):      # (warm-up: code objects, allocator, optimiser state)
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, fn in (("device", device_steps), ("torch", torch_steps)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) * 1e3 / steps)
    info = {"ms_per_step": out, "device": torch.cuda.get_device_name(0), "lds_bytes": env.sac_layout()["lds_bytes"],
            "tiles": -(-minibatch // 32), "workgroups": min(-(-minibatch // 32), 32)}
    env.close()
    return info


def measure_env(block, steps, reps):
    """rollout(steps) or collect_replay(steps) at B 4096, S 10 under a [256, 256] head actor -> samples in ms"""
    import torch
    S, B = 10, 4096
    env = _env(S, B)
    torch.manual_seed(0)
    env.set_head_policy_network(_mlp(10 * S, 2 * S), "gauss_tanh", stochastic=True, seed=1)
    if block == "replay":
        env.bind_replay(steps)
    fn = (lambda: env.collect_replay(steps)) if block == "replay" else (lambda: env.rollout(steps))
    env.reset()
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1))
    env.close()
    return {"ms": out}


def summarise(series, reps, with_parent):
    """The figures of one block from its samples (`reps` per child, the children in the order they ran)"""
    case = {"samples_ms": series, "this_ms": statistics.median(series["this"])}
    if with_parent:
        pa, pb = statistics.median(series["parent_a"]), statistics.median(series["parent_b"])
        both = series["parent_a"] + series["parent_b"]
        parent, spread = statistics.median(both), abs(pa / pb - 1.0)
        # (a child is one process: its median is one run of the parent library; their range is the parent's run-to-run spread)
        runs = [statistics.median(x[i:i + reps]) for x in (series["parent_a"], series["parent_b"]) for i in range(0, len(x), reps)]
        case.update({"parent_ms": parent, "parent_vs_parent": spread, "this_over_parent": case["this_ms"] / parent,
                     "within_parent_spread": abs(case["this_ms"] / parent - 1.0) <= spread, "parent_range_ms": [min(both), max(both)],
                     "this_median_within_parent_range": min(both) <= case["this_ms"] <= max(both),
                     "parent_run_medians_ms": [min(runs), max(runs)], "this_median_within_parent_runs": min(runs) <= case["this_ms"] <= max(runs)})
    return case


def _child(args, block, lib=None, S=0, minibatch=0):
    env = dict(os.environ)
    if lib:
        env["RANENV_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", block, "--steps", str(args.steps if block == "update" else args.ttis), "--reps", str(args.reps),
           "--S", str(S), "--minibatch", str(minibatch)]
    res = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=600)
    print(f"[sac_update_probe] {block} S {S} minibatch {minibatch} ({'parent' if lib else 'this build'}) done", file=sys.stderr, flush=True)
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="gradient steps per block")
    ap.add_argument("--ttis", type=int, default=200, help="TTIs of a rollout / collect_replay sample")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--child", default=None, choices=("update", "rollout", "replay"))
    ap.add_argument("--S", type=int, default=0)
    ap.add_argument("--minibatch", type=int, default=0)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure_update(args.S, args.minibatch, args.steps, args.reps) if args.child == "update" else measure_env(args.child, args.steps, args.reps)))
        return
    # every measurement in a process of its own: the parent of them all never opens the GPU
    record = {"probe": "sac_update", "steps": args.steps, "ttis": args.ttis, "reps": args.reps, "alternations": args.alternations, "update": {}, "env": {}}
    for S in (5, 10):
        for minibatch in (256, 4096):
            r = _child(args, "update", None, S, minibatch)
            record["device"] = r.pop("device")
            med = {k: statistics.median(v) for k, v in r["ms_per_step"].items()}
            r.update({"device_ms_per_step": med["device"], "torch_ms_per_step": med["torch"], "torch_over_device": med["torch"] / med["device"]})
            record["update"][f"S{S}_mb{minibatch}"] = r
    for block in ("rollout", "replay"):
        series = {"this": [], "parent_a": [], "parent_b": []}
        for _ in range(args.alternations):
            if args.baseline_lib:
                series["parent_a"] += _child(args, block, args.baseline_lib)["ms"]
            series["this"] += _child(args, block)["ms"]
            if args.baseline_lib:
                series["parent_b"] += _child(args, block, args.baseline_lib)["ms"]
        record["env"][block] = summarise(series, args.reps, bool(args.baseline_lib))
    line = json.dumps(record)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
