"""What off-policy (SAC) collection costs on the device, at the two sizes of the DESIGN 4.p table, under a [256, 256] relu SAC actor
("gauss_tanh") and, for the targets, two [256, 256] relu critics.

Writes one JSON record to profiles/sac_probe.json (and prints it):
  (a) per size, ALTERNATING in child processes of their own (--alternations times each): rollout(K) with the parent commit's library
      (--baseline-lib), rollout(K) with this build, collect_replay(K) with this build (ring capacity K).  `rollout_untaxed` holds every
      figure, the time per TTI of both libraries, the baseline's own run-to-run spread and whether this build's best time lies within it:
      the existing rollout must not have slowed down.  `collect_replay` holds its figures and the extra time per TTI over rollout.
  (b) replay_sample(n) + sac_targets(n) for n = 65 536 on a full ring against the same work in eager torch on the same GPU: an index
      draw (torch.randint), five gathers from the ring, the actor's forward, the squashed-Gaussian epilogue with torch.randn noise, the two
      critics' forwards and the target (the arithmetic of adapters.sac_targets_torch with the host-side Philox noise left out of the clock).

    python tools/sac_probe.py [--steps 200] [--reps 3] [--baseline-lib parent.so] [--alternations 3]
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
WIDTHS, ACT = [256, 256], "relu"
N_SAMPLE = 65536
OUT = os.path.join(REPO, "profiles", "sac_probe.json")


def _mlp(torch, dims, seed):
    torch.manual_seed(seed)
    mods = []
    for i in range(len(dims) - 1):
        mods.append(torch.nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            mods.append(torch.nn.ReLU())
    return torch.nn.Sequential(*mods)


def _time(torch, fn, reps):
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


def _env(torch, _lib, kw):
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    wl = make_mult_slice_workload(device=torch.device("cuda", 0), policy=_lib.POLICY_MAPF, intra=_lib.INTRA_RR, n_scenarios=64, n_traces=64,
                                  trace_len=256, max_steps=100000, **kw)
    env = wl.env
    env.enable_heads()
    actor = _mlp(torch, [10 * env.S] + WIDTHS + [2 * env.S], 2).to(env.device)
    env.set_head_policy_network(actor, "gauss_tanh", stochastic=True, seed=1, allow_sorted=True)
    return wl, env, actor


def measure_rollout(steps, reps):
    """rollout(K) under the SAC actor: a path the parent commit's library has too (RANENV_LIB selects the library)."""
    import ctypes
    import torch
    from intent_radio_sched_multi_slice_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.FUNCTIONS if not hasattr(raw, n)]:
        _lib.FUNCTIONS.pop(name)
    out = {}
    for size, kw in SIZES.items():
        wl, env, _ = _env(torch, _lib, kw)
        env.reset()
        env.rollout(8)
        torch.cuda.synchronize()
        out[size] = _time(torch, lambda: env.rollout(steps), reps)
        env.close()
        del wl, env
        torch.cuda.empty_cache()
    return out


def measure_collect(steps, reps):
    import torch
    from intent_radio_sched_multi_slice_amd import _lib
    out = {}
    for size, kw in SIZES.items():
        wl, env, _ = _env(torch, _lib, kw)
        env.bind_replay(steps)
        env.reset()
        env.collect_replay(8)
        torch.cuda.synchronize()
        out[size] = _time(torch, lambda: env.collect_replay(steps), reps)
        env.close()
        del wl, env
        torch.cuda.empty_cache()
    return out


def measure_targets(reps):
    import math
    import torch
    from intent_radio_sched_multi_slice_amd import _lib
    out = {}
    n = N_SAMPLE
    for size, kw in SIZES.items():
        wl, env, actor = _env(torch, _lib, kw)
        S, B, dev = env.S, env.B, env.device
        cap = 16
        ring = env.bind_replay(cap)
        env.reset()
        env.collect_replay(cap)
        q1, q2 = _mlp(torch, [11 * S] + WIDTHS + [1], 3).to(dev), _mlp(torch, [11 * S] + WIDTHS + [1], 4).to(dev)
        env.set_sac_critics(q1, q2)
        flat = {k: t.reshape((cap * B,) + t.shape[2:]) for k, t in ring.items()}

        def device(draw=[0]):
            draw[0] += 1
            mb = env.replay_sample(n, seed=3, draw=draw[0], reward="colran")
            return env.sac_targets(mb["next_obs"], mb["reward"], mb["done"], gamma=0.99, ent_coef=0.2, stochastic=True, seed=5, draw=draw[0],
                                   outputs=("target",))["target"]

        def eager():
            with torch.no_grad():
                ix = torch.randint(0, cap * B, (n,), device=dev)
                obs, nxt, done = flat["obs"][ix], flat["next_obs"][ix], flat["done"][ix]
                act, rew = flat["action"][ix].to(torch.float32), flat["reward_head"][ix, 1].to(torch.float32)
                o = actor(nxt).to(torch.float64)
                mu, ls = o[:, :S], o[:, S:].clamp(-20.0, 2.0)
                z = torch.randn((n, S), dtype=torch.float64, device=dev)
                a = torch.tanh(mu + torch.exp(ls) * z)
                logp = (((-0.5 * z) * z - ls) - 0.5 * math.log(2.0 * math.pi) - torch.log((1.0 - a * a) + 1e-6)).sum(-1)
                xa = torch.cat([nxt, a.to(torch.float32)], dim=1)
                qmin = torch.minimum(q1(xa)[:, 0], q2(xa)[:, 0]).to(torch.float64)
                nd = (done == 0).to(torch.float64)
                return obs, act, (rew.to(torch.float64) + nd * (0.99 * (qmin - 0.2 * logp))).to(torch.float32)

        device()
        eager()
        torch.cuda.synchronize()
        c = {"n": n, "device_ms": _time(torch, device, reps), "eager_torch_ms": _time(torch, eager, reps)}
        c["eager_over_device"] = c["eager_torch_ms"] / c["device_ms"]
        out[size] = c
        env.close()
        del wl, env
        torch.cuda.empty_cache()
    out["device"] = torch.cuda.get_device_name(0)
    return out


def _child(what, steps, reps, lib=None):
    env = dict(os.environ)
    if lib:
        env["RANENV_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--steps", str(steps), "--reps", str(reps)]
    res = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=500)
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--child", choices=("rollout", "collect", "targets"), default=None)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.child:
        fn = {"rollout": lambda: measure_rollout(args.steps, args.reps), "collect": lambda: measure_collect(args.steps, args.reps),
              "targets": lambda: measure_targets(args.reps)}[args.child]
        print(json.dumps(fn()))
        return
    # every measurement in a process of its own: the parent of them all never opens the GPU
    base, new, coll = [], [], []
    for _ in range(args.alternations):
        if args.baseline_lib:
            base.append(_child("rollout", args.steps, args.reps, args.baseline_lib))
        new.append(_child("rollout", args.steps, args.reps))
        coll.append(_child("collect", args.steps, args.reps))
    targets = _child("targets", args.steps, args.reps)
    record = {"probe": "sac", "steps": args.steps, "reps": args.reps, "alternations": args.alternations, "device": targets.pop("device"),
              "actor": "256x256 relu gauss_tanh", "rollout_untaxed": {}, "collect_replay": {}, "sample_and_targets": targets}
    for size in SIZES:
        n, c = [r[size] for r in new], [r[size] for r in coll]
        record["collect_replay"][size] = {"collect_replay_ms": c, "rollout_ms": n, "extra_us_per_tti": (min(c) - min(n)) * 1e3 / args.steps,
                                          "collect_over_rollout": min(c) / min(n),
                                          "env_steps_per_s": SIZES[size]["batch"] * args.steps / (min(c) * 1e-3)}
        if base:
            b = [r[size] for r in base]
            u = {"baseline_ms": b, "this_ms": n, "baseline_us_per_tti": min(b) * 1e3 / args.steps, "this_us_per_tti": min(n) * 1e3 / args.steps,
                 "baseline_spread": max(b) / min(b) - 1.0, "this_spread": max(n) / min(n) - 1.0, "this_over_baseline": min(n) / min(b)}
            u["within_baseline_spread"] = u["this_over_baseline"] <= 1.0 + u["baseline_spread"]
            record["rollout_untaxed"][size] = u
    line = json.dumps(record)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
