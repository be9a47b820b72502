"""What the device PPO update of the head policies costs: `ppo_update_head` against the eager-torch SGD loop on the same chunks, at SB3's
regime -- 2048 rows, minibatch 64, 10 epochs, a [64, 64] tanh actor / critic pair -- at S 5 (U 25) and S 10 (U 100); and what it must NOT
change: `rollout(200)` and `collect_head(200)` under a head policy with this library and with the parent commit's.

Writes profiles/ppo_head_probe.json (and prints it as one line), one MI355X, one job:
  update[S]: device_ms / torch_ms -- medians of --blocks blocks, the two sides alternated block by block -- and their ratio
  unchanged: with --baseline-lib PATH (the parent commit's libranenv_hip.so): rollout_ms and collect_head_ms at B 4096 / S 5 with either
             library, each measurement a child process of its own, alternated; ratio of the medians and the parent's own spread

    python tools/ppo_head_probe.py [--blocks 5] [--baseline-lib parent.so] [--alternations 4]
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
OUT = os.path.join(REPO, "profiles", "ppo_head_probe.json")
NEW_EXPORTS = ("ranenv_ppo_bind_head", "ranenv_ppo_update_head", "ranenv_ppo_head_layout", "ranenv_ppo_head_state", "ranenv_get_head_net_weights",
               "ranenv_get_head_log_std")
ROWS, MINIBATCH, EPOCHS, T = 2048, 64, 10, 32
HP = dict(lr=3e-4, clip=0.2, vf_coeff=0.5, ent_coeff=0.0, grad_clip=0.5, eps=1e-5)
SIZES = {5: dict(n_slices=5, n_ues=25, n_rbs=135, rbs_per_rbg=5, max_ues_slice=10), 10: dict(n_slices=10, n_ues=100, n_rbs=135, rbs_per_rbg=1, max_ues_slice=10)}


def _mlp(torch, dims):
    mods = []
    for i in range(len(dims) - 1):
        mods.append(torch.nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods)


def _head_env(torch, B, S):
    """A reset env under a stochastic [64, 64] tanh head policy with its critic; returns (env, actor, critic, log_std)"""
    import numpy as np
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    wl = make_mult_slice_workload(B, torch.device("cuda", 0), policy=_lib.POLICY_MAPF, intra=_lib.INTRA_RR, n_scenarios=8, n_traces=8,
                                  trace_len=64, max_steps=1000, **SIZES[S])
    env = wl.env
    wl.tables.sorted_slices[...] = np.arange(env.S, dtype=np.int32)
    env.load_scenarios(wl.tables)
    env.enable_heads(((1 + np.arange(S) % 2)[None, :] * (wl.tables.slice_has_req != 0)).astype(np.int32))
    torch.manual_seed(S)
    actor, critic, log_std = _mlp(torch, [10 * S, 64, 64, S]).cuda(), _mlp(torch, [10 * S, 64, 64, 1]).cuda(), torch.zeros(S, device="cuda")
    env.set_head_policy_network(actor, "gauss_clip", log_std, stochastic=True, seed=3)
    env.set_head_value_network(critic)
    env.reset()
    return env, actor, critic, log_std


def torch_loop(torch, rec, order, actor, critic, log_std, S):
    """SB3's PPO.train in eager torch on the same chunks; returns milliseconds"""
    N = rec["logp"].numel()
    obs, act = rec["obs_head"].reshape(N, 10 * S), rec["action"].reshape(N, S).to(torch.float32)
    logp0, adv0, vt0 = rec["logp"].reshape(N), rec["adv"].reshape(N), rec["vtarg"].reshape(N)
    ls = torch.nn.Parameter(log_std.clone())
    params = list(actor.parameters()) + list(critic.parameters()) + [ls]
    opt = torch.optim.Adam(params, lr=HP["lr"], eps=HP["eps"])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for ep in range(EPOCHS):
        for c0 in range(0, N, MINIBATCH):
            idx = order[ep, c0:c0 + MINIBATCH].long()
            dist = torch.distributions.Normal(actor(obs[idx]), torch.exp(ls))
            logp, ent = dist.log_prob(act[idx]).sum(-1), dist.entropy().sum(-1)
            adv = adv0[idx]
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
            ratio = torch.exp(logp - logp0[idx])
            surr = torch.minimum(ratio * adv, ratio.clamp(1.0 - HP["clip"], 1.0 + HP["clip"]) * adv)
            loss = -surr.mean() + HP["vf_coeff"] * (critic(obs[idx])[:, 0] - vt0[idx]).pow(2).mean() - HP["ent_coeff"] * ent.mean()
            opt.zero_grad(set_to_none=True)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(params, HP["grad_clip"])
            opt.step()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def measure_update(blocks):
    import torch
    from intent_radio_sched_multi_slice_amd.adapters import ppo_head_row_order
    out = {}
    for S in (5, 10):
        env, actor, critic, log_std = _head_env(torch, ROWS // T, S)
        env.ppo_bind(head=True)
        rec = env.collect_head(T)
        order = ppo_head_row_order(rec, EPOCHS, seed=1)
        dev, eager = [], []
        for b in range(blocks + 1):                   # (block 0 loads the kernel and warms torch up: dropped)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = env.ppo_update_head(rec, epochs=EPOCHS, minibatch=MINIBATCH, order=order, **HP)
            dev.append(1e3 * (time.perf_counter() - t0))
            eager.append(torch_loop(torch, rec, order, actor, critic, log_std, S))
        lay = env.ppo_head_layout()
        out[str(S)] = {"device_ms": statistics.median(dev[1:]), "torch_ms": statistics.median(eager[1:]), "device_all_ms": dev, "torch_all_ms": eager,
                       "speedup": statistics.median(eager[1:]) / statistics.median(dev[1:]), "rows": ROWS, "optimiser_steps": int(st["minibatches"].sum()),
                       "lds_bytes": lay["lds_bytes"], "parameters_packed": lay["actor"] + lay["critic"] + S}
        print(S, out[str(S)], flush=True)
        env.close()
    return out


def measure_unchanged(steps=200, blocks=5):
    import torch
    from intent_radio_sched_multi_slice_amd import _lib
    lib = __import__("ctypes").CDLL(_lib.LIB_PATH)
    for n in NEW_EXPORTS:                             # (a library without the new exports can run it)
        if not hasattr(lib, n):
            _lib.FUNCTIONS.pop(n, None)
    env, *_ = _head_env(torch, 4096, 5)
    res = {}
    for name, call in (("rollout_ms", lambda: env.rollout(steps)), ("collect_head_ms", lambda: env.collect_head(steps))):
        call()
        ms = []
        for _ in range(blocks):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        res[name] = statistics.median(ms)
    return res


def _child(lib):
    env = dict(os.environ)
    if lib:
        env["RANENV_LIB"] = os.path.abspath(lib)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, check=True, capture_output=True, text=True, timeout=600)
    return json.loads(res.stdout.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--alternations", type=int, default=4)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure_unchanged()))
        return
    result = {"regime": {"rows": ROWS, "minibatch": MINIBATCH, "epochs": EPOCHS, "nets": "[64, 64] tanh", **HP}}
    if args.baseline_lib:
        base, new = [], []
        for _ in range(args.alternations):
            base.append(_child(args.baseline_lib))
            new.append(_child(None))
        result["unchanged"] = {}
        for k in ("rollout_ms", "collect_head_ms"):
            b, n = [x[k] for x in base], [x[k] for x in new]
            result["unchanged"][k] = {"baseline_ms": b, "this_ms": n, "ratio": statistics.median(n) / statistics.median(b), "baseline_spread": max(b) / min(b) - 1.0}
    result["update"] = measure_update(args.blocks)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
