"""What the PPO minibatch row lists cost, drawn in torch (adapters.ppo_row_order) and by the library's own kernels
(env.ppo_row_order: ranenv_ppo_row_count + ranenv_ppo_row_order), on one device in one job:

  (a) lists       the row lists alone, both kinds, to the point where they are usable (the torch path's host synchronisation and
                  the device path's one wait for the counts included): the shape of examples/train_ppo_large_batch_on_device.py
                  (B 4096 x 64 TTIs, its S, 4 epochs) and the reference's 2048 rows x 10 epochs (B 64 x 32 TTIs)
  (b) iteration   one iteration of examples/train_ppo_large_batch_on_device.py with and without --device-order, split into collect,
                  row lists, inter update and intra update (the update of both kinds less the update of the inter kind alone)
  (c) unchanged   with --baseline-lib PATH (the parent commit's libranenv_hip.so): rollout(200) at B 4096 and a plain ppo_update
                  with this library and with that one in processes of their own

Medians over alternated blocks of calls behind a warm-up call; every series is kept whole, with its spread (max / min - 1).  The
device path counts as faster only where the gap exceeds both series' spreads ("gap_beyond_spreads").  Writes
profiles/ppo_row_order_probe.json (--out: elsewhere) and prints it as one line.

    python tools/ppo_row_order_probe.py [--parts a,b,c] [--blocks 3] [--baseline-lib parent.so] [--out FILE]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_update_probe as up  # noqa: E402

OUT = os.path.join(REPO, "profiles", "ppo_row_order_probe.json")
NEW_EXPORTS = ("ranenv_ppo_row_count", "ranenv_ppo_row_order")
HP = dict(lr=3e-4, clip=0.2, vf_coeff=0.5, ent_coeff=0.01, grad_clip=0.5)


def _series(ms):
    return {"ms": statistics.median(ms), "all_ms": ms, "spread": max(ms) / min(ms) - 1.0}


def _versus(torch_s, device_s):
    """The two series side by side: the ratio of the medians, and whether the gap exceeds both spreads"""
    ratio = torch_s["ms"] / device_s["ms"]
    gap = abs(torch_s["ms"] - device_s["ms"]) / min(torch_s["ms"], device_s["ms"])
    return {"torch": torch_s, "device": device_s, "torch_over_device": ratio, "gap_beyond_spreads": gap > max(torch_s["spread"], device_s["spread"])}


def _large_batch_env(torch, B, slabs=64, spread=True):
    """The handle of examples/train_ppo_large_batch_on_device.py: its workload, nets, seeds and binding"""
    import numpy as np
    from intent_radio_sched_multi_slice_amd._lib import INTRA_PF, POLICY_MAPF
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    L, n_ep = 100, 64
    env = make_mult_slice_workload(B, torch.device("cuda", 0), policy=POLICY_MAPF, intra=INTRA_PF, n_scenarios=n_ep, n_traces=n_ep, trace_len=L,
                                   max_steps=L).env
    S, W = env.S, env.W
    env.set_se_mode("gather")
    ep = np.arange(n_ep)
    env.set_episode_table(scenario=ep, se_base=ep * L, se_len=L, trf_base=ep * L, trf_len=L)
    env.enable_autoreset(0, n_ep, random_episodes=True, seed=7, episode_numbers=np.arange(B) % n_ep)
    torch.manual_seed(0)
    mlp = lambda i, o: up._mlp(torch, [i, 64, 64, o])      # noqa: E731
    pi_inter, vf_inter, pi_intra, vf_intra = mlp(10 * S, 2 * S), mlp(10 * S, 1), mlp(W, 3), mlp(W, 1)
    env.set_policy_network(pi_inter, pi_intra, stochastic=True, seed=1000)
    env.set_value_network(vf_inter, vf_intra)
    env.ppo_bind(spread=True, slabs=slabs) if spread else env.ppo_bind()
    env.reset()
    return env


def _timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def measure_lists(blocks, calls=5):
    import torch
    from intent_radio_sched_multi_slice_amd.adapters import ppo_row_order
    out = {}
    for key, B, T, epochs, spread in (("large_batch_B4096_T64_e4", 4096, 64, 4, True), ("reference_B64_T32_e10", 64, 32, 10, False)):
        env = _large_batch_env(torch, B, spread=spread)
        rec = env.collect(T)
        paths = {"torch": lambda s: ppo_row_order(rec, [0, B], epochs, s), "device": lambda s: env.ppo_row_order(rec, epochs, s)}
        ms = {k: [] for k in paths}
        for name, fn in paths.items():
            lists, _ = _timed(torch, lambda: fn(0))                          # (warm-up: kernels loaded, buffers allocated)
        for blk in range(blocks):
            for name, fn in paths.items():
                for c in range(calls):
                    lists, t = _timed(torch, lambda: fn(1 + blk * calls + c))
                    ms[name].append(t)
        out[key] = _versus(_series(ms["torch"]), _series(ms["device"]))
        out[key].update(S=env.S, rows_inter=B * T, rows_intra=int(lists["first_intra"][-1]), epochs=epochs)
        print("lists", key, json.dumps(out[key]), flush=True)
        env.close()
    return out


def measure_iteration(blocks, iters=2, B=4096, T=64, epochs=4, minibatch=65536):
    import torch
    from intent_radio_sched_multi_slice_amd.adapters import ppo_row_order
    env = _large_batch_env(torch, B)
    draw = {"torch": lambda rec, s: ppo_row_order(rec, [0, B], epochs, s), "device": lambda rec, s: env.ppo_row_order(rec, epochs, s)}
    parts = {name: {"collect": [], "lists": [], "update": [], "update_inter_only": []} for name in draw}

    def iteration(name, seed, keep):
        rec, t_collect = _timed(torch, lambda: env.collect(T, gamma=0.99, lam=0.95))
        order, t_lists = _timed(torch, lambda: draw[name](rec, seed))
        _, t_both = _timed(torch, lambda: env.ppo_update(rec, epochs=epochs, minibatch=minibatch, order=order, **HP))
        inter = {"order_inter": order["order_inter"], "first_inter": order["first_inter"]}
        _, t_inter = _timed(torch, lambda: env.ppo_update(rec, epochs=epochs, minibatch=minibatch, order=inter, **HP))
        if keep:
            for k, t in (("collect", t_collect), ("lists", t_lists), ("update", t_both), ("update_inter_only", t_inter)):
                parts[name][k].append(t)

    for name in draw:
        iteration(name, 0, False)
    seed = 1
    for _ in range(blocks):
        for name in draw:
            for _ in range(iters):
                iteration(name, seed, True)
                seed += 1
    out = {"B": B, "T": T, "epochs": epochs, "minibatch": minibatch, "slabs": 64}
    for name, p in parts.items():
        s = {k: _series(v) for k, v in p.items()}
        s["update_intra_ms"] = s["update"]["ms"] - s["update_inter_only"]["ms"]
        s["iteration_ms"] = s["collect"]["ms"] + s["lists"]["ms"] + s["update"]["ms"]
        s["lists_share"] = s["lists"]["ms"] / s["iteration_ms"]
        out[name] = s
    out["lists"] = _versus(out["torch"]["lists"], out["device"]["lists"])
    out["iteration_torch_over_device"] = out["torch"]["iteration_ms"] / out["device"]["iteration_ms"]
    print("iteration", json.dumps(out), flush=True)
    env.close()
    return out


def _child(lib):
    env = dict(os.environ)
    if lib:
        env["RANENV_LIB"] = os.path.abspath(lib)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=600)
    return json.loads(res.stdout.strip().split("\n")[-1])


def _child_unchanged():
    import torch
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.adapters import ppo_row_order
    lib = __import__("ctypes").CDLL(_lib.LIB_PATH)
    for n in NEW_EXPORTS:                             # (the parent's library has not the new exports and runs both)
        if not hasattr(lib, n):
            _lib.FUNCTIONS.pop(n, None)
    _lib.EXPORTS = tuple(_lib.FUNCTIONS)
    rollout = up.measure_rollout()
    B = up.ROWS // up.T
    env = up._workload(torch, B)
    S = env.S
    torch.manual_seed(B)
    env.set_policy_network(up._mlp(torch, [10 * S, 64, 64, 2 * S]).cuda(), None, stochastic=True, seed=3)
    env.set_value_network(up._mlp(torch, [10 * S, 64, 64, 1]).cuda(), None)
    env.ppo_bind()
    env.reset()
    rec = env.collect(up.T)
    order = ppo_row_order(rec, [0, B], up.EPOCHS, seed=1, intra=False)
    ms = []
    for _ in range(6):
        _, t = _timed(torch, lambda: env.ppo_update(rec, epochs=up.EPOCHS, minibatch=up.MINIBATCH, order=order, **up.HP))
        ms.append(t)
    print(json.dumps({"rollout_ms": rollout, "update_ms": statistics.median(ms[1:])}))


def measure_unchanged(baseline, alternations):
    base, new = [], []
    for _ in range(alternations):
        base.append(_child(baseline))
        new.append(_child(None))
    out = {}
    for k in ("rollout_ms", "update_ms"):
        b, n = [x[k] for x in base], [x[k] for x in new]
        ratio, spread = statistics.median(n) / statistics.median(b), max(max(b) / min(b), max(n) / min(n)) - 1.0
        out[k] = {"baseline": b, "this": n, "ratio": ratio, "spread": spread, "within_spread": abs(ratio - 1.0) <= spread}
    print("unchanged", json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        _child_unchanged()
        return
    parts = set(args.parts.split(","))
    result = {}
    if os.path.exists(args.out):                     # (parts measured in an earlier job of the same series stay)
        with open(args.out) as f:
            result.update(json.load(f))
    if "c" in parts and args.baseline_lib:
        result["unchanged"] = measure_unchanged(args.baseline_lib, args.alternations)
    if "a" in parts:
        result["lists"] = measure_lists(args.blocks)
    if "b" in parts:
        result["iteration"] = measure_iteration(args.blocks)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
