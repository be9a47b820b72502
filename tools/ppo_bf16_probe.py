"""What training ONE agent's bf16 nets costs under ppo_bind(spread=True, bf16=True) against the f32 spread binding, S 5 / U 25, inter nets
only, one job:

  (a) collected    262 144 inter rows (B 4096 x 64 TTIs), 4 epochs, minibatch 8192 and 65 536, [64, 64], [256, 256] and [512] x 3 nets:
                   the bf16 binding against the f32 spread binding (``wide`` for [512] x 3) at equal slabs, 64 and 256, twin handles
                   from the same initial weights, with the eager-torch loop of tools/ppo_update_probe.py over the same chunks beside them
  (b) reference    the reference's settings, 2048 rows x 10 epochs at minibatch 64 and 16, the same nets and bindings
  (c) iteration    collect(200) at B 4096 with f32 and with bf16 nets ([512] x 3 actors and critics), alternated: with (a) one full
                   iteration, collect + update, both ways
  (d) unchanged    with --baseline-lib PATH (the parent commit's libranenv_hip.so): tools/ppo_spread_probe.py's part (c) -- rollout(200)
                   and an f32 ppo_update with this library and with that one in processes of their own

Device timings are medians over alternated blocks of calls behind a warm-up call; every series is kept whole, with its spread
(max / min - 1).  Writes profiles/ppo_bf16_probe.json (--out: elsewhere) and prints it as one line.

    python tools/ppo_bf16_probe.py [--parts a,b,c,d] [--blocks 3] [--baseline-lib parent.so] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_spread_probe as sp  # noqa: E402
import ppo_update_probe as up  # noqa: E402
import ppo_wide_probe as wp  # noqa: E402

OUT = os.path.join(REPO, "profiles", "ppo_bf16_probe.json")
NETS = ([64, 64], [256, 256], wp.VERYBIG)


def _agent(torch, B, T, widths, epochs, nets, precision, **bind):
    """tools/ppo_spread_probe.py's handle with the inter pair bound in ``precision``"""
    from intent_radio_sched_multi_slice_amd.adapters import ppo_row_order
    env = up._workload(torch, B)
    env.set_policy_network(nets[0], None, stochastic=True, seed=3, precision=precision)
    env.set_value_network(nets[1], None, precision=precision)
    env.ppo_bind(**bind)
    env.reset()
    rec = env.collect(T)
    return env, rec, ppo_row_order(rec, [0, B], epochs, seed=1, intra=False)


def compare(torch, B, T, widths, epochs, minibatch, blocks, calls=3):
    S = 5
    torch.manual_seed(B + len(widths))
    nets = (up._mlp(torch, [10 * S] + widths + [2 * S]).cuda(), up._mlp(torch, [10 * S] + widths + [1]).cuda())
    wide = widths == wp.VERYBIG
    handles = {}
    for slabs in (64, 256):
        handles[f"f32_{slabs}"] = _agent(torch, B, T, widths, epochs, nets, "f32", spread=True, slabs=slabs, wide=wide)
        handles[f"bf16_{slabs}"] = _agent(torch, B, T, widths, epochs, nets, "bf16", spread=True, slabs=slabs, bf16=True)
    for h in handles.values():
        sp._calls(torch, *h, 1, epochs, minibatch)                          # (warm-up: the first call also loads the kernels)
    ms = {name: [] for name in handles}
    for _ in range(blocks):
        for name, h in handles.items():
            ms[name] += sp._calls(torch, *h, calls, epochs, minibatch)
    out = {name: sp._series(x) for name, x in ms.items()}
    env, rec, order = handles["f32_64"]
    out["torch"] = sp._series([sp._torch_ms(torch, rec, order, nets, env.S, epochs, minibatch) for _ in range(2)])
    out["rows"], out["optimiser_steps"] = B * T, epochs * -(-B * T // minibatch)
    for slabs in (64, 256):
        out[f"f32_over_bf16_{slabs}"] = out[f"f32_{slabs}"]["ms"] / out[f"bf16_{slabs}"]["ms"]
    out["torch_over_bf16_64"] = out["torch"]["ms"] / out["bf16_64"]["ms"]
    for h in handles.values():
        h[0].close()
    return out


def measure(part, blocks, nets=NETS):
    import torch
    out = {}
    for widths in nets:
        for minibatch in ((8192, 65536) if part == "collected" else (64, 16)):
            key = "x".join(map(str, widths)) + f"_mb{minibatch}"
            if part == "collected":
                out[key] = compare(torch, 4096, 64, widths, 4, minibatch, blocks)
            else:
                out[key] = compare(torch, up.ROWS // up.T, up.T, widths, up.EPOCHS, minibatch, blocks)
            print(part, key, json.dumps(out[key]), flush=True)
    return out


def measure_collect(blocks, T=200, B=4096):
    import torch
    S = 5
    torch.manual_seed(1)
    nets = (up._mlp(torch, [10 * S] + wp.VERYBIG + [2 * S]).cuda(), up._mlp(torch, [10 * S] + wp.VERYBIG + [1]).cuda())
    envs = {}
    for precision in ("f32", "bf16"):
        env = up._workload(torch, B)
        env.set_policy_network(nets[0], None, stochastic=True, seed=3, precision=precision)
        env.set_value_network(nets[1], None, precision=precision)
        env.reset()
        env.collect(T)
        envs[precision] = env
    ms = {p: [] for p in envs}
    for _ in range(blocks):
        for p, env in envs.items():
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                env.collect(T)
                torch.cuda.synchronize()
                ms[p].append(1e3 * (time.perf_counter() - t0))
    out = {p: sp._series(x) for p, x in ms.items()}
    out["f32_over_bf16"] = out["f32"]["ms"] / out["bf16"]["ms"]
    out["ttis"], out["batch"] = T, B
    for env in envs.values():
        env.close()
    print("iteration", json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b,c,d")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    parts = set(args.parts.split(","))
    result = {"size": "S5_U25", "hp": up.HP}
    if os.path.exists(args.out):                     # (parts measured in an earlier job of the same series stay)
        with open(args.out) as f:
            result.update(json.load(f))
    if "d" in parts and args.baseline_lib:
        result["unchanged"] = sp.measure_unchanged(args.baseline_lib, args.alternations)
    if "a" in parts:
        result["collected"] = measure("collected", args.blocks)
    if "b" in parts:
        result["reference"] = measure("reference", args.blocks)
    if "c" in parts:
        result["collect_200"] = measure_collect(args.blocks)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
