"""What training the single SB3 PPO head agent costs under the spread head binding (ppo_bind(head=True, spread=True)), SB3's [64, 64] tanh
pair at S 5 (U 25) and S 10 (U 100), one job:

  (a) collected    the batch collect_head() leaves the agent -- 262 144 rows (B 4096 x 64 TTIs), 4 epochs, minibatch 8192 and 65 536 --
                   under 64 and 256 slabs, against the plain head binding (force=True) on a twin handle and against the eager-torch
                   loop of tools/ppo_head_probe.py (the example's) over the same chunks
  (b) reference    SB3's own regime: 2048 rows, 10 epochs, minibatch 64, the same four series
  (c) unchanged    with --baseline-lib PATH (the parent commit's libranenv_hip.so): rollout(200) and collect_head(200) at B 4096 / S 5
                   and a plain ppo_update_head at SB3's regime, with this library and with that one in processes of their own

Device timings are medians over alternated blocks of calls behind a warm-up call; every series is kept whole, with its spread
(max / min - 1).  Writes profiles/ppo_head_spread_probe.json (--out: elsewhere) and prints it as one line.

    python tools/ppo_head_spread_probe.py [--parts a,b,c] [--blocks 3] [--baseline-lib parent.so] [--out FILE]
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppo_head_probe as hp  # noqa: E402

OUT = os.path.join(REPO, "profiles", "ppo_head_spread_probe.json")
NEW_EXPORTS = ("ranenv_ppo_bind_head_spread", "ranenv_ppo_head_spread_bytes")
BINDS = {"spread_64": dict(spread=True, slabs=64), "spread_256": dict(spread=True, slabs=256), "plain": dict()}


def _calls(torch, env, rec, order, n, epochs, minibatch):
    ms = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env.ppo_update_head(rec, epochs=epochs, minibatch=minibatch, order=order, force=True, **hp.HP)      # (returns behind a device read-back)
        ms.append(1e3 * (time.perf_counter() - t0))
    return ms


def _series(ms):
    return {"ms": statistics.median(ms), "all_ms": ms, "spread": max(ms) / min(ms) - 1.0}


def _torch_ms(torch, rec, order, nets, S, epochs, minibatch):
    saved = hp.EPOCHS, hp.MINIBATCH
    hp.EPOCHS, hp.MINIBATCH = epochs, minibatch
    torch.distributions.Distribution.set_default_validate_args(False)      # (timed, not judged)
    try:
        actor, critic, log_std = copy.deepcopy(nets)
        return hp.torch_loop(torch, rec, order, actor, critic, log_std, S)
    finally:
        hp.EPOCHS, hp.MINIBATCH = saved


def compare(torch, S, B, T, epochs, minibatch, blocks, calls, plain_calls):
    """{name: series} of BINDS on twin handles (the same nets by the same seed), blocks alternated, and the eager loop"""
    from intent_radio_sched_multi_slice_amd.adapters import ppo_head_row_order
    handles = {}
    for name, bind in BINDS.items():
        env, *nets = hp._head_env(torch, B, S)
        env.ppo_bind(head=True, **bind)
        rec = env.collect_head(T)
        handles[name] = (env, rec, ppo_head_row_order(rec, epochs, seed=1), nets)
        _calls(torch, *handles[name][:3], 1, epochs, minibatch)             # (warm-up: the first call also loads the kernels)
    ms = {name: [] for name in BINDS}
    for _ in range(blocks):
        for name in BINDS:
            ms[name] += _calls(torch, *handles[name][:3], plain_calls if name == "plain" else calls, epochs, minibatch)
    env, rec, order, nets = handles["plain"]
    out = {name: _series(x) for name, x in ms.items()}
    out["torch"] = _series([_torch_ms(torch, rec, order, nets, S, epochs, minibatch) for _ in range(3)][1:])      # (the first run warms torch up)
    out["rows"], out["optimiser_steps"] = B * T, epochs * -(-B * T // minibatch)
    for name in ("plain", "torch"):
        out[name + "_over_spread_64"] = out[name]["ms"] / out["spread_64"]["ms"]
        out[name + "_over_spread_256"] = out[name]["ms"] / out["spread_256"]["ms"]
    for env, _, _, _ in handles.values():
        env.close()
    return out


def measure(part, blocks):
    import torch
    out = {}
    for S in (5, 10):
        for minibatch in ((8192, 65536) if part == "collected" else (hp.MINIBATCH,)):
            key = f"S{S}_mb{minibatch}"
            if part == "collected":
                out[key] = compare(torch, S, 4096, 64, 4, minibatch, blocks, 3, 1)
            else:
                out[key] = compare(torch, S, hp.ROWS // hp.T, hp.T, hp.EPOCHS, minibatch, blocks, 3, 3)
            print(part, key, json.dumps(out[key]), flush=True)
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
    from intent_radio_sched_multi_slice_amd.adapters import ppo_head_row_order
    lib = __import__("ctypes").CDLL(_lib.LIB_PATH)
    for n in NEW_EXPORTS:                             # (the parent's library has not the new exports and runs all three)
        if not hasattr(lib, n):
            _lib.FUNCTIONS.pop(n, None)
    _lib.EXPORTS = tuple(_lib.FUNCTIONS)
    res = hp.measure_unchanged()
    env, *_ = hp._head_env(torch, hp.ROWS // hp.T, 5)
    env.ppo_bind(head=True)
    rec = env.collect_head(hp.T)
    order = ppo_head_row_order(rec, hp.EPOCHS, seed=1)
    res["update_head_ms"] = statistics.median(_calls(torch, env, rec, order, 6, hp.EPOCHS, hp.MINIBATCH)[1:])
    print(json.dumps(res))


def measure_unchanged(baseline, alternations):
    base, new = [], []
    for _ in range(alternations):
        base.append(_child(baseline))
        new.append(_child(None))
    out = {}
    for k in ("rollout_ms", "collect_head_ms", "update_head_ms"):
        b, n = [x[k] for x in base], [x[k] for x in new]
        ratio, spread = statistics.median(n) / statistics.median(b), max(b) / min(b) - 1.0
        out[k] = {"baseline": b, "this": n, "ratio": ratio, "baseline_spread": spread, "within_spread": abs(ratio - 1.0) <= spread}
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
    result = {"nets": "[64, 64] tanh", "hp": hp.HP}
    if os.path.exists(args.out):                     # (parts measured in an earlier job of the same series stay)
        with open(args.out) as f:
            result.update(json.load(f))
    if "c" in parts and args.baseline_lib:
        result["unchanged"] = measure_unchanged(args.baseline_lib, args.alternations)
    if "b" in parts:
        result["reference"] = measure("reference", args.blocks)
    if "a" in parts:
        result["collected"] = measure("collected", args.blocks)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
