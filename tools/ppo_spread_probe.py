"""What training ONE agent costs under the spread binding (ppo_bind(spread=True)), S 5 / U 25, inter nets only, one job:

  (a) collected    the batch collect() leaves one agent -- 262 144 inter rows (B 4096 x 64 TTIs), 4 epochs, minibatch 8192 and 65 536,
                   [64, 64] and [256, 256] nets -- under 64 and 256 slabs, against the plain binding (force=True) on a twin handle and
                   against the eager-torch loop of tools/ppo_update_probe.py over the same chunks
  (b) reference    the reference's settings: 2048 rows, 10 epochs, minibatch 64 with [64, 64] and [256, 256]; minibatch 16 and 64 with
                   [512] x 3 under the wide plan on both sides
  (c) unchanged    with --baseline-lib PATH (the parent commit's libranenv_hip.so): rollout(200) at B 4096 and a plain ppo_update (G 1,
                   [64, 64], the regime of tools/ppo_update_probe.py) with this library and with that one in processes of their own

Device timings are medians over alternated blocks of calls behind a warm-up call; every series is kept whole, with its spread
(max / min - 1).  Writes profiles/ppo_spread_probe.json (--out: elsewhere) and prints it as one line.

    python tools/ppo_spread_probe.py [--parts a,b,c] [--blocks 3] [--baseline-lib parent.so] [--out FILE]
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
import ppo_wide_probe as wp  # noqa: E402

OUT = os.path.join(REPO, "profiles", "ppo_spread_probe.json")
NEW_EXPORTS = ("ranenv_ppo_bind_spread", "ranenv_ppo_spread_bytes", "ranenv_ppo_spread_plan",
               "ranenv_ppo_bind_spread_bfloat", "ranenv_ppo_spread_bfloat_bytes")      # (... and tools/ppo_bf16_probe.py's, which runs part (c) against its parent)


def _agent(torch, B, T, widths, epochs, nets=None, **bind):
    """A reset env of B envs under ONE agent's inter pair, bound as ``bind`` says, with its record of T TTIs and its row lists"""
    from intent_radio_sched_multi_slice_amd.adapters import ppo_row_order
    env = up._workload(torch, B)
    S = env.S
    if nets is None:
        torch.manual_seed(B + len(widths))
        nets = (up._mlp(torch, [10 * S] + widths + [2 * S]).cuda(), up._mlp(torch, [10 * S] + widths + [1]).cuda())
    env.set_policy_network(nets[0], None, stochastic=True, seed=3)
    env.set_value_network(nets[1], None)
    env.ppo_bind(**bind)
    env.reset()
    rec = env.collect(T)
    return env, rec, ppo_row_order(rec, [0, B], epochs, seed=1, intra=False), nets


def _calls(torch, env, rec, order, n, epochs, minibatch):
    ms = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env.ppo_update(rec, epochs=epochs, minibatch=minibatch, order=order, force=True, **up.HP)      # (returns behind a device read-back)
        ms.append(1e3 * (time.perf_counter() - t0))
    return ms


def _series(ms):
    return {"ms": statistics.median(ms), "all_ms": ms, "spread": max(ms) / min(ms) - 1.0}


def _torch_ms(torch, rec, order, nets, S, epochs, minibatch):
    import copy
    saved = up.EPOCHS, up.MINIBATCH
    up.EPOCHS, up.MINIBATCH = epochs, minibatch
    torch.distributions.Distribution.set_default_validate_args(False)      # (timed, not judged)
    try:
        pair = copy.deepcopy(nets)
        return 1e3 * up.torch_loop(torch, rec, order["order_inter"], order["first_inter"], [pair[0]], [pair[1]], S)
    finally:
        up.EPOCHS, up.MINIBATCH = saved


def compare(torch, B, T, widths, epochs, minibatch, binds, blocks, calls):
    """{name: series} of ``binds`` ({name: (ppo_bind arguments, calls per block)}) on twin handles, blocks alternated, and the eager loop"""
    handles, nets = {}, None
    for name, (bind, _) in binds.items():
        handles[name] = _agent(torch, B, T, widths, epochs, nets, **bind)
        nets = handles[name][3]
        _calls(torch, *handles[name][:3], 1, epochs, minibatch)             # (warm-up: the first call also loads the kernels)
    ms = {name: [] for name in binds}
    for _ in range(blocks):
        for name, (_, per_block) in binds.items():
            ms[name] += _calls(torch, *handles[name][:3], per_block if per_block else calls, epochs, minibatch)
    env, rec, order, _ = next(iter(handles.values()))
    out = {name: _series(x) for name, x in ms.items()}
    out["torch"] = _series([_torch_ms(torch, rec, order, nets, env.S, epochs, minibatch) for _ in range(2)])
    out["rows"], out["optimiser_steps"] = B * T, epochs * -(-B * T // minibatch)
    for env, _, _, _ in handles.values():
        env.close()
    return out


def measure_collected(blocks):
    import torch
    out = {}
    for widths in ([64, 64], [256, 256]):
        for minibatch in (8192, 65536):
            binds = {"spread_64": (dict(spread=True, slabs=64), 3), "spread_256": (dict(spread=True, slabs=256), 3), "plain": (dict(), 1)}
            key = "x".join(map(str, widths)) + f"_mb{minibatch}"
            out[key] = compare(torch, 4096, 64, widths, 4, minibatch, binds, blocks, 3)
            out[key]["plain_over_spread_64"] = out[key]["plain"]["ms"] / out[key]["spread_64"]["ms"]
            out[key]["torch_over_spread_64"] = out[key]["torch"]["ms"] / out[key]["spread_64"]["ms"]
            print("collected", key, json.dumps(out[key]), flush=True)
    return out


def measure_reference(blocks):
    import torch
    out = {}
    cases = [([64, 64], 64, False), ([256, 256], 64, False), (wp.VERYBIG, 16, True), (wp.VERYBIG, 64, True)]
    for widths, minibatch, wide in cases:
        binds = {"spread_64": (dict(spread=True, slabs=64, wide=wide), 3), "plain": (dict(wide=wide), 3)}
        key = "x".join(map(str, widths)) + f"_mb{minibatch}"
        out[key] = compare(torch, up.ROWS // up.T, up.T, widths, up.EPOCHS, minibatch, binds, blocks, 3)
        out[key]["plain_over_spread_64"] = out[key]["plain"]["ms"] / out[key]["spread_64"]["ms"]
        out[key]["torch_over_spread_64"] = out[key]["torch"]["ms"] / out[key]["spread_64"]["ms"]
        print("reference", key, json.dumps(out[key]), flush=True)
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
    lib = __import__("ctypes").CDLL(_lib.LIB_PATH)
    for n in NEW_EXPORTS:                             # (the parent's library has not the new exports and runs both)
        if not hasattr(lib, n):
            _lib.FUNCTIONS.pop(n, None)
    _lib.EXPORTS = tuple(_lib.FUNCTIONS)
    rollout = up.measure_rollout()
    env, rec, order, _ = _agent(torch, up.ROWS // up.T, up.T, [64, 64], up.EPOCHS)
    ms = _calls(torch, env, rec, order, 6, up.EPOCHS, up.MINIBATCH)[1:]
    print(json.dumps({"rollout_ms": rollout, "update_ms": statistics.median(ms)}))


def measure_unchanged(baseline, alternations):
    base, new = [], []
    for _ in range(alternations):
        base.append(_child(baseline))
        new.append(_child(None))
    out = {}
    for k in ("rollout_ms", "update_ms"):
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
    result = {"size": "S5_U25", "hp": up.HP}
    if os.path.exists(args.out):                     # (parts measured in an earlier job of the same series stay)
        with open(args.out) as f:
            result.update(json.load(f))
    if "c" in parts and args.baseline_lib:
        result["unchanged"] = measure_unchanged(args.baseline_lib, args.alternations)
    if "a" in parts:
        result["collected"] = measure_collected(args.blocks)
    if "b" in parts:
        result["reference"] = measure_reference(args.blocks)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
