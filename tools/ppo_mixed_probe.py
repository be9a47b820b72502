"""What training a MIXED population on the device costs, at the regime of tools/ppo_update_probe.py -- 2048 rows per member, minibatch
64, 10 epochs, S 5 / U 25, inter nets only -- for G = 8 and 64 members whose architectures cycle through the reference's four
trainable ones, [64, 64], [256, 256], [400, 300] and [256, 256, 256]:

  (a) mixed_ms      one ppo_update call over the mixed population (median of --repeats calls behind a warm-up call)
  (b) uniform_ms    the sum of four ppo_update calls, one per architecture, each over a uniform population of G / 4 members
  (c) torch_ms      the eager-torch SGD loop over the same chunks, member after member (one pass)

A mixed call cannot be faster than its slowest member, which works on one compute unit; (b)'s four calls each wait for theirs.

With --baseline-lib PATH (the parent commit's libranenv_hip.so): a uniform [64, 64] ppo_update over 8 members and rollout(200) at
B 4096, with this library and with that one, in processes of their own, alternated in one job -- their kernels are unchanged, so the
medians should lie within the spread the parent shows against itself in the same job.

Writes profiles/ppo_mixed_probe.json (--out: elsewhere) and prints it as one line.

    python tools/ppo_mixed_probe.py [--repeats 3] [--members 8,64] [--baseline-lib parent.so] [--out FILE]
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

OUT = os.path.join(REPO, "profiles", "ppo_mixed_probe.json")
ARCHS = ([64, 64], [256, 256], [400, 300], [256, 256, 256])
NEW_EXPORTS = ("ranenv_ppo_bind_mixed", "ranenv_ppo_member_layout", "ranenv_ppo_lds_bytes")


def _population(torch, G, widths_of, mixed):
    """A reset env of G members of 2048 rows under the nets widths_of(m), PPO state bound, with its record and row lists"""
    from intent_radio_sched_multi_slice_amd.adapters import ppo_row_order
    B = G * (up.ROWS // up.T)
    env = up._workload(torch, B)
    S = env.S
    torch.manual_seed(G)
    actors = [up._mlp(torch, [10 * S] + widths_of(m) + [2 * S]).cuda() for m in range(G)]
    critics = [up._mlp(torch, [10 * S] + widths_of(m) + [1]).cuda() for m in range(G)]
    env.set_population(sizes=[B // G] * G)
    env.set_policy_network(actors, None, stochastic=True, seed=3, mixed=mixed)
    env.set_value_network(critics, None, mixed=mixed)
    env.ppo_bind(mixed=mixed)
    env.reset()
    rec = env.collect(up.T)
    order = ppo_row_order(rec, env.population(), up.EPOCHS, seed=1, intra=False)
    return env, rec, order, actors, critics


def _time_update(torch, env, rec, order, repeats):
    ms = []
    for _ in range(repeats + 1):                      # (the first call also loads the kernel)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env.ppo_update(rec, epochs=up.EPOCHS, minibatch=up.MINIBATCH, order=order, **up.HP)       # (returns behind a device read-back)
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms[1:]), ms


def measure_mixed(repeats, members):
    import torch
    out = {}
    for G in members:
        assert G % len(ARCHS) == 0
        env, rec, order, actors, critics = _population(torch, G, lambda m: ARCHS[m % len(ARCHS)], True)
        mixed_ms, mixed_all = _time_update(torch, env, rec, order, repeats)
        lds = [env.ppo_member_layout(m, "inter")["lds_bytes"] for m in range(len(ARCHS))]
        torch_ms = 1e3 * up.torch_loop(torch, rec, order["order_inter"], order["first_inter"], actors, critics, env.S)
        env.close()
        uniform = {}
        for widths in ARCHS:
            env, rec, order, _, _ = _population(torch, G // len(ARCHS), lambda m: widths, False)
            uniform["x".join(map(str, widths))] = _time_update(torch, env, rec, order, repeats)[0]
            env.close()
        out[str(G)] = {"mixed_ms": mixed_ms, "mixed_all_ms": mixed_all, "uniform_ms": sum(uniform.values()), "uniform_each_ms": uniform,
                       "torch_ms": torch_ms, "member_lds_bytes": lds, "mixed_over_uniform": mixed_ms / sum(uniform.values()),
                       "torch_over_mixed": torch_ms / mixed_ms}
        print(G, out[str(G)], flush=True)
    return out


def measure_unchanged(repeats=5):
    """(uniform [64, 64] ppo_update over 8 members, rollout(200) at B 4096) in ms, with the library RANENV_LIB names"""
    import torch
    from intent_radio_sched_multi_slice_amd import _lib
    lib = __import__("ctypes").CDLL(_lib.LIB_PATH)
    for n in NEW_EXPORTS:                             # (the parent's library has none of them and can run both)
        if not hasattr(lib, n):
            _lib.FUNCTIONS.pop(n, None)
    from intent_radio_sched_multi_slice_amd.adapters import ppo_row_order
    G, B = 8, 8 * (up.ROWS // up.T)
    env = up._workload(torch, B)
    S = env.S
    torch.manual_seed(G)
    env.set_population(sizes=[B // G] * G)
    env.set_policy_network([up._mlp(torch, [10 * S, 64, 64, 2 * S]).cuda() for _ in range(G)], None, stochastic=True, seed=3)
    env.set_value_network([up._mlp(torch, [10 * S, 64, 64, 1]).cuda() for _ in range(G)], None)
    env.ppo_bind()
    env.reset()
    rec = env.collect(up.T)
    order = ppo_row_order(rec, env.population(), up.EPOCHS, seed=1, intra=False)
    update_ms = _time_update(torch, env, rec, order, repeats)[0]
    env.close()
    return update_ms, up.measure_rollout()


def _child(lib):
    env = dict(os.environ)
    if lib:
        env["RANENV_LIB"] = os.path.abspath(lib)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, check=True, capture_output=True, text=True, timeout=600)
    return json.loads(res.stdout.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--members", default="8,64")
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        update_ms, rollout_ms = measure_unchanged()
        print(json.dumps({"update_ms": update_ms, "rollout_ms": rollout_ms}))
        return
    result = {"regime": {"rows_per_member": up.ROWS, "minibatch": up.MINIBATCH, "epochs": up.EPOCHS, "size": "S5_U25", "architectures": list(ARCHS)}}
    if args.baseline_lib:
        base, new = [], []
        for _ in range(args.alternations):
            base.append(_child(args.baseline_lib))
            new.append(_child(None))
        result["unchanged"] = {}
        for key in ("update_ms", "rollout_ms"):
            b, n = [x[key] for x in base], [x[key] for x in new]
            ratio, spread = statistics.median(n) / statistics.median(b), max(b) / min(b) - 1.0
            result["unchanged"][key] = {"baseline": b, "this": n, "ratio": ratio, "baseline_spread": spread, "within_spread": abs(ratio - 1.0) <= spread}
    result["cases"] = measure_mixed(args.repeats, [int(x) for x in args.members.split(",")])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
