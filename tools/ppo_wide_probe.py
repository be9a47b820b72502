"""What training nets beyond the LDS plan costs under the wide binding (ppo_bind(wide=True)), S 5 / U 25, inter nets only, one job:

  (a) verybig        ppo_update under a wide binding for [512, 512, 512] at G = 1 / 8 / 64 in the regime of tools/ppo_update_probe.py
                     (2048 rows per member, minibatch 64, 10 epochs), beside the eager-torch loop of that probe over the same chunks
                     (at G = 64 the loop, sequential member after member, is timed on 8 members and scaled by 8)
  (b) pre_computed   the same at the reference's pre_computed regime: minibatch 16, 10 epochs
  (c) parking        [64, 64] and [256, 256] at G = 8 under the wide binding over the plain one: the cost of parking the rows
  (d) mixed          a mixed wide call whose members cycle through all five architectures of the reference's search, against the sum
                     of five uniform calls (the four that fit it under the plain binding, [512] x 3 under the wide one)
  (e) rollout        with --baseline-lib PATH (the parent commit's libranenv_hip.so): rollout(200) at B 4096 with this library and with
                     that one in processes of their own

Device timings are medians of --repeats calls behind a warm-up call; where two bindings or two libraries are compared their blocks
alternate.  Writes profiles/ppo_wide_probe.json (--out: elsewhere) and prints it as one line.

    python tools/ppo_wide_probe.py [--repeats 3] [--members 1,8,64] [--parts a,b,c,d,e] [--baseline-lib parent.so] [--out FILE]
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

OUT = os.path.join(REPO, "profiles", "ppo_wide_probe.json")
VERYBIG = [512, 512, 512]
ARCHS = ([64, 64], [256, 256], [400, 300], [256, 256, 256], VERYBIG)
NEW_EXPORTS = ("ranenv_ppo_bind_wide", "ranenv_ppo_wide_bytes")
TORCH_MEMBERS = 8                        # members the eager-torch loop is timed on; beyond, its time is scaled by G / 8


def _population(torch, G, widths_of, mixed, wide):
    """A reset env of G members of 2048 rows under the nets widths_of(m), PPO state bound, with its record, row lists and nets"""
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
    env.ppo_bind(mixed=mixed, wide=wide)
    env.reset()
    rec = env.collect(up.T)
    order = ppo_row_order(rec, env.population(), up.EPOCHS, seed=1, intra=False)
    return env, rec, order, actors, critics


def _calls(torch, env, rec, order, n, minibatch):
    ms = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env.ppo_update(rec, epochs=up.EPOCHS, minibatch=minibatch, order=order, **up.HP)       # (returns behind a device read-back)
        ms.append(1e3 * (time.perf_counter() - t0))
    return ms


def _time_update(torch, env, rec, order, repeats, minibatch=up.MINIBATCH):
    ms = _calls(torch, env, rec, order, repeats + 1, minibatch)          # (the first call also loads the kernel)
    return statistics.median(ms[1:]), ms


def measure_verybig(repeats, members, minibatch, with_torch):
    import torch
    out = {}
    for G in members:
        env, rec, order, actors, critics = _population(torch, G, lambda m: VERYBIG, False, True)
        dev, all_ms = _time_update(torch, env, rec, order, repeats, minibatch)
        steps = up.EPOCHS * -(-up.ROWS // minibatch)
        row = {"device_ms": dev, "device_all_ms": all_ms, "optimiser_steps_per_member": steps, "ms_per_step": dev / steps,
               "lds_bytes": env.ppo_member_layout(0, "inter")["lds_bytes"]}
        if with_torch:
            saved = up.MINIBATCH
            up.MINIBATCH = minibatch                 # (the eager loop cuts its chunks by the module's figure)
            # (timed, not judged: at minibatch 16 the eager loop's lr 3e-4 drives some 512-wide member to NaN, which Normal would refuse)
            torch.distributions.Distribution.set_default_validate_args(False)
            n = min(G, TORCH_MEMBERS)                # (the loop is sequential, member after member: the first n members' time x G / n)
            row["torch_ms"] = 1e3 * up.torch_loop(torch, rec, order["order_inter"], order["first_inter"], actors[:n], critics[:n], env.S) * (G / n)
            row["torch_members_timed"] = n
            up.MINIBATCH = saved
            row["speedup"] = row["torch_ms"] / dev
        out[str(G)] = row
        print("verybig", minibatch, G, row, flush=True)
        env.close()
    return out


def measure_parking(repeats, G=8, blocks=3):
    import torch
    out = {}
    for widths in ([64, 64], [256, 256]):
        wide = _population(torch, G, lambda m: widths, False, True)
        plain = _population(torch, G, lambda m: widths, False, False)
        for env, rec, order, _, _ in (wide, plain):
            _calls(torch, env, rec, order, 1, up.MINIBATCH)
        w_ms, p_ms = [], []
        for _ in range(blocks):                      # (alternated blocks)
            w_ms += _calls(torch, wide[0], wide[1], wide[2], repeats, up.MINIBATCH)
            p_ms += _calls(torch, plain[0], plain[1], plain[2], repeats, up.MINIBATCH)
        w, p = statistics.median(w_ms), statistics.median(p_ms)
        out["x".join(map(str, widths))] = {"wide_ms": w, "plain_ms": p, "wide_over_plain": w / p, "wide_all_ms": w_ms, "plain_all_ms": p_ms,
                                           "plain_spread": max(p_ms) / min(p_ms) - 1.0}
        print("parking", widths, out["x".join(map(str, widths))], flush=True)
        wide[0].close()
        plain[0].close()
    return out


def measure_mixed(repeats, G=10):
    import torch
    assert G % len(ARCHS) == 0
    env, rec, order, _, _ = _population(torch, G, lambda m: ARCHS[m % len(ARCHS)], True, True)
    mixed_ms, mixed_all = _time_update(torch, env, rec, order, repeats)
    lds = [env.ppo_member_layout(m, "inter")["lds_bytes"] for m in range(len(ARCHS))]
    env.close()
    uniform = {}
    for widths in ARCHS:
        env, rec, order, _, _ = _population(torch, G // len(ARCHS), lambda m: widths, False, widths == VERYBIG)
        uniform["x".join(map(str, widths))] = _time_update(torch, env, rec, order, repeats)[0]
        env.close()
    out = {"members": G, "mixed_ms": mixed_ms, "mixed_all_ms": mixed_all, "uniform_ms": sum(uniform.values()), "uniform_each_ms": uniform,
           "member_lds_bytes": lds, "mixed_over_uniform": mixed_ms / sum(uniform.values())}
    print("mixed", out, flush=True)
    return out


def _child(lib):
    env = dict(os.environ)
    if lib:
        env["RANENV_LIB"] = os.path.abspath(lib)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-rollout"], env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=600)
    return json.loads(res.stdout.strip().split("\n")[-1])["rollout_ms"]


def _child_rollout():
    import torch  # noqa: F401  (its HIP runtime has to be in the process before the library's own is resolved, _lib.load)
    from intent_radio_sched_multi_slice_amd import _lib
    lib = __import__("ctypes").CDLL(_lib.LIB_PATH)
    for n in NEW_EXPORTS + up.NEW_EXPORTS:           # (the parent's library has not the new exports and can run the rollout)
        if not hasattr(lib, n):
            _lib.FUNCTIONS.pop(n, None)
    _lib.EXPORTS = tuple(_lib.FUNCTIONS)
    print(json.dumps({"rollout_ms": up.measure_rollout()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--members", default="1,8,64")
    ap.add_argument("--parts", default="a,b,c,d,e")
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--child-rollout", action="store_true")
    args = ap.parse_args()
    if args.child_rollout:
        _child_rollout()
        return
    parts, members = set(args.parts.split(",")), [int(x) for x in args.members.split(",")]
    result = {"regime": {"rows_per_member": up.ROWS, "epochs": up.EPOCHS, "size": "S5_U25", "verybig": VERYBIG}}
    if "e" in parts and args.baseline_lib:
        base, new = [], []
        for _ in range(args.alternations):
            base.append(_child(args.baseline_lib))
            new.append(_child(None))
        ratio, spread = statistics.median(new) / statistics.median(base), max(base) / min(base) - 1.0
        result["rollout"] = {"baseline_ms": base, "this_ms": new, "ratio": ratio, "baseline_spread": spread, "within_spread": abs(ratio - 1.0) <= spread}
        print("rollout", result["rollout"], flush=True)
    if "a" in parts:
        result["verybig_minibatch_64"] = measure_verybig(args.repeats, members, up.MINIBATCH, True)
    if "b" in parts:
        result["pre_computed_minibatch_16"] = measure_verybig(args.repeats, members, 16, True)
    if "c" in parts:
        result["parking"] = measure_parking(args.repeats)
    if "d" in parts:
        result["mixed"] = measure_mixed(args.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
