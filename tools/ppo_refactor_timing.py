"""Do the PPO training kernels of two builds cost the same?  The device update of every PPO training path, in the update regimes of
the paths' own probes (tools/ppo_update_probe.py, ppo_mixed_probe.py, ppo_wide_probe.py, ppo_per_slice_probe.py, ppo_head_probe.py,
ppo_spread_probe.py, ppo_head_spread_probe.py: their workloads, nets, row lists and timed calls, without the eager-torch loops),
under a baseline library and under the tree's own, alternated baseline / this / baseline / this, every series in a process of its own.

A path holds its speed when the median of this build's calls is not above the baseline's by more than the baseline's own spread between
its series (max / min - 1 of the series' medians).  Writes profiles/ppo_refactor_timing.json (--out: elsewhere): every call of every
series, and per path the two medians, the baseline's spread, the ratio and the verdict.

    python tools/ppo_refactor_timing.py --baseline-lib parent.so [--series 2] [--paths "per slice,head"] [--out FILE]
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
OUT = os.path.join(REPO, "profiles", "ppo_refactor_timing.json")


def measure(only):
    """{path: [ms of every timed call]} under the library the package loads; a path's first call (it loads the kernels) is dropped.
    ``only``: the paths whose name holds one of these strings (empty: all)"""
    import torch
    from intent_radio_sched_multi_slice_amd.adapters import ppo_head_row_order, ppo_row_order
    import ppo_head_probe as hp
    import ppo_head_spread_probe as hs
    import ppo_mixed_probe as mp
    import ppo_per_slice_probe as ps
    import ppo_spread_probe as sp
    import ppo_update_probe as up
    import ppo_wide_probe as wp
    out = {}
    wanted = lambda name: not only or any(x in name for x in only)  # noqa: E731

    def keep(name, ms):
        out[name] = ms[1:]
        print(name, [round(x, 2) for x in ms], flush=True)

    # ranenv_ppo_update_kernel, _mixed, _wide, _mixed_wide: 2048 rows per member, 10 epochs, minibatch 64
    for name, G, widths_of, mixed, wide, calls in (("uniform 8 x [64, 64]", 8, lambda m: [64, 64], False, False, 6),
                                                  ("mixed 8 members", 8, lambda m: mp.ARCHS[m % len(mp.ARCHS)], True, False, 4),
                                                  ("wide 8 x [512] x 3", 8, lambda m: wp.VERYBIG, False, True, 4),
                                                  ("mixed wide 10 members", 10, lambda m: wp.ARCHS[m % len(wp.ARCHS)], True, True, 4)):
        if not wanted(name):
            continue
        env, rec, order, _, _ = wp._population(torch, G, widths_of, mixed, wide)
        keep(name, wp._calls(torch, env, rec, order, calls, up.MINIBATCH))
        env.close()

    # ranenv_ppo_update_kernel_slices, _slices_wide: S 5, [64, 64], the per-slice probe's nets and lists
    for name, bind in (("per slice S 5 [64, 64]", dict()), ("per slice wide S 5 [64, 64]", dict(wide=True))):
        if not wanted(name):
            continue
        S, widths = 5, [64, 64]
        torch.manual_seed(S)
        env = ps._workload(torch, S)
        W = env.W
        inter, v_inter = up._mlp(torch, [10 * S] + widths + [2 * S]).cuda(), up._mlp(torch, [10 * S] + widths + [1]).cuda()
        intra, v_intra = [up._mlp(torch, [W] + widths + [3]).cuda() for _ in range(S)], [up._mlp(torch, [W] + widths + [1]).cuda() for _ in range(S)]
        env.set_policy_network(inter, intra, stochastic=True, seed=3)
        env.set_value_network(v_inter, v_intra)
        env.ppo_bind(per_slice=True, **bind)
        env.reset()
        rec = env.collect(up.T)
        order = ppo_row_order(rec, [0, ps.B], up.EPOCHS, seed=1, per_slice=True)
        ms = []
        for _ in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            env.ppo_update_per_slice(rec, epochs=up.EPOCHS, minibatch=up.MINIBATCH, order=order, **up.HP)
            ms.append(1e3 * (time.perf_counter() - t0))
        keep(name, ms)
        env.close()

    # ranenv_ppo_update_kernel_head and the head spread kernels: S 5, SB3's [64, 64] pair
    for name, B, T, epochs, minibatch, bind, calls in (("head S 5", hp.ROWS // hp.T, hp.T, hp.EPOCHS, hp.MINIBATCH, dict(), 6),
                                                       ("head spread 64 slabs, 2048 rows", hp.ROWS // hp.T, hp.T, hp.EPOCHS, hp.MINIBATCH, dict(spread=True, slabs=64), 6),
                                                       ("head spread 64 slabs, 262144 rows", 4096, 64, 4, 8192, dict(spread=True, slabs=64), 6)):
        if not wanted(name):
            continue
        env, *_ = hp._head_env(torch, B, 5)
        env.ppo_bind(head=True, **bind)
        rec = env.collect_head(T)
        keep(name, hs._calls(torch, env, rec, ppo_head_row_order(rec, epochs, seed=1), calls, epochs, minibatch))
        env.close()

    # the spread kernels of the IBSched nets: pass, pass wide, reduce, apply
    for name, B, T, widths, epochs, minibatch, bind, calls in (("spread 64 slabs [64, 64], 2048 rows", up.ROWS // up.T, up.T, [64, 64], up.EPOCHS, 64, dict(slabs=64), 6),
                                                               ("spread 64 slabs [64, 64], 262144 rows", 4096, 64, [64, 64], 4, 8192, dict(slabs=64), 6),
                                                               ("spread wide 64 slabs [512] x 3, 2048 rows", up.ROWS // up.T, up.T, wp.VERYBIG, up.EPOCHS, 64, dict(slabs=64, wide=True), 4)):
        if not wanted(name):
            continue
        env, rec, order, _ = sp._agent(torch, B, T, widths, epochs, spread=True, **bind)
        keep(name, sp._calls(torch, env, rec, order, calls, epochs, minibatch))
        env.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--series", type=int, default=2)
    ap.add_argument("--paths", default="")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        measure([x for x in args.paths.split(",") if x])
        return
    assert args.baseline_lib, "--baseline-lib: the library to compare with"
    runs = {"baseline": [], "this": []}
    for _ in range(args.series):
        for which in ("baseline", "this"):
            env = dict(os.environ)
            env.pop("RANENV_LIB", None)
            if which == "baseline":
                env["RANENV_LIB"] = os.path.abspath(args.baseline_lib)
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--paths", args.paths], env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=300)
            runs[which].append(json.loads(res.stdout.strip().split("\n")[-1]))
            print(which, "series", len(runs[which]), "done", flush=True)
    table = {}
    for path in runs["baseline"][0]:
        base, this = [r[path] for r in runs["baseline"]], [r[path] for r in runs["this"]]
        medians = [statistics.median(s) for s in base]
        b, t, spread = statistics.median(sum(base, [])), statistics.median(sum(this, [])), max(medians) / min(medians) - 1.0
        table[path] = {"baseline_ms": b, "baseline_spread": spread, "this_ms": t, "ratio": t / b, "holds": t / b <= 1.0 + spread,
                       "baseline_series_ms": base, "this_series_ms": this}
        print(f"{path}: baseline {b:.2f} ms (spread {100 * spread:.2f} %), this {t:.2f} ms, ratio {t / b:.4f}{'' if table[path]['holds'] else '  SLOWER'}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(table, f, indent=1)


if __name__ == "__main__":
    main()
