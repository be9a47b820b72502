"""What training the non-shared IBSched agent over the chip costs (ppo_bind(per_slice=True, spread=True, slabs=N)), one MI355X, one job,
alternated blocks, medians, spreads reported:

  large     B 4096 x 64 TTIs (262 144 inter rows), 4 epochs, minibatch 8192, S 5 and S 10, [64, 64] and [256, 256] nets, the row
            lists drawn on the device once per shape:
              spread64_ms / spread256_ms   ppo_update_per_slice under this binding at 64 and at 256 slabs
              plain_ms                     the same call under ppo_bind(per_slice=True) with force=True: 1 + S workgroups (one repeat per block)
              shared64_ms / shared256_ms   ppo_update under ppo_bind(spread=True) on the SAME record for one shared intra pair
  reference the reference's own regime -- 2048 record rows, minibatch 64, 10 epochs -- under this binding (64 slabs) and the per-slice one
  parent    with --baseline-lib PATH (the parent commit's libranenv_hip.so): rollout(200) at B 4096 and a plain ppo_update_per_slice
            (the reference's regime, S 5, [64, 64]) with this library and with that one in processes of their own, alternated: ratio of
            the medians and the parent's own spread in this job.  The kernels of both are identical: that spread is the margin.

Writes profiles/ppo_per_slice_spread_probe.json (--out: elsewhere) and prints it as one line.

    python tools/ppo_per_slice_spread_probe.py [--repeats 3] [--blocks 2] [--slices 5,10] [--baseline-lib parent.so] [--out FILE]
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
import ppo_per_slice_probe as pp  # noqa: E402
import ppo_update_probe as up  # noqa: E402

OUT = os.path.join(REPO, "profiles", "ppo_per_slice_spread_probe.json")
LARGE = dict(batch=4096, ttis=64, epochs=4, minibatch=8192)
SLABS = (64, 256)
NETS = (("64x64", [64, 64]), ("256x256", [256, 256]))


def _timed(torch, f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()                                      # (returns behind a device read-back)
    return 1e3 * (time.perf_counter() - t0)


def _blocks(torch, calls, blocks, repeats, once=()):
    """{name: [ms]} of the calls in alternated blocks; the names in ``once`` run one repeat per block"""
    ms = {k: [] for k in calls}
    for f in calls.values():                 # (the first call also loads the kernel)
        f()
    for _ in range(blocks):
        for k, f in calls.items():
            for _ in range(1 if k in once else repeats):
                ms[k].append(_timed(torch, f))
    return ms


def _summary(ms):
    out = {}
    for k, v in ms.items():
        out[k + "_ms"], out[k + "_all_ms"], out[k + "_spread"] = statistics.median(v), v, max(v) / min(v) - 1.0
    return out


def _handles(torch, S, widths, batch, binds):
    """One handle per entry of ``binds`` ({name: (shared intra pair?, ppo_bind arguments)}) under the same nets"""
    torch.manual_seed(S)
    envs = {k: pp._workload(torch, S, batch) for k in binds}
    W = next(iter(envs.values())).W
    inter, v_inter = up._mlp(torch, [10 * S] + widths + [2 * S]).cuda(), up._mlp(torch, [10 * S] + widths + [1]).cuda()
    intra, v_intra = [up._mlp(torch, [W] + widths + [3]).cuda() for _ in range(S)], [up._mlp(torch, [W] + widths + [1]).cuda() for _ in range(S)]
    for k, (shared, bind) in binds.items():
        envs[k].set_policy_network(inter, intra[0] if shared else intra, stochastic=True, seed=3)
        envs[k].set_value_network(v_inter, v_intra[0] if shared else v_intra)
        envs[k].ppo_bind(**bind)
    return envs


def measure_large(repeats, blocks, slices):
    import torch
    out = {}
    E, MB = LARGE["epochs"], LARGE["minibatch"]
    for S in slices:
        for name, widths in NETS:
            binds = {"plain": (False, dict(per_slice=True))}
            for n in SLABS:
                binds[f"spread{n}"] = (False, dict(per_slice=True, spread=True, slabs=n))
                binds[f"shared{n}"] = (True, dict(spread=True, slabs=n))
            envs = _handles(torch, S, widths, LARGE["batch"], binds)
            lead = envs["spread64"]
            lead.reset()
            rec = lead.collect(LARGE["ttis"])
            o_per = lead.ppo_row_order(rec, E, seed=1, per_slice=True)
            o_shared = envs["shared64"].ppo_row_order(rec, E, seed=1)
            calls = {}
            for k, e in envs.items():
                if k.startswith("shared"):
                    calls[k] = lambda e=e: e.ppo_update(rec, epochs=E, minibatch=MB, order=o_shared, **up.HP)
                else:
                    calls[k] = lambda e=e, k=k: e.ppo_update_per_slice(rec, epochs=E, minibatch=MB, order=o_per, force=k == "plain", **up.HP)
            row = _summary(_blocks(torch, calls, blocks, repeats, once=("plain",)))
            first = o_per["first_intra"]
            row.update(inter_rows=int(o_per["first_inter"][1]), intra_rows_per_slice=[int(x) for x in (first[1:] - first[:-1])],
                       intra_rows_shared=int(o_shared["first_intra"][1]))
            for n in SLABS:
                row[f"plain_over_spread{n}"] = row["plain_ms"] / row[f"spread{n}_ms"]
                row[f"spread{n}_over_shared{n}"] = row[f"spread{n}_ms"] / row[f"shared{n}_ms"]
            out[f"S{S}_{name}"] = row
            print(f"S{S}_{name}", {k: v for k, v in row.items() if not k.endswith("_all_ms")}, flush=True)
            for e in envs.values():
                e.close()
    return out


def measure_reference(repeats, blocks, slices):
    """The reference's regime (2048 record rows, minibatch 64, 10 epochs): this binding at 64 slabs against the per-slice one"""
    import torch
    from intent_radio_sched_multi_slice_amd.adapters import ppo_row_order
    out = {}
    for S in slices:
        for name, widths in NETS:
            envs = _handles(torch, S, widths, pp.B, {"plain": (False, dict(per_slice=True)), "spread64": (False, dict(per_slice=True, spread=True, slabs=64))})
            envs["plain"].reset()
            rec = envs["plain"].collect(up.T)
            order = ppo_row_order(rec, [0, pp.B], up.EPOCHS, seed=1, per_slice=True)
            calls = {k: (lambda e=e: e.ppo_update_per_slice(rec, epochs=up.EPOCHS, minibatch=up.MINIBATCH, order=order, **up.HP)) for k, e in envs.items()}
            row = _summary(_blocks(torch, calls, blocks, repeats))
            row["spread64_over_plain"] = row["spread64_ms"] / row["plain_ms"]
            out[f"S{S}_{name}"] = row
            print(f"reference S{S}_{name}", {k: v for k, v in row.items() if not k.endswith("_all_ms")}, flush=True)
            for e in envs.values():
                e.close()
    return out


def _child(lib):
    env = dict(os.environ)
    if lib:
        env["RANENV_LIB"] = os.path.abspath(lib)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=600)
    return json.loads(res.stdout.strip().split("\n")[-1])


def _child_run():
    """rollout(200) at B 4096 and the plain per-slice update in the reference's regime, with whatever library RANENV_LIB names"""
    import torch
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.adapters import ppo_row_order
    lib = __import__("ctypes").CDLL(_lib.LIB_PATH)
    for n in list(_lib.FUNCTIONS):           # (the parent's library has not the new exports and can run both)
        if not hasattr(lib, n):
            _lib.FUNCTIONS.pop(n)
    _lib.EXPORTS = tuple(_lib.FUNCTIONS)
    rollout = up.measure_rollout()
    env = _handles(torch, 5, [64, 64], pp.B, {"plain": (False, dict(per_slice=True))})["plain"]
    env.reset()
    rec = env.collect(up.T)
    order = ppo_row_order(rec, [0, pp.B], up.EPOCHS, seed=1, per_slice=True)
    f = lambda: env.ppo_update_per_slice(rec, epochs=up.EPOCHS, minibatch=up.MINIBATCH, order=order, **up.HP)  # noqa: E731
    f()
    ms = [_timed(torch, f) for _ in range(5)]
    env.close()
    print(json.dumps({"rollout_ms": rollout, "update_ms": statistics.median(ms)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--slices", default="5,10")
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        _child_run()
        return
    slices = [int(x) for x in args.slices.split(",")]
    result = {"large_regime": dict(LARGE, slabs=list(SLABS), ues_per_slice=5),
              "reference_regime": {"record_rows": up.ROWS, "minibatch": up.MINIBATCH, "epochs": up.EPOCHS, "ues_per_slice": 5}}
    if args.baseline_lib:
        base, new = [], []
        for _ in range(args.alternations):
            base.append(_child(args.baseline_lib))
            new.append(_child(None))
        result["parent"] = {}
        for what in ("rollout_ms", "update_ms"):
            b, n = [x[what] for x in base], [x[what] for x in new]
            ratio, spread = statistics.median(n) / statistics.median(b), max(b) / min(b) - 1.0
            result["parent"][what] = {"baseline": b, "this": n, "ratio": ratio, "baseline_spread": spread, "within_spread": abs(ratio - 1.0) <= spread}
        print("parent", result["parent"], flush=True)
    result["reference"] = measure_reference(args.repeats, args.blocks, slices)
    result["large"] = measure_large(args.repeats, args.blocks, slices)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
