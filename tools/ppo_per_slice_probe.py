"""What training non-shared intra policies on the device costs (ppo_bind(per_slice=True), ppo_update_per_slice), one job:

  update    at 2048 record rows (T 32 x B 64), minibatch 64, 10 epochs, for S 5 and S 10 with [64, 64] and [256, 256] nets, alternated and
            reported as medians of --repeats calls per block:
              per_slice_ms   ppo_update_per_slice: 1 + S workgroups, slice s's pair on slice s's live rows
              shared_ms      ppo_update on the SAME record for one shared intra pair: 2 workgroups, the intra one on all live rows
              torch_ms       the eager-torch SGD loop of examples/train_ppo_on_device.py over the 1 + S policies, one after the other,
                             on the same chunks (one repeat)
  rollout   with --baseline-lib PATH (the parent commit's libranenv_hip.so): rollout(200) at B 4096 with this library and with that
            one in processes of their own, alternated: ratio of the medians and the parent's own spread in this job

Writes profiles/ppo_per_slice_probe.json (--out: elsewhere) and prints it as one line.

    python tools/ppo_per_slice_probe.py [--repeats 3] [--blocks 3] [--slices 5,10] [--baseline-lib parent.so] [--out FILE]
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

OUT = os.path.join(REPO, "profiles", "ppo_per_slice_probe.json")
B = up.ROWS // up.T


def _workload(torch, S, batch=B):
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    return make_mult_slice_workload(batch, torch.device("cuda", 0), policy=_lib.POLICY_MAPF, intra=_lib.INTRA_PF, n_scenarios=8, n_traces=8,
                                    trace_len=64, max_steps=1000, n_slices=S, n_ues=5 * S, n_rbs=135, rbs_per_rbg=5, max_ues_slice=5).env


def torch_intra_loop(torch, rec, order, first, actors, critics, S):
    """The example's eager SGD for the S intra pairs on slice s's chunks of ``order``, pair after pair; returns seconds"""
    W = rec["obs_intra"].shape[-1]
    obs, act = rec["obs_intra"].reshape(-1, W), rec["action_intra"].reshape(-1).long()
    cell = lambda name: rec[name][..., 1:].reshape(-1)  # noqa: E731  (row (t * B + b) * S + s <-> cell [t][b][1 + s])
    logp0, adv0, vt0 = cell("logp"), cell("adv"), cell("vtarg")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s, (pi, vf) in enumerate(zip(actors, critics)):
        opt = torch.optim.Adam(list(pi.parameters()) + list(vf.parameters()), lr=up.HP["lr"])
        lo, hi = int(first[s]), int(first[s + 1])
        for ep in range(up.EPOCHS):
            for c0 in range(lo, hi, up.MINIBATCH):
                idx = order[ep, c0:min(c0 + up.MINIBATCH, hi)].long()
                cat = torch.distributions.Categorical(logits=pi(obs[idx]))
                adv = adv0[idx]
                adv = (adv - adv.mean()) / (adv.std() + 1e-8)
                ratio = torch.exp(cat.log_prob(act[idx]) - logp0[idx])
                surr = torch.minimum(ratio * adv, ratio.clamp(1.0 - up.HP["clip"], 1.0 + up.HP["clip"]) * adv)
                loss = -surr.mean() + up.HP["vf_coeff"] * (vf(obs[idx])[:, 0] - vt0[idx]).pow(2).mean() - up.HP["ent_coeff"] * cat.entropy().mean()
                opt.zero_grad(set_to_none=True)
                loss.backward()
                torch.nn.utils.clip_grad_norm_([p for g in opt.param_groups for p in g["params"]], up.HP["grad_clip"])
                opt.step()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def measure_update(repeats, blocks, slices):
    import torch
    from intent_radio_sched_multi_slice_amd.adapters import ppo_row_order
    out = {}
    for S in slices:
        for name, widths in (("64x64", [64, 64]), ("256x256", [256, 256])):
            torch.manual_seed(S)
            per, shared = _workload(torch, S), _workload(torch, S)
            W = per.W
            inter, v_inter = up._mlp(torch, [10 * S] + widths + [2 * S]).cuda(), up._mlp(torch, [10 * S] + widths + [1]).cuda()
            intra, v_intra = [up._mlp(torch, [W] + widths + [3]).cuda() for _ in range(S)], [up._mlp(torch, [W] + widths + [1]).cuda() for _ in range(S)]
            per.set_policy_network(inter, intra, stochastic=True, seed=3)
            per.set_value_network(v_inter, v_intra)
            per.ppo_bind(per_slice=True)
            shared.set_policy_network(inter, intra[0], stochastic=True, seed=3)
            shared.set_value_network(v_inter, v_intra[0])
            shared.ppo_bind()
            per.reset()
            rec = per.collect(up.T)
            o_per = ppo_row_order(rec, [0, B], up.EPOCHS, seed=1, per_slice=True)
            o_shared = ppo_row_order(rec, [0, B], up.EPOCHS, seed=1)
            calls = {"per_slice": lambda: per.ppo_update_per_slice(rec, epochs=up.EPOCHS, minibatch=up.MINIBATCH, order=o_per, **up.HP),
                     "shared": lambda: shared.ppo_update(rec, epochs=up.EPOCHS, minibatch=up.MINIBATCH, order=o_shared, **up.HP)}
            ms = {k: [] for k in calls}
            for f in calls.values():             # (the first call also loads the kernel)
                f()
            for _ in range(blocks):              # (alternated blocks)
                for k, f in calls.items():
                    for _ in range(repeats):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        f()                      # (returns behind a device read-back)
                        ms[k].append(1e3 * (time.perf_counter() - t0))
            t_torch = 1e3 * (up.torch_loop(torch, rec, o_per["order_inter"], o_per["first_inter"], [inter], [v_inter], S)
                             + torch_intra_loop(torch, rec, o_per["order_intra"], o_per["first_intra"], intra, v_intra, S))
            p, sh = statistics.median(ms["per_slice"]), statistics.median(ms["shared"])
            row = {"per_slice_ms": p, "shared_ms": sh, "per_slice_over_shared": p / sh, "torch_ms": t_torch, "torch_over_per_slice": t_torch / p,
                   "per_slice_all_ms": ms["per_slice"], "shared_all_ms": ms["shared"], "shared_spread": max(ms["shared"]) / min(ms["shared"]) - 1.0,
                   "intra_rows_per_slice": [int(x) for x in (o_per["first_intra"][1:] - o_per["first_intra"][:-1])], "inter_rows": up.ROWS}
            out[f"S{S}_{name}"] = row
            print(f"S{S}_{name}", row, flush=True)
            per.close()
            shared.close()
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
    for n in list(_lib.FUNCTIONS):                   # (the parent's library has not the new exports and can run the rollout)
        if not hasattr(lib, n):
            _lib.FUNCTIONS.pop(n)
    _lib.EXPORTS = tuple(_lib.FUNCTIONS)
    print(json.dumps({"rollout_ms": up.measure_rollout()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--slices", default="5,10")
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--child-rollout", action="store_true")
    args = ap.parse_args()
    if args.child_rollout:
        _child_rollout()
        return
    result = {"regime": {"record_rows": up.ROWS, "minibatch": up.MINIBATCH, "epochs": up.EPOCHS, "ues_per_slice": 5}}
    if args.baseline_lib:
        base, new = [], []
        for _ in range(args.alternations):
            base.append(_child(args.baseline_lib))
            new.append(_child(None))
        ratio, spread = statistics.median(new) / statistics.median(base), max(base) / min(base) - 1.0
        result["rollout"] = {"baseline_ms": base, "this_ms": new, "ratio": ratio, "baseline_spread": spread, "within_spread": abs(ratio - 1.0) <= spread}
        print("rollout", result["rollout"], flush=True)
    result["update"] = measure_update(args.repeats, args.blocks, [int(x) for x in args.slices.split(",")])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
