"""What the device PPO update costs: `ppo_update` against the eager-torch SGD loop of examples/train_ppo_on_device.py run per member,
at the reference's regime -- 2048 rows per member, minibatch 64, 10 epochs -- for G = 1, 8, 64 members and [64, 64] / [256, 256] nets
(S 5 / U 25, inter nets only on both sides: the same rows, the same chunks).

Writes profiles/ppo_update_probe.json (and prints it as one line):
  cases[net][G]: device_ms (median of --repeats ppo_update calls), torch_ms (the eager loop over all G members, one repeat), speedup
  rollout: with --baseline-lib PATH (the parent commit's libranenv_hip.so), rollout(200) at B 4096 with this library and with that
           one in processes of their own, alternated: ratio of the medians and the parent's own spread in this job

    python tools/ppo_update_probe.py [--repeats 3] [--baseline-lib parent.so] [--members 1,8,64]
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
OUT = os.path.join(REPO, "profiles", "ppo_update_probe.json")
NEW_EXPORTS = ("ranenv_ppo_bind", "ranenv_ppo_update", "ranenv_ppo_layout", "ranenv_ppo_state", "ranenv_ppo_probe_logp", "ranenv_get_net_weights")
ROWS, MINIBATCH, EPOCHS, T = 2048, 64, 10, 32
HP = dict(lr=3e-4, clip=0.2, vf_coeff=0.5, ent_coeff=0.01, grad_clip=0.5)


def _mlp(torch, dims):
    mods = []
    for i in range(len(dims) - 1):
        mods.append(torch.nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods)


def _workload(torch, B, **kw):
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    return make_mult_slice_workload(B, torch.device("cuda", 0), policy=_lib.POLICY_MAPF, intra=_lib.INTRA_PF, n_scenarios=8, n_traces=8,
                                    trace_len=64, max_steps=1000, n_slices=5, n_ues=25, n_rbs=135, rbs_per_rbg=5, max_ues_slice=5, **kw).env


def torch_loop(torch, rec, order, first, actors, critics, S):
    """The example's eager SGD on the same chunks, member after member; returns seconds"""
    from intent_radio_sched_multi_slice_amd.adapters import masked_gaussian_params, sorted_action_mask
    N = rec["logp"].shape[0] * rec["logp"].shape[1]
    obs, act = rec["obs_inter"].reshape(N, 10 * S), rec["action_inter"].reshape(N, S).to(torch.float32)
    mask = sorted_action_mask(rec["mask_inter"].reshape(N, S))
    logp0, adv0, vt0 = rec["logp"][..., 0].reshape(N), rec["adv"][..., 0].reshape(N), rec["vtarg"][..., 0].reshape(N)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for m, (pi, vf) in enumerate(zip(actors, critics)):
        opt = torch.optim.Adam(list(pi.parameters()) + list(vf.parameters()), lr=HP["lr"])
        lo, hi = int(first[m]), int(first[m + 1])
        for ep in range(EPOCHS):
            for c0 in range(lo, hi, MINIBATCH):
                idx = order[ep, c0:min(c0 + MINIBATCH, hi)].long()
                out = pi(obs[idx])
                mean, std = masked_gaussian_params(out[:, :S], out[:, S:], mask[idx])
                dist = torch.distributions.Normal(mean, std)
                logp, ent = dist.log_prob(act[idx]).sum(-1), (dist.entropy() * mask[idx]).sum(-1)
                adv = adv0[idx]
                adv = (adv - adv.mean()) / (adv.std() + 1e-8)
                ratio = torch.exp(logp - logp0[idx])
                surr = torch.minimum(ratio * adv, ratio.clamp(1.0 - HP["clip"], 1.0 + HP["clip"]) * adv)
                loss = -surr.mean() + HP["vf_coeff"] * (vf(obs[idx])[:, 0] - vt0[idx]).pow(2).mean() - HP["ent_coeff"] * ent.mean()
                opt.zero_grad(set_to_none=True)
                loss.backward()
                torch.nn.utils.clip_grad_norm_([p for g in opt.param_groups for p in g["params"]], HP["grad_clip"])
                opt.step()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def measure_update(repeats, members):
    import torch
    from intent_radio_sched_multi_slice_amd.adapters import ppo_row_order
    out = {}
    for name, widths in (("64x64", [64, 64]), ("256x256", [256, 256])):
        out[name] = {}
        for G in members:
            B = G * (ROWS // T)
            env = _workload(torch, B)
            S = env.S
            torch.manual_seed(G)
            actors = [_mlp(torch, [10 * S] + widths + [2 * S]).cuda() for _ in range(G)]
            critics = [_mlp(torch, [10 * S] + widths + [1]).cuda() for _ in range(G)]
            env.set_population(sizes=[B // G] * G)
            env.set_policy_network(actors, None, stochastic=True, seed=3)
            env.set_value_network(critics, None)
            env.ppo_bind()
            env.reset()
            rec = env.collect(T)
            order = ppo_row_order(rec, env.population(), EPOCHS, seed=1, intra=False)
            ms = []
            for _ in range(repeats + 1):              # (the first call also loads the kernel)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                env.ppo_update(rec, epochs=EPOCHS, minibatch=MINIBATCH, order=order, **HP)
                ms.append(1e3 * (time.perf_counter() - t0))
            t_torch = 1e3 * torch_loop(torch, rec, order["order_inter"], order["first_inter"], actors, critics, S)
            dev = statistics.median(ms[1:])
            out[name][str(G)] = {"device_ms": dev, "device_all_ms": ms, "torch_ms": t_torch, "speedup": t_torch / dev, "rows_per_member": ROWS,
                                 "optimiser_steps_per_member": EPOCHS * (ROWS // MINIBATCH)}
            print(name, G, out[name][str(G)], flush=True)
            env.close()
    return out


def measure_rollout(steps=200, blocks=5):
    import torch
    from intent_radio_sched_multi_slice_amd import _lib
    lib = __import__("ctypes").CDLL(_lib.LIB_PATH)
    for n in NEW_EXPORTS:                             # (a library without the new exports can run it)
        if not hasattr(lib, n):
            _lib.FUNCTIONS.pop(n, None)
    env = _workload(torch, 4096)
    S, W = env.S, env.W
    torch.manual_seed(0)
    env.set_policy_network(_mlp(torch, [10 * S, 64, 64, 2 * S]), _mlp(torch, [W, 64, 64, 3]), stochastic=True, seed=1)
    env.reset()
    env.rollout(steps)
    ms = []
    for _ in range(blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env.rollout(steps)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms)


def _child(lib):
    env = dict(os.environ)
    if lib:
        env["RANENV_LIB"] = os.path.abspath(lib)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-rollout"], env=env, check=True, capture_output=True, text=True, timeout=600)
    return json.loads(res.stdout.strip().split("\n")[-1])["rollout_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--members", default="1,8,64")
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--alternations", type=int, default=4)
    ap.add_argument("--child-rollout", action="store_true")
    args = ap.parse_args()
    if args.child_rollout:
        print(json.dumps({"rollout_ms": measure_rollout()}))
        return
    result = {"regime": {"rows_per_member": ROWS, "minibatch": MINIBATCH, "epochs": EPOCHS, "size": "S5_U25"}}
    if args.baseline_lib:
        base, new = [], []
        for _ in range(args.alternations):
            base.append(_child(args.baseline_lib))
            new.append(_child(None))
        result["rollout"] = {"baseline_ms": base, "this_ms": new, "ratio": statistics.median(new) / statistics.median(base),
                             "baseline_spread": max(base) / min(base) - 1.0}
    result["cases"] = measure_update(args.repeats, [int(x) for x in args.members.split(",")])
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
