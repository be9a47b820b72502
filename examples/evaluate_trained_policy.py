"""Evaluate a trained IBSched policy pair on the device against the MARR / MAPF baselines on the same test episodes.

The reference's test loop (simu.py:547-566) for a trained agent, here with the policy nets running on the GPU in front of every
TTI (BatchedRanEnv.set_policy_network, RANENV_POLICY_NETWORK): every env plays --episodes episodes under each agent, and the
paper's violation / distance metrics (results/gen_results.py:874-1022, kept by the device) are printed side by side.

    python examples/evaluate_trained_policy.py --random [--batch 1024] [--episodes 2] [--steps 200]
    python examples/evaluate_trained_policy.py --weights ckpt.pt [--intra-weights intra.pt] [--intra-input mask_obs] [--stochastic]
    python examples/evaluate_trained_policy.py --random --hidden 512,512,512 --precision both [--json]

--weights / --intra-weights: a torch state dict of an RLlib FullyConnectedNetwork (keys internal_model._hidden_layers.{i}._model.0.*,
internal_model._logits._model.0.*; adapters.rllib_fcnet_layers) or of a torch.nn.Sequential of Linear + Tanh (keys {i}.weight /
{i}.bias).  --random draws nets of --hidden widths instead.  Without intra weights the slices schedule with --fixed-intra.
--precision bf16 runs the nets on the bf16 matrix cores (set_policy_network(precision="bf16"): weights, inputs and hidden
activations rounded to bf16, include/ranenv.h); "both" evaluates the same episodes under the f32 and the bf16 nets and prints the
metrics side by side with their largest relative difference -- how far the episode figures move.  With --random nets that says how
sensitive these episodes are to a perturbation of the actions in the third digit, not how a trained policy behaves.
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from intent_radio_sched_multi_slice_amd import _lib, adapters  # noqa: E402
from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload  # noqa: E402

INTRA = {"rr": _lib.INTRA_RR, "pf": _lib.INTRA_PF, "mt": _lib.INTRA_MT}


def load_layers(path):
    sd = torch.load(path, map_location="cpu")
    if any(k.startswith("internal_model.") for k in sd):
        return adapters.rllib_fcnet_layers(sd)
    n = sorted({int(k.split(".")[0]) for k in sd})
    return [(sd[f"{i}.weight"], sd[f"{i}.bias"]) for i in n]


def random_layers(dims, seed):
    torch.manual_seed(seed)
    lins = [torch.nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:])]
    return [(m.weight.detach(), m.bias.detach()) for m in lins]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--episodes", type=int, default=2)
    ap.add_argument("--steps", type=int, default=200, help="TTIs per episode")
    ap.add_argument("--weights")
    ap.add_argument("--intra-weights")
    ap.add_argument("--intra-input", default="obs", choices=("obs", "mask_obs"))
    ap.add_argument("--activation", default="tanh", choices=("tanh", "relu"))
    ap.add_argument("--random", action="store_true")
    ap.add_argument("--hidden", default="256,256")
    ap.add_argument("--fixed-intra", default="pf", choices=sorted(INTRA))
    ap.add_argument("--stochastic", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--precision", default="f32", choices=("f32", "bf16", "both"))
    ap.add_argument("--json", action="store_true", help="also print one JSON line: per agent the per-TTI means, and the f32 / bf16 difference")
    args = ap.parse_args()
    if not args.random and not args.weights:
        ap.error("give --weights or --random")
    dev = torch.device("cuda", 0)
    B, n_ep = args.batch, args.episodes
    wl = make_mult_slice_workload(B, dev, policy=_lib.POLICY_MAPF, intra=INTRA[args.fixed_intra], n_scenarios=64, n_traces=64,
                                  trace_len=args.steps, max_steps=args.steps)
    env = wl.env
    hidden = [int(x) for x in args.hidden.split(",")]
    n_in_intra = env.net_input_dims(args.intra_input)[1]
    if args.random:
        inter = random_layers([10 * env.S] + hidden + [2 * env.S], args.seed)
        intra = random_layers([n_in_intra] + hidden + [3], args.seed + 1)
    else:
        inter = load_layers(args.weights)
        intra = load_layers(args.intra_weights) if args.intra_weights else None
    # every env plays episodes e, e + 1, ... of one episode table: the same test episodes for every agent
    eps = env.episodes
    env.set_episode_table(scenario=eps["scenario"], se_base=eps["se_base"], se_len=eps["se_len"], se_offset=eps["se_offset"],
                          trf_base=eps["trf_base"], trf_len=eps["trf_len"], trf_offset=eps["trf_offset"])
    results = {}
    precisions = ("f32", "bf16") if args.precision == "both" else (args.precision,)
    for name in tuple(f"network {p}" for p in precisions) + ("MARR", "MAPF"):
        if name.startswith("network"):
            env.set_policy_network(inter, intra, stochastic=args.stochastic, seed=args.seed, intra_input=args.intra_input,
                                   activation=args.activation, fixed_intra=INTRA[args.fixed_intra], precision=name.split()[1])
        else:
            env.set_policy(_lib.POLICY_MARR if name == "MARR" else _lib.POLICY_MAPF, INTRA[args.fixed_intra])
        env.enable_autoreset(0, B, episode_numbers=np.arange(B, dtype=np.int32))
        env.enable_metrics(n_ep)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        results[name] = env.evaluate(n_ep)
        t1.record()
        torch.cuda.synchronize()
        results[name]["_s"] = t0.elapsed_time(t1) * 1e-3
    print(f"{B} envs x {n_ep} episodes of {args.steps} TTIs (S {env.S}, U {env.U}); per-TTI means over all episodes")
    print(f"{'metric':<22}" + "".join(f"{n:>14}" for n in results))
    metrics = [m for m in env.METRIC_NAMES if m != "ttis"]
    means = {n: {m: float(np.mean(r[m] / r["ttis"])) for m in metrics} | {"ttis": float(np.mean(r["ttis"]))} for n, r in results.items()}
    for m in metrics:
        print(f"{m:<22}" + "".join(f"{means[n][m]:>14.4f}" for n in results))
    print(f"{'env-steps/s':<22}" + "".join(f"{B * n_ep * args.steps / r['_s']:>14.3g}" for r in results.values()))
    diff = None
    if args.precision == "both":
        a, b = means["network f32"], means["network bf16"]
        diff = {m: abs(a[m] - b[m]) / max(abs(a[m]), 1e-300) for m in a}
        worst = max(diff, key=diff.get)
        print(f"f32 -> bf16: largest relative difference of the {len(diff)} episode metrics {diff[worst]:.3g} ({worst})")
    if args.json:
        import json
        print(json.dumps({"batch": B, "episodes": n_ep, "steps": args.steps, "hidden": hidden, "activation": args.activation,
                          "stochastic": args.stochastic, "means": means, "relative_difference": diff,
                          "env_steps_per_s": {n: B * n_ep * args.steps / r["_s"] for n, r in results.items()}}))
    env.close()


if __name__ == "__main__":
    main()
