"""The paper's per-slice evaluation figures (results/gen_results.py:236-259,550-625: violations per slice type, violations per slice
type and intent metric, the three network throughputs) for a whole batch of environments, without the host between two TTIs:

    python examples/evaluate_per_slice.py [--batch 1024] [--episodes 2] [--steps 200] [--policy inter.pt [--intra-policy intra.pt]]

MARR + round-robin and MAPF + proportional fairness -- and the IBSched nets of --policy (a state dict of an nn.Sequential, or an
RLlib FullyConnectedNetwork checkpoint) if given -- play the SAME episodes (one episode table, the same seeds), each in ONE
evaluate(per_slice=True): per-(env, slice) sums kept by a small kernel behind every step, appended per episode by the device's
auto-reset together with the scenario row the episode was played on, aggregated by slice type on the host
(scenario.slice_type_report).  Synthetic scenarios / channels of the reference's laws: the real datasets are not shipped.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from intent_radio_sched_multi_slice_amd import _lib, adapters
from intent_radio_sched_multi_slice_amd.scenario import SLICE_REPORT_METRICS, SLICE_TYPE_NAMES, slice_type_from_tables, slice_type_report
from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload


def load_layers(path):
    sd = torch.load(path, map_location="cpu")
    if any(k.startswith("internal_model.") for k in sd):
        return adapters.rllib_fcnet_layers(sd)
    n = sorted({int(k.split(".")[0]) for k in sd})
    return [(sd[f"{i}.weight"], sd[f"{i}.bias"]) for i in n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--episodes", type=int, default=2)
    ap.add_argument("--steps", type=int, default=200, help="TTIs per episode")
    ap.add_argument("--policy", help="weights of the IBSched inter-slice actor")
    ap.add_argument("--intra-policy", help="weights of the IBSched intra-slice actor (else proportional fairness)")
    ap.add_argument("--intra-input", default="obs", choices=("obs", "mask_obs"))
    ap.add_argument("--activation", default="tanh", choices=("tanh", "relu"))
    ap.add_argument("--priority-only", action="store_true", help="count priority slices only (calc_slice_violations(priority=True))")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, n_ep, T = args.batch, args.episodes, args.steps
    wl = make_mult_slice_workload(B, dev, policy=_lib.POLICY_MAPF, intra=_lib.INTRA_PF, n_scenarios=64, n_traces=64, trace_len=T, max_steps=T)
    env = wl.env
    eps = env.episodes
    env.set_episode_table(scenario=eps["scenario"], se_base=eps["se_base"], se_len=eps["se_len"], se_offset=eps["se_offset"],
                          trf_base=eps["trf_base"], trf_len=eps["trf_len"], trf_offset=eps["trf_offset"])
    slice_type = slice_type_from_tables(wl.tables)            # [n_scenarios, S]: which template sits at which slice index
    agents = [("MARR+RR", _lib.POLICY_MARR, _lib.INTRA_RR), ("MAPF+PF", _lib.POLICY_MAPF, _lib.INTRA_PF)]
    if args.policy:
        agents.append(("IBSched", None, None))
    reports = {}
    for name, policy, intra in agents:
        if policy is None:
            env.set_policy_network(load_layers(args.policy), load_layers(args.intra_policy) if args.intra_policy else None,
                                   intra_input=args.intra_input, activation=args.activation, fixed_intra=_lib.INTRA_PF)
        else:
            env.set_policy(policy, intra)
        env.enable_autoreset(0, B, episode_numbers=np.arange(B, dtype=np.int32))
        env.enable_metrics(n_ep)
        env.enable_slice_metrics()
        res = env.evaluate(n_ep, per_slice=True)
        reports[name] = slice_type_report(res["slice"], res["scenario"], slice_type, wl.tables, priority_only=args.priority_only)
        reports[name]["_ttis"] = float(res["ttis"].sum())
    env.close()

    names = list(reports)
    print(f"{B} envs x {n_ep} episodes of {T} TTIs (S {env.S}, U {env.U}); the same episodes for every agent"
          + (" -- priority slices only" if args.priority_only else ""))
    print("\nviolations_per_slice_type (slice-TTIs in violation)")
    print(f"{'slice type':<26}" + "".join(f"{n:>14}" for n in names))
    for t in SLICE_TYPE_NAMES:
        if any(t in reports[n]["violations_per_slice_type"] for n in names):
            print(f"{t:<26}" + "".join(f"{reports[n]['violations_per_slice_type'].get(t, 0):>14d}" for n in names))
    print("\nviolations_slice_metric (slice-TTIs in violation of one intent metric)")
    print(f"{'slice type / metric':<26}" + "".join(f"{n:>14}" for n in names))
    for t in SLICE_TYPE_NAMES:
        for m in SLICE_REPORT_METRICS:
            if any(m in reports[n]["violations_slice_metric"].get(t, {}) for n in names):
                print(f"{t + ' / ' + m:<26.26}" + "".join(f"{reports[n]['violations_slice_metric'].get(t, {}).get(m, 0):>14d}" for n in names))
    print("\nnetwork throughput, Mbit per env-TTI")
    for key in ("total_network_throughput", "total_network_eff_throughput", "total_network_requested_throughput"):
        print(f"{key:<36}" + "".join(f"{reports[n][key] / reports[n]['_ttis']:>14.3f}" for n in names))


if __name__ == "__main__":
    main()
