"""Which episodes of a table are heavy, which are light, and which cannot be served at all -- before a single environment step:

    python examples/scenario_load.py [--episodes 256] [--steps 200] [--show 3]

The reference answers this with plot_rbs_needed_network_scenarios (results/gen_results.py:1251-1451): per episode the mean, over
its TTIs, of the RBs the network would need to serve every slice's requested traffic at the slices' mean spectral efficiency; it
plots the heaviest, the median and the lightest scenario.  It reads spectral_efficiencies from history files, i.e. needs a recorded
run per scenario.  The figures do not depend on the agent: here they come from one streaming pass over the SE pool in HBM
(BatchedRanEnv.se_tile_stats: mean / std / min / max per UE and tile) and one small kernel over the episode table
(BatchedRanEnv.scenario_load), picked by scenario.rank_by_load exactly as the reference picks them.  An episode that needs more
than R RBs on average cannot have its intents met by any agent.  Synthetic scenarios / channels of the reference's laws: the real
datasets are not shipped.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from intent_radio_sched_multi_slice_amd.scenario import rank_by_load
from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200, help="TTIs per episode")
    ap.add_argument("--show", type=int, default=3, help="slices printed per picked episode (the most demanding ones)")
    args = ap.parse_args()
    n, T = args.episodes, args.steps
    wl = make_mult_slice_workload(n, torch.device("cuda", 0), n_scenarios=64, n_traces=64, trace_len=T, max_steps=T)
    env = wl.env
    eps = env.episodes
    env.set_episode_table(scenario=eps["scenario"], se_base=eps["se_base"], se_len=eps["se_len"], se_offset=eps["se_offset"],
                          trf_base=eps["trf_base"], trf_len=eps["trf_len"], trf_offset=eps["trf_offset"])
    stats = env.se_tile_stats()                                   # [tiles, 4, U]: built here, one pass over the pool
    load = env.scenario_load(per_step=True)                       # the bound table, max_steps TTIs each
    total = load["episode_mean"].cpu().numpy()                    # [n, 3]: avg / min / max needed RBs of the network
    per_slice = load["per_step_slice"].mean(dim=1).cpu().numpy()  # [n, S, 6], averaged over the TTIs for printing
    heavy, median, light = rank_by_load(total[:, 0])
    print(f"{n} episodes of {T} TTIs (S {env.S}, U {env.U}, R {env.R}); statistics of {stats.shape[0]} tiles")
    print(f"episodes needing more than R = {env.R} RBs on average: {int((total[:, 0] > env.R).sum())} of {n}"
          f" (even at mean + std of the SE: {int((total[:, 1] > env.R).sum())})")
    for tag, i in (("heaviest", heavy), ("median", median), ("lightest", light)):
        e = eps[i]
        print(f"\n{tag}: episode {i} (scenario row {int(e['scenario'])}, trace at tile {int(e['se_base'])}): "
              f"{total[i, 0]:.1f} RBs on average (between {total[i, 1]:.1f} and {total[i, 2]:.1f})")
        order = np.argsort(-per_slice[i, :, 0])[:args.show]
        for s in order:
            members = int((wl.tables.ue_slice[int(e["scenario"])] == s).sum())
            print(f"  slice {int(s)}: {members} UEs x {wl.tables.slice_traffic[int(e['scenario']), s]:.0f} Mbps need {per_slice[i, s, 0]:.1f} RBs"
                  f" at {per_slice[i, s, 3]:.2f} Mbps per RB")
    env.close()


if __name__ == "__main__":
    main()
