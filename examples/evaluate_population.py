"""A population of IBSched agents evaluated in ONE batch, each member on its own scenario -- the test loop of the reference's
fine-tuned agents (simu.py:427-443: `finetune_*_sched_{n}`, one agent per scenario of env_config_scenarios["finetune_mult_slice_seq"]),
and what a hyper-parameter search ranks its trials by (agents/ray_agent.py:217-240):

    python examples/evaluate_population.py --random [--members 10] [--envs-per-member 64] [--episodes 2] [--steps 200]

Member m owns a contiguous block of envs, pinned to scenario m's episodes through enable_autoreset(episode_numbers=...), and acts with
its own inter / intra nets (set_population + set_policy_network with lists of G nets): one policy launch per TTI and agent kind for the
whole population.  MAPF + proportional fairness plays the same episodes beside it.  --random: nets of the reference's shape ([64, 64],
tanh) with random weights -- the real checkpoints are not shipped; the ranking then says nothing about learning, the plumbing is the point.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from intent_radio_sched_multi_slice_amd import _lib
from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload


def random_net(dims, seed):
    torch.manual_seed(seed)
    mods = []
    for i in range(len(dims) - 1):
        mods.append(torch.nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--random", action="store_true", help="random nets of the reference's shape (required: no checkpoints are shipped)")
    ap.add_argument("--members", type=int, default=10, help="G: agents = scenarios (the reference's number_scenarios is 10)")
    ap.add_argument("--envs-per-member", type=int, default=64)
    ap.add_argument("--episodes", type=int, default=2)
    ap.add_argument("--steps", type=int, default=200, help="TTIs per episode")
    args = ap.parse_args()
    if not args.random:
        ap.error("give --random: the fine-tuned agents' checkpoints are not shipped")
    G, n_ep, T = args.members, args.episodes, args.steps
    B = G * args.envs_per_member
    dev = torch.device("cuda", 0)
    wl = make_mult_slice_workload(B, dev, policy=_lib.POLICY_MAPF, intra=_lib.INTRA_PF, n_scenarios=G, n_traces=G, trace_len=T, max_steps=T)
    env = wl.env
    # A member-major episode table: rows m * n_ep .. m * n_ep + n_ep - 1 are scenario m on trace m, each at its own offsets.  Member m's
    # envs start at row m * n_ep and auto-reset advances by one row per episode: n_ep episodes, all of them on scenario m.
    member = np.repeat(np.arange(G), args.envs_per_member)
    k = np.arange(n_ep * G)
    env.set_episode_table(scenario=k // n_ep, se_base=(k // n_ep) * T, se_len=T, se_offset=(k * 7) % T, trf_base=(k // n_ep) * T, trf_len=T,
                          trf_offset=(k * 3) % T)
    env.set_population(sizes=[args.envs_per_member] * G)
    S, W = env.S, env.W
    inters = [random_net([10 * S, 64, 64, 2 * S], 100 + m) for m in range(G)]
    intras = [random_net([W, 64, 64, 3], 200 + m) for m in range(G)]

    def evaluate():
        env.enable_autoreset(0, n_ep * G, episode_numbers=(member * n_ep).astype(np.int32))
        env.enable_metrics(n_ep)
        return env.evaluate_population(n_ep)
    env.set_policy_network(inters, intras, stochastic=False)
    pop = evaluate()
    env.set_policy(_lib.POLICY_MAPF, _lib.INTRA_PF)
    mapf = evaluate()
    env.close()

    print(f"{G} members x {args.envs_per_member} envs x {n_ep} episodes of {T} TTIs (S {S}, U {env.U}); member m plays scenario m; one batch of {B}")
    print(f"{'rank':>4} {'member':>6} {'reward/ep':>12} {'violations/ep':>14} | {'MAPF reward/ep':>15} {'MAPF viol./ep':>14}")
    order = np.lexsort((pop["violations"], -pop["reward"]))
    for r, m in enumerate(order):
        print(f"{r + 1:>4} {m:>6} {pop['reward'][m]:>12.3f} {pop['violations'][m]:>14.2f} | {mapf['reward'][m]:>15.3f} {mapf['violations'][m]:>14.2f}")


if __name__ == "__main__":
    main()
