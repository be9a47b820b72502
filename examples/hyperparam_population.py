"""The trials of a hyper-parameter search as ONE mixed population: every member draws its own architecture and its own GAE discount
parameters from the reference's search space (agents/ray_agent.py: `net_arch` :61-67 and :135-145, `gamma` :112-126, `lambda` :128),
collects its PPO batch and is ranked beside the others -- one batch, one policy launch per TTI and agent kind:

    python examples/hyperparam_population.py --random [--members 10] [--envs-per-member 64] [--steps 200] [--seed 0]

Member m owns a contiguous block of envs (set_population) and acts with ITS nets: `set_policy_network(..., mixed=True)` /
`set_value_network(..., mixed=True)` take lists whose nets differ in depth and width.  `collect()` with sequences of gamma / lam
computes every member's advantages under its own pair.  The worst member is then replaced by a copy of the best through
`set_population_member` -- across architectures, PBT's exploit step -- where the best one's packed nets fit the worst one's extent
(every member's extent is the largest member's size, so they always do here).
--random: random weights -- no trial checkpoints are shipped; the ranking says nothing about learning, the plumbing is the point.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from intent_radio_sched_multi_slice_amd import _lib
from intent_radio_sched_multi_slice_amd.batched_env import packed_net_floats
from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload

# The reference's search space (agents/ray_agent.py:61-67, 112-126, 128)
NET_ARCH = {"small": [64, 64], "medium": [256, 256], "big": [400, 300], "large": [256, 256, 256], "verybig": [512, 512, 512]}
GAMMA = [0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.98, 0.99, 0.995, 0.999, 0.9999]
LAMBDA = [0.8, 0.9, 0.92, 0.95, 0.98, 0.99, 1.0]


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
    ap.add_argument("--random", action="store_true", help="random weights (required: no trial checkpoints are shipped)")
    ap.add_argument("--members", type=int, default=10, help="G: trials in the batch (<= 64)")
    ap.add_argument("--envs-per-member", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200, help="TTIs per episode and per collected batch")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not args.random:
        ap.error("give --random: no trial checkpoints are shipped")
    G, T = args.members, args.steps
    B = G * args.envs_per_member
    rng = np.random.default_rng(args.seed)
    trials = [{"arch": str(rng.choice(list(NET_ARCH))), "gamma": float(rng.choice(GAMMA)), "lam": float(rng.choice(LAMBDA))} for _ in range(G)]

    wl = make_mult_slice_workload(B, torch.device("cuda", 0), policy=_lib.POLICY_MAPF, intra=_lib.INTRA_PF, n_scenarios=8, n_traces=8, trace_len=T,
                                  max_steps=T)
    env = wl.env
    S, W = env.S, env.W

    def nets_of(m, seed):
        h = NET_ARCH[trials[m]["arch"]]
        return {"inter": random_net([10 * S] + h + [2 * S], seed), "intra": random_net([W] + h + [3], seed + 1),
                "v_inter": random_net([10 * S] + h + [1], seed + 2), "v_intra": random_net([W] + h + [1], seed + 3)}
    nets = [nets_of(m, 1000 + 10 * m) for m in range(G)]
    env.set_population(sizes=[args.envs_per_member] * G)
    env.set_policy_network([n["inter"] for n in nets], [n["intra"] for n in nets], stochastic=True, seed=args.seed, mixed=True)
    env.set_value_network([n["v_inter"] for n in nets], [n["v_intra"] for n in nets], mixed=True)

    # one PPO batch per trial, each under its own gamma / lambda
    env.reset()
    rec = env.collect(T, gamma=[t["gamma"] for t in trials], lam=[t["lam"] for t in trials])
    print(f"{G} trials x {args.envs_per_member} envs, one batch of {B} (S {S}, U {env.U}); collect({T}):")
    print(f"{'member':>6} {'net_arch':>18} {'gamma':>7} {'lambda':>6} {'floats':>8} | {'obs_inter':>16} {'adv':>16} {'mean reward':>12} {'mean adv':>10} {'mean vtarg':>10}")
    for m, sl in enumerate(env.population_slices()):
        info = env.population_net("inter", m)
        print(f"{m:>6} {str(info['hidden']):>18} {trials[m]['gamma']:>7} {trials[m]['lam']:>6} {info['used']:>8} | {str(tuple(rec['obs_inter'][:, sl].shape)):>16} "
              f"{str(tuple(rec['adv'][:, sl].shape)):>16} {rec['reward'][:, sl, 0].mean().item():>12.4f} {rec['adv'][:, sl, 0].mean().item():>10.4f} "
              f"{rec['vtarg'][:, sl, 0].mean().item():>10.4f}")

    # rank the trials by an evaluation episode, all in the same batch
    def evaluate():
        env.enable_autoreset(0, B, episode_numbers=np.arange(B, dtype=np.int32))
        env.enable_metrics(1)
        return env.evaluate_population(1)
    eps = env.episodes
    env.set_episode_table(**{k: eps[k] for k in ("scenario", "se_base", "se_len", "se_offset", "trf_base", "trf_len", "trf_offset")})
    res = evaluate()
    order = np.lexsort((res["violations"], -res["reward"]))
    print(f"\nevaluate_population(1): {'rank':>4} {'member':>6} {'net_arch':>10} {'reward/ep':>12} {'violations/ep':>14}")
    for r, m in enumerate(order):
        print(f"{'':>23} {r + 1:>4} {m:>6} {trials[m]['arch']:>10} {res['reward'][m]:>12.3f} {res['violations'][m]:>14.2f}")

    # PBT's exploit step: the worst member becomes a copy of the best, whatever the two architectures
    best, worst = int(order[0]), int(order[-1])
    extent = env.population_net("inter", worst)["extent"]
    assert packed_net_floats(nets[best]["inter"]) <= extent
    env.set_population_member(worst, **nets[best])
    trials[worst] = dict(trials[best])
    print(f"\nmember {worst} ({env.population_net('inter', worst)['hidden']}) is now a copy of member {best}; its extent holds {extent} floats, "
          f"the copy uses {env.population_net('inter', worst)['used']}")
    res = evaluate()
    print(f"after the copy: reward/ep of member {worst} {res['reward'][worst]:.3f}, of member {best} {res['reward'][best]:.3f}")
    env.close()


if __name__ == "__main__":
    main()
