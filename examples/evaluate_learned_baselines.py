"""Evaluate a trained SchedTWC / SchedColORAN policy on the device beside MARR and MAPF on the same test episodes.

The reference's test loop (simu.py:547-566) for its two learned baselines -- SB3 PPO / SAC MlpPolicy agents on the head observation
(agents/sched_twc.py, agents/sched_colran.py) -- with the actor running on the GPU in front of every TTI
(BatchedRanEnv.set_head_policy_network, RANENV_POLICY_HEAD_NETWORK).  Every env plays --episodes episodes under each agent; printed
side by side: the paper's violation / distance metrics (results/gen_results.py:874-1022) and the mean episode reward of the agent's
own reward, the number SB3's EvalCallback selects best_model by (sched_twc.py:93-103) -- both kept by the device.

    python examples/evaluate_learned_baselines.py --random [--algo ppo|sac] [--reward twc|colran] [--batch 1024] [--episodes 2]
    python examples/evaluate_learned_baselines.py --weights ckpt.pt --algo ppo|sac --reward twc|colran [--stochastic]
    python examples/evaluate_learned_baselines.py --random --agent sb3_sched|sb3_pf_sched [--algo ppo|sac]

--weights: ``policy.state_dict()`` of an SB3 PPO / SAC MlpPolicy saved with torch.save (adapters.sb3_ppo_layers /
sb3_sac_actor_layers; the key names are restated from SB3's documented module layout, parity with SB3 itself is unpinned).
--random draws a net of SB3's default shape for the algorithm instead.  The scenario tables are built without slice sorting, as
SchedTWC runs IBSched (sched_twc.py:75-82).
--agent sb3_sched / sb3_pf_sched: the reference's IBSchedSB3 (agents/sb3_sched.py, agents/sb3_pf_sched.py) instead -- the same SB3
actor on IBSched's own player_0 observation (``observation="inter"``: obs_inter, sorted slices, no head outputs) with round-robin /
proportional fair inside the slices; its reward is the episode metrics' "reward" column, the number CustomEvalCallback ranks by.
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

DEFAULT_HIDDEN = {"ppo": ([64, 64], "tanh"), "sac": ([256, 256], "relu")}


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
    ap.add_argument("--algo", default="ppo", choices=("ppo", "sac"))
    ap.add_argument("--reward", default="twc", choices=("twc", "colran"))
    ap.add_argument("--agent", default=None, choices=("sb3_sched", "sb3_pf_sched"), help="IBSchedSB3 on obs_inter instead of a head agent")
    ap.add_argument("--random", action="store_true")
    ap.add_argument("--stochastic", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not args.random and not args.weights:
        ap.error("give --weights or --random")
    dev = torch.device("cuda", 0)
    B, n_ep = args.batch, args.episodes
    wl = make_mult_slice_workload(B, dev, policy=_lib.POLICY_MAPF, intra=_lib.INTRA_RR, n_scenarios=64, n_traces=64,
                                  trace_len=args.steps, max_steps=args.steps)
    env = wl.env
    inter = args.agent is not None
    if not inter:
        wl.tables.sorted_slices[...] = np.arange(env.S, dtype=np.int32)  # enable_sort_slices=False
        env.load_scenarios(wl.tables)
    # (the synthetic scenario pool carries no slice names: slices with a request are eMBB / URLLC by index parity here, so that both
    # terms of SchedColORAN's reward are live; with the reference's scenarios use scenario.slice_usecase_from_req)
    usecase = ((1 + np.arange(env.S) % 2)[None, :] * (wl.tables.slice_has_req != 0)).astype(np.int32)
    env.enable_heads(usecase)
    hidden, act = DEFAULT_HIDDEN[args.algo]
    S = env.S
    if args.algo == "ppo":
        if args.random:
            actor, log_std = random_layers([10 * S] + hidden + [S], args.seed), torch.zeros(S)
        else:
            actor, log_std, _ = adapters.sb3_ppo_layers(torch.load(args.weights, map_location="cpu"))
        dist = "gauss_clip"
    else:
        actor = random_layers([10 * S] + hidden + [2 * S], args.seed) if args.random else \
            adapters.sb3_sac_actor_layers(torch.load(args.weights, map_location="cpu"))
        log_std, dist = None, "gauss_tanh"
    # every env plays episodes e, e + 1, ... of one episode table: the same test episodes for every agent
    eps = env.episodes
    env.set_episode_table(scenario=eps["scenario"], se_base=eps["se_base"], se_len=eps["se_len"], se_offset=eps["se_offset"],
                          trf_base=eps["trf_base"], trf_len=eps["trf_len"], trf_offset=eps["trf_offset"])
    col = 0 if args.reward == "twc" else 1
    agent = f"{args.agent}-{args.algo}" if inter else f"Sched{'TWC' if col == 0 else 'ColORAN'}-{args.algo}"
    intra = _lib.INTRA_PF if args.agent == "sb3_pf_sched" else _lib.INTRA_RR
    results = {}
    for name in (agent, "MARR", "MAPF"):
        if name == agent:
            env.set_head_policy_network(actor, dist, log_std, stochastic=args.stochastic, seed=args.seed, activation=act,
                                        fixed_intra=intra, observation="inter" if inter else "head")
        else:
            env.set_policy(_lib.POLICY_MARR if name == "MARR" else _lib.POLICY_MAPF, intra)
        env.enable_autoreset(0, B, episode_numbers=np.arange(B, dtype=np.int32))
        env.enable_metrics(n_ep)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        results[name] = env.evaluate(n_ep)
        t1.record()
        torch.cuda.synchronize()
        results[name]["_s"] = t0.elapsed_time(t1) * 1e-3
        results[name]["_head"] = results[name]["reward"] if inter else env.head_episode_metrics()["episode_log"][:, :n_ep, col].cpu().numpy()
    print(f"{B} envs x {n_ep} episodes of {args.steps} TTIs (S {env.S}, U {env.U}); per-TTI means over all episodes")
    print(f"{'metric':<28}" + "".join(f"{n:>18}" for n in results))
    for m in ("reward", "violations", "priority_violations", "distance", "priority_distance", "pkts_sent", "pkts_dropped"):
        print(f"{m:<28}" + "".join(f"{float(np.mean(r[m] / r['ttis'])):>18.4f}" for r in results.values()))
    print(f"{'mean episode ' + ('ibsched' if inter else args.reward) + ' reward':<28}" + "".join(f"{float(np.mean(r['_head'])):>18.4f}" for r in results.values()))
    print(f"{'env-steps/s':<28}" + "".join(f"{B * n_ep * args.steps / r['_s']:>18.3g}" for r in results.values()))
    env.close()


if __name__ == "__main__":
    main()
