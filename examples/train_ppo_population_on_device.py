"""A PPO hyper-parameter search with BOTH halves on the device: G trials share one batch, `collect()` records every trial's rollout
and `ppo_update()` runs every trial's SGD schedule in one launch -- one workgroup per trial and agent kind.

    python examples/train_ppo_population_on_device.py [--trials 64] [--batch 4096] [--ttis 32] [--iters 5]

The reference searches over lr, sgd_minibatch_size, num_sgd_iter, clip_param, entropy_coeff, vf_loss_coeff, grad_clip, gamma and
lambda with nets of [64, 64] (agents/ray_agent.py:70-146,154-166); a trial's train batch is `batch / trials x ttis` env-steps -- 2048
at the defaults, the reference's train_batch_size.  Here per iteration:

  1. `env.collect(T, gamma=[...], lam=[...])`: every trial's rollout under its own nets, GAE with its own (gamma, lambda);
  2. `env.ppo_update(rec, epochs=[...], minibatch=[...], lr=[...], ...)`: every trial's epochs x minibatches of clipped-surrogate
     loss, gradient clip and Adam, in place in the weights the next `collect()` acts on -- no rebind, no host between the steps;
  3. the trials are ranked by the mean inter-slice reward of their own envs.

An example of the API, not a tuned search.  Prints env-steps/s with the updates included, the share of the update in it, and the ranking.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from intent_radio_sched_multi_slice_amd._lib import INTRA_PF, POLICY_MAPF
from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload


def mlp(n_in, n_out, width=64):
    return torch.nn.Sequential(torch.nn.Linear(n_in, width), torch.nn.Tanh(), torch.nn.Linear(width, width), torch.nn.Tanh(),
                               torch.nn.Linear(width, n_out))


def draw_trials(G, rng):
    """G points of the reference's search space (agents/ray_agent.py:90-134)"""
    return {"lr": np.exp(rng.uniform(np.log(5e-6), np.log(1e-4), G)), "minibatch": rng.choice([8, 16, 32, 64, 128, 256, 512], G),
            "epochs": rng.choice([1, 5, 10, 20], G), "clip": rng.choice([0.1, 0.2, 0.3, 0.4], G),
            "ent_coeff": np.exp(rng.uniform(np.log(1e-8), np.log(0.1), G)), "vf_coeff": rng.uniform(0.0, 1.0, G),
            "grad_clip": rng.choice([0.3, 0.5, 0.6, 0.7, 0.8, 0.9, 1, 2, 5], G).astype(np.float64),
            "gamma": rng.choice([0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.98, 0.99, 0.995, 0.999, 0.9999], G),
            "lam": rng.choice([0.8, 0.9, 0.92, 0.95, 0.98, 0.99, 1.0], G)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--ttis", type=int, default=32, help="TTIs per collect(): a trial's train batch is batch / trials x ttis env-steps")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--episode-len", type=int, default=100)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, T, G, L = args.batch, args.ttis, args.trials, args.episode_len
    n_ep = 64
    wl = make_mult_slice_workload(B, dev, policy=POLICY_MAPF, intra=INTRA_PF, n_scenarios=n_ep, n_traces=n_ep, trace_len=L, max_steps=L)
    env = wl.env
    S, W = env.S, env.W
    env.set_se_mode("gather")
    ep = np.arange(n_ep)
    env.set_episode_table(scenario=ep, se_base=ep * L, se_len=L, trf_base=ep * L, trf_len=L)
    env.enable_autoreset(0, n_ep, random_episodes=True, seed=7, episode_numbers=np.arange(B) % n_ep)

    torch.manual_seed(0)
    trials = draw_trials(G, np.random.default_rng(0))
    nets = {"inter": [mlp(10 * S, 2 * S) for _ in range(G)], "intra": [mlp(W, 3) for _ in range(G)],
            "v_inter": [mlp(10 * S, 1) for _ in range(G)], "v_intra": [mlp(W, 1) for _ in range(G)]}
    with torch.no_grad():
        for net in nets["inter"]:
            net[-1].bias[S:].fill_(-0.5)      # initial log_std
    env.set_population(sizes=[B // G] * (G - 1) + [B - (G - 1) * (B // G)])
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=1000)
    env.set_value_network(nets["v_inter"], nets["v_intra"])
    env.ppo_bind()
    env.reset()
    torch.cuda.synchronize()
    members = env.population_slices()
    t_update, t0 = 0.0, time.perf_counter()
    for it in range(args.iters):
        rec = env.collect(T, gamma=trials["gamma"], lam=trials["lam"])
        torch.cuda.synchronize()
        tu = time.perf_counter()
        stats = env.ppo_update(rec, epochs=trials["epochs"], minibatch=trials["minibatch"], lr=trials["lr"], clip=trials["clip"],
                               vf_coeff=trials["vf_coeff"], ent_coeff=trials["ent_coeff"], grad_clip=trials["grad_clip"], seed=it)
        t_update += time.perf_counter() - tu
        reward = np.array([float(rec["reward"][:, sl, 0].mean()) for sl in members])
        best = int(np.argmax(reward))
        last = np.maximum(trials["epochs"] - 1, 0)
        print(f"iter {it}: mean inter reward over the trials {reward.mean():+.4f}, best trial {best} ({reward[best]:+.4f}); "
              f"its last epoch: policy loss {stats['policy_loss'][best, 0, last[best]]:+.4f}, KL {stats['kl'][best, 0, last[best]]:+.2e}, "
              f"clip fraction {stats['clip_frac'][best, 0, last[best]]:.3f}")
    dt = time.perf_counter() - t0
    print(f"{args.iters * B * T / dt:,.0f} env-steps/s with the updates included; the updates took {100 * t_update / dt:.0f} % of the time")
    order = np.argsort(-reward)
    for m in order[:5]:
        print(f"  trial {m}: reward {reward[m]:+.4f}  " + "  ".join(f"{k} {trials[k][m]:.3g}" for k in trials))
    export = env.net_weights("inter", int(order[0]))      # the winner's trained inter actor, as (W, b) pairs
    print(f"winner's inter actor: {[tuple(w.shape) for w, _ in export]}")
    env.close()


if __name__ == "__main__":
    main()
