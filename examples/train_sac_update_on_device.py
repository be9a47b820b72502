"""SAC on SchedColORAN's head at SB3's settings with the whole learner on the device: collection, sampling and the gradient steps.

    python examples/train_sac_update_on_device.py [--batch 256] [--ttis 16] [--iters 10] [--grad-steps 16] [--capacity 64] [--slabs 32]
    python examples/train_sac_update_on_device.py --agent sb3_sched|sb3_pf_sched      (IBSchedSB3: obs_inter, reward[:, 0], RR / PF intra)

examples/train_sac_on_device.py keeps the losses, the three optimisers and the polyak loop in eager torch and therefore trains on
minibatches of 65 536 rows.  Here the learner is `env.sac_update` (ranenv_sac_update, include/ranenv.h "SAC update"), so the
minibatch is SB3's 256 and nothing crosses to the host between two gradient steps.  With SB3's defaults ([256, 256] relu, gamma 0.99,
tau 0.005, lr 3e-4, ent_coef "auto", target entropy -S), per iteration:

  1. `env.collect_replay(T)`: T TTIs of B envs under the head actor -- the buffer the update trains in place, so every iteration acts on
     the actor the previous one left, with no re-bind;
  2. ONE `env.replay_sample(steps * 256)`;
  3. ONE `env.sac_update(batch, steps)`: per step the soft Bellman target under the target critics, the critics' step, the actor's step
     under the new critics, the entropy coefficient's step and the polyak update -- four launches, no host in between.

`--grad-steps` is the caller's choice of gradient steps per iteration (SB3's `train_freq` / `gradient_steps` scheduling stays the
caller's loop).  An example of the API, not a tuned trainer: a freshly initialised actor plays the part of SB3's `learning_starts`
phase.  Prints the split of wall time between collection, sampling and the update, and the statistics of each iteration's last step.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from intent_radio_sched_multi_slice_amd._lib import INTRA_PF, INTRA_RR, POLICY_MAPF
from intent_radio_sched_multi_slice_amd.adapters import sb3_sac_state_dict
from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload

GAMMA, TAU, LR, MINIBATCH = 0.99, 0.005, 3e-4, 256


def mlp(n_in, n_out, width=256):
    return torch.nn.Sequential(torch.nn.Linear(n_in, width), torch.nn.ReLU(), torch.nn.Linear(width, width), torch.nn.ReLU(),
                               torch.nn.Linear(width, n_out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--ttis", type=int, default=16, help="TTIs per collect_replay() call")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--grad-steps", type=int, default=16, help="gradient steps of 256 rows per iteration")
    ap.add_argument("--capacity", type=int, default=64, help="slots (TTIs) of the replay ring: capacity x batch transitions")
    ap.add_argument("--slabs", type=int, default=32, help="gradient slabs: the most workgroups a pass spreads a minibatch's tiles over")
    ap.add_argument("--episode-len", type=int, default=100)
    ap.add_argument("--se-mode", choices=("stream", "gather"), default="gather")
    ap.add_argument("--agent", default="colran", choices=("colran", "sb3_sched", "sb3_pf_sched"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, T, L, G = args.batch, args.ttis, args.episode_len, args.grad_steps
    n_ep = 64
    wl = make_mult_slice_workload(B, dev, policy=POLICY_MAPF, intra=INTRA_RR, n_scenarios=n_ep, n_traces=n_ep, trace_len=L, max_steps=L)
    env = wl.env
    S = env.S
    inter = args.agent != "colran"
    if not inter:
        wl.tables.sorted_slices[...] = np.arange(S, dtype=np.int32)     # SchedColORAN runs with enable_sort_slices=False
        env.load_scenarios(wl.tables)
    env.set_se_mode(args.se_mode)
    if not inter:
        env.enable_heads(np.ones_like(wl.tables.slice_active, dtype=np.int32))
    observation, reward, col = ("inter", "ibsched", 0) if inter else ("head", "colran", 1)
    intra = INTRA_PF if args.agent == "sb3_pf_sched" else INTRA_RR
    ep = np.arange(n_ep)
    env.set_episode_table(scenario=ep, se_base=ep * L, se_len=L, trf_base=ep * L, trf_len=L)
    env.enable_autoreset(0, n_ep, random_episodes=True, seed=7, episode_numbers=np.arange(B) % n_ep)

    torch.manual_seed(0)
    actor, q1, q2 = mlp(10 * S, 2 * S), mlp(11 * S, 1), mlp(11 * S, 1)
    print(f"LDS of the update's passes for these nets: {env.sac_lds_bytes([10 * S, 256, 256, 2 * S], [11 * S, 256, 256, 1])} bytes")
    env.set_head_policy_network(actor, "gauss_tanh", stochastic=True, seed=1000, fixed_intra=intra, observation=observation)
    env.set_sac_critics(q1, q2)              # the targets; sac_bind starts the live critics as copies of them, as SB3 does
    env.sac_bind(ent_coef="auto", slabs=args.slabs)
    ring = env.bind_replay(args.capacity)
    env.reset()
    torch.cuda.synchronize()
    t_collect = t_sample = t_update = 0.0
    t0 = time.perf_counter()
    for it in range(args.iters):
        tc = time.perf_counter()
        env.collect_replay(T)
        torch.cuda.synchronize()
        ts = time.perf_counter()
        batch = env.replay_sample(G * MINIBATCH, seed=11, draw=it, reward=reward)
        torch.cuda.synchronize()
        tu = time.perf_counter()
        out = env.sac_update(batch, G, minibatch=MINIBATCH, lr=LR, gamma=GAMMA, tau=TAU, seed=13, draw=it)
        te = time.perf_counter()
        t_collect, t_sample, t_update = t_collect + ts - tc, t_sample + tu - ts, t_update + te - tu
        last = (env.replay_count() - 1) % args.capacity
        print(f"iteration {it + 1:3d}: mean {'SchedColORAN' if not inter else args.agent} reward of the last TTI {ring['reward_head'][last, :, col].mean().item():+.4f}, "
              f"alpha {out['ent_coef'][-1]:.3f}, critic loss {out['critic_loss'][-1]:.4f}, actor loss {out['actor_loss'][-1]:+.4f}, "
              f"mean log pi {out['logp_mean'][-1]:+.3f}", flush=True)
    dt = time.perf_counter() - t0
    n = B * T * args.iters
    print(f"{B} envs x {T} TTIs x {args.iters} iterations, {G} gradient steps of minibatch {MINIBATCH} each (SE mode {args.se_mode}): "
          f"{n / dt / 1e6:.3f} M env-steps/s with the updates included; collection {100 * t_collect / dt:.0f} % of the time, sampling "
          f"{100 * t_sample / dt:.0f} %, the update {100 * t_update / dt:.0f} % ({1e3 * t_update / (G * args.iters):.3f} ms per gradient step)")
    # the trained agent as an SB3 state dict (key names restated from SB3's module layout; parity with SB3 itself is unpinned)
    sd = sb3_sac_state_dict(*(env.sac_net_weights(k) for k in ("actor", "q1", "q2", "q1_target", "q2_target")), log_ent_coef=env.sac_log_ent_coef())
    print(f"state dict: {len(sd)} tensors, log_ent_coef {float(sd['log_ent_coef']):+.4f}")
    env.close()


if __name__ == "__main__":
    main()
