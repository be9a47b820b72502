"""SAC in miniature on SchedColORAN's head with the host out of the data path: replay ring, minibatches and Bellman targets on the GPU.

    python examples/train_sac_on_device.py [--batch 4096] [--ttis 16] [--iters 10] [--grad-steps 8] [--minibatch 65536] [--capacity 64]
    python examples/train_sac_on_device.py --agent sb3_sched|sb3_pf_sched      (IBSchedSB3: obs_inter, reward[:, 0], RR / PF intra)

The reference builds its SB3 agents in a "sac" flavour beside "ppo" (agents/sched_colran.py:111-133, agents/sched_twc.py:111-133,
agents/sb3_sched.py:104-120): SB3's SAC("MlpPolicy", ...) -- an actor with a tanh-squashed Gaussian, two Q-nets and their polyak-averaged
targets, a replay buffer, an automatically tuned entropy coefficient.  Here, with SB3's defaults where they fit ([256, 256] relu, gamma
0.99, tau 0.005, lr 3e-4, target entropy -S), per iteration:

  1. `env.collect_replay(T)`: T TTIs of B envs under the actor ON THE DEVICE; every transition (obs, consumed action, both head rewards,
     done, next_obs -- the terminal observation where an episode ended) goes to the replay ring in HBM;
  2. `--grad-steps` gradient steps: `env.replay_sample(n)` draws a uniform minibatch, `env.sac_targets(...)` computes
     r + gamma (1 - d) (min(Q1', Q2')(s', a') - alpha log pi(a'|s')) under the bound actor and TARGET critics -- one actor and two critic
     forwards per row, on the device's matrix cores -- then the critic, actor and alpha losses and the polyak update in eager torch;
  3. `set_head_policy_network` / `set_sac_critics` with the new weights.

An example of the API, not a tuned trainer: a freshly initialised actor plays the part of SB3's `learning_starts` phase of uniform random
actions, the actor and target critics that the device uses are those of the iteration's start (SB3 refreshes them every gradient step),
and minibatches are far larger than SB3's 256 so that the torch side does not drown the measurement in tiny kernels.  Prints the split of
wall time between collection, sample + targets, and torch, and the mean SchedColORAN reward per iteration.
"""
import argparse
import copy
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from intent_radio_sched_multi_slice_amd._lib import INTRA_PF, INTRA_RR, POLICY_MAPF
from intent_radio_sched_multi_slice_amd.adapters import sac_targets_torch
from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload

GAMMA, TAU, LR = 0.99, 0.005, 3e-4
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
HALF_LN_2PI = 0.5 * math.log(2.0 * math.pi)


def mlp(n_in, n_out, width=256):
    return torch.nn.Sequential(torch.nn.Linear(n_in, width), torch.nn.ReLU(), torch.nn.Linear(width, width), torch.nn.ReLU(),
                               torch.nn.Linear(width, n_out))


def sample_action(actor, obs, S):
    """a ~ pi(.|obs) by the reparameterisation trick and its log-probability (SB3's SquashedDiagGaussianDistribution)."""
    out = actor(obs)
    mu, ls = out[:, :S], out[:, S:].clamp(LOG_STD_MIN, LOG_STD_MAX)
    z = torch.randn_like(mu)
    a = torch.tanh(mu + torch.exp(ls) * z)
    logp = (-0.5 * z * z - ls - HALF_LN_2PI).sum(-1) - torch.log(1.0 - a * a + 1e-6).sum(-1)
    return a, logp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--ttis", type=int, default=16, help="TTIs per collect_replay() call")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--grad-steps", type=int, default=8)
    ap.add_argument("--minibatch", type=int, default=65536)
    ap.add_argument("--capacity", type=int, default=64, help="slots (TTIs) of the replay ring: capacity x batch transitions")
    ap.add_argument("--episode-len", type=int, default=100)
    ap.add_argument("--check", action="store_true", help="compare the first minibatch's targets with adapters.sac_targets_torch")
    ap.add_argument("--se-mode", choices=("stream", "gather"), default="gather")
    ap.add_argument("--agent", default="colran", choices=("colran", "sb3_sched", "sb3_pf_sched"),
                    help="colran: SchedColORAN's head; sb3_sched / sb3_pf_sched: the reference's IBSchedSB3 on IBSched's player_0 observation "
                         "and reward (agents/sb3_sched.py, agents/sb3_pf_sched.py), round-robin / proportional fair inside the slices")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, T, L, G, N = args.batch, args.ttis, args.episode_len, args.grad_steps, args.minibatch
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
    actor, q1, q2 = mlp(10 * S, 2 * S).to(dev), mlp(11 * S, 1).to(dev), mlp(11 * S, 1).to(dev)
    q1_t, q2_t = copy.deepcopy(q1), copy.deepcopy(q2)
    log_alpha = torch.zeros((), device=dev, requires_grad=True)          # SB3: ent_coef "auto" starts at 1
    q_params = list(q1.parameters()) + list(q2.parameters())
    opt_actor, opt_q, opt_alpha = (torch.optim.Adam(p, lr=LR) for p in (actor.parameters(), q_params, [log_alpha]))
    target_entropy = -float(S)

    def bind(it):
        env.set_head_policy_network(actor, "gauss_tanh", stochastic=True, seed=1000 + it, fixed_intra=intra, observation=observation)
        env.set_sac_critics(q1_t, q2_t)

    bind(0)                                  # (first: choosing the observation source unbinds a ring)
    ring = env.bind_replay(args.capacity)
    env.reset()
    torch.cuda.synchronize()
    t_collect = t_device = 0.0
    t0 = time.perf_counter()
    for it in range(args.iters):
        tc = time.perf_counter()
        env.collect_replay(T)
        torch.cuda.synchronize()
        t_collect += time.perf_counter() - tc
        for g in range(G):
            draw = it * G + g
            td = time.perf_counter()
            mb = env.replay_sample(N, seed=11, draw=draw, reward=reward)
            alpha = float(log_alpha.exp())
            target = env.sac_targets(mb["next_obs"], mb["reward"], mb["done"], gamma=GAMMA, ent_coef=alpha, stochastic=True, seed=13, draw=draw,
                                     outputs=("target",))["target"]
            torch.cuda.synchronize()
            t_device += time.perf_counter() - td
            if args.check and draw == 0:        # the normative float32 restatement of the same rows, in eager torch
                want = sac_targets_torch(mb["next_obs"], mb["reward"], mb["done"], actor, q1_t, q2_t, GAMMA, alpha, True, 13, draw, device=dev)
                print(f"first minibatch: largest |device target - torch restatement| {(target.cpu() - want['target']).abs().max().item():.3g}")
            obs, act = mb["obs"], mb["action"]
            # critics: both regress on the same target
            xa = torch.cat([obs, act], dim=1)
            loss_q = 0.5 * ((q1(xa)[:, 0] - target).pow(2).mean() + (q2(xa)[:, 0] - target).pow(2).mean())
            opt_q.zero_grad(set_to_none=True)
            loss_q.backward()
            opt_q.step()
            # actor and the entropy coefficient
            a, logp = sample_action(actor, obs, S)
            loss_alpha = -(log_alpha * (logp.detach() + target_entropy)).mean()
            opt_alpha.zero_grad(set_to_none=True)
            loss_alpha.backward()
            opt_alpha.step()
            xa = torch.cat([obs, a], dim=1)
            loss_pi = (alpha * logp - torch.minimum(q1(xa)[:, 0], q2(xa)[:, 0])).mean()
            opt_actor.zero_grad(set_to_none=True)
            loss_pi.backward()
            opt_actor.step()
            with torch.no_grad():           # polyak update of the target critics
                for net, tgt in ((q1, q1_t), (q2, q2_t)):
                    for p, pt in zip(net.parameters(), tgt.parameters()):
                        pt.mul_(1.0 - TAU).add_(p, alpha=TAU)
        bind(it + 1)
        last = (env.replay_count() - 1) % args.capacity
        print(f"iteration {it + 1:3d}: mean {'SchedColORAN' if not inter else args.agent} reward of the last TTI {ring['reward_head'][last, :, col].mean().item():+.4f}, "
              f"alpha {float(log_alpha.exp()):.3f}, critic loss {loss_q.item():.4f}", flush=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n = B * T * args.iters
    t_torch = dt - t_collect - t_device
    print(f"{B} envs x {T} TTIs x {args.iters} iterations, {G} gradient steps of minibatch {N} each (SE mode {args.se_mode}): "
          f"{n / dt / 1e6:.2f} M env-steps/s with the updates included; collection {n / t_collect / 1e6:.2f} M env-steps/s "
          f"({100 * t_collect / dt:.0f} % of the time), sample + targets {100 * t_device / dt:.0f} %, torch {100 * t_torch / dt:.0f} %")
    env.close()


if __name__ == "__main__":
    main()
