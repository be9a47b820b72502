"""Train the reference's SB3 PPO("MlpPolicy") agents with collection AND the SGD on the device: the host touches it once per batch.

    python examples/train_sb3_ppo_on_device.py --agent twc|colran|ibsched [--batch 64] [--episode-len 32] [--iters 5] [--out policy.pt] [--device-order]
    python examples/train_sb3_ppo_on_device.py --agent twc --spread 64 --batch 4096 --episode-len 64 --epochs 4 --minibatch 8192

--agent twc / colran: SchedTWC / SchedColORAN on the head observation (agents/sched_twc.py:111-118, agents/sched_colran.py), scenario
tables without slice sorting; --agent ibsched: IBSchedSB3 on player_0's row of obs_inter (agents/sb3_sched.py:104-111), round-robin inside
the slices.  Per iteration:

  1. `env.collect_head(T)`: T = one episode of B envs under the actor ON THE DEVICE; observations, sampled actions, log-probabilities,
     values, rewards, GAE advantages and value targets stay in HBM;
  2. `env.ppo_update_head(rec)`: SB3's PPO.train -- 10 epochs of minibatch 64, clip 0.2, vf 0.5, ent 0.0, max_grad_norm 0.5, Adam 3e-4
     eps 1e-5, per-minibatch advantage normalisation, the state-independent log_std trained with the nets -- in ONE launch of one
     workgroup, in place: the next collect_head acts on the trained policy with no rebind.

Printed per iteration: the mean episode reward of the agent's own reward from the device-side episode sums, and the update's statistics.
The default batch is SB3's: n_steps 2048 rows per update (64 envs x 32 TTIs).  At the end the trained policy is written as an SB3
state dict (adapters.sb3_ppo_state_dict; key names restated from SB3's documented module layout, parity with SB3 itself is unpinned).

--spread [SLABS] (default 64 slabs): the head binding's spread form, `env.ppo_bind(head=True, spread=True, slabs=SLABS)` -- every
optimiser step of `ppo_update_head` runs as three launches spread over up to SLABS workgroups, for batches one workgroup cannot digest:
the second command line trains on 262 144 rows per update (4096 envs x 64 TTIs), which the plain head binding refuses (more than 2^20
rows x epochs) and the spread one takes; `ppo_head_spread_bytes` tells what the slabs cost.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from intent_radio_sched_multi_slice_amd import _lib, adapters  # noqa: E402
from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload  # noqa: E402


def layers(dims, seed):
    torch.manual_seed(seed)
    return [(m.weight.detach(), m.bias.detach()) for m in (torch.nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:]))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agent", default="twc", choices=("twc", "colran", "ibsched"))
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--episode-len", type=int, default=32, help="TTIs per episode = TTIs per collect_head call")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--minibatch", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--spread", type=int, nargs="?", const=64, default=None, metavar="SLABS",
                    help="the spread head binding: every optimiser step over up to SLABS (1..256, default 64) workgroups")
    ap.add_argument("--device-order", action="store_true", help='draw the row lists on the device: ppo_update_head(..., order="device")')
    ap.add_argument("--out", default="sb3_ppo_policy.pt")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, L = args.batch, args.episode_len
    wl = make_mult_slice_workload(B, dev, policy=_lib.POLICY_MAPF, intra=_lib.INTRA_RR, n_scenarios=64, n_traces=64, trace_len=L, max_steps=L)
    env = wl.env
    S, inter = env.S, args.agent == "ibsched"
    if not inter:
        wl.tables.sorted_slices[...] = np.arange(S, dtype=np.int32)      # enable_sort_slices=False (sched_twc.py:75-82)
        env.load_scenarios(wl.tables)
        env.enable_heads(((1 + np.arange(S) % 2)[None, :] * (wl.tables.slice_has_req != 0)).astype(np.int32))
    eps = env.episodes
    env.set_episode_table(scenario=eps["scenario"], se_base=eps["se_base"], se_len=eps["se_len"], se_offset=eps["se_offset"],
                          trf_base=eps["trf_base"], trf_len=eps["trf_len"], trf_offset=eps["trf_offset"])
    env.enable_autoreset(0, B, random_episodes=True, seed=args.seed, episode_numbers=np.arange(B, dtype=np.int32))
    env.set_head_policy_network(layers([10 * S, 64, 64, S], args.seed), "gauss_clip", torch.zeros(S), stochastic=True, seed=args.seed,
                                activation="tanh", observation="inter" if inter else "head")
    env.set_head_value_network(layers([10 * S, 64, 64, 1], args.seed + 1), activation="tanh")
    if args.spread is None:
        env.ppo_bind(head=True)
    else:
        from intent_radio_sched_multi_slice_amd.batched_env import ppo_head_spread_bytes
        env.ppo_bind(head=True, spread=True, slabs=args.spread)
        kib = ppo_head_spread_bytes([10 * S, 64, 64, S], [10 * S, 64, 64, 1], S, args.spread) / 1024
        print(f"spread head binding: {args.spread} slabs, {kib:.0f} KiB of gradient slabs; {B * L} rows per update")
    env.reset()
    reward = {"twc": "twc", "colran": "colran", "ibsched": "ibsched"}[args.agent]
    t0 = time.perf_counter()
    for it in range(args.iters):
        env.enable_metrics(2)                      # (zeroes the sums: every iteration plays one whole episode per env)
        rec = env.collect_head(L, reward=reward)
        st = env.ppo_update_head(rec, epochs=args.epochs, minibatch=args.minibatch, seed=args.seed + it, order="device" if args.device_order else None)
        if inter:
            ep = env.episode_metrics()["episode_log"][:, 0, 1]
        else:
            ep = env.head_episode_metrics()["episode_log"][:, 0, 0 if args.agent == "twc" else 1]
        print(f"iteration {it + 1:3d}: mean episode {reward} reward {float(ep.mean()):+.4f}; last epoch: policy loss {st['policy_loss'][-1]:+.4f}, "
              f"value loss {st['value_loss'][-1]:.4f}, clip fraction {st['clip_frac'][-1]:.3f}, log_std mean {float(env.head_log_std().mean()):+.4f}", flush=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"{args.iters} iterations of {B} envs x {L} TTIs, {args.epochs} epochs of minibatch {args.minibatch}: {dt / args.iters * 1e3:.1f} ms per iteration")
    host = lambda net: [(w.cpu(), b.cpu()) for w, b in net]  # noqa: E731
    sd = adapters.sb3_ppo_state_dict(host(env.head_net_weights("actor")), env.head_log_std().cpu(), host(env.head_net_weights("critic")))
    torch.save(sd, args.out)
    print(f"wrote {args.out}: {len(sd)} tensors")
    env.close()


if __name__ == "__main__":
    main()
