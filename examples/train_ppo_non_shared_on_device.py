"""The reference's non-shared IBSched training entry in miniature with BOTH halves on the device: `collect()` records the batch and
`ppo_update_per_slice()` trains the 1 + S policies in one launch -- nothing leaves the device between a `collect()` and the next.

    python examples/train_ppo_non_shared_on_device.py [--batch 64] [--ttis 32] [--iters 5] [--epochs 10] [--minibatch 64] [--width 64] [--device-order]
    python examples/train_ppo_non_shared_on_device.py --spread [SLABS]      # the large batch: B 4096 x 64 TTIs, 4 epochs, minibatch 8192

The reference's `scratch_ray_ib_sched_non_shared` agent (simu.py: "train": True, "shared_policies": False) trains one RLlib PPO policy
for the inter-slice agent and one per slice for the intra-slice agents (agents/ray_agent.py:420-460), each a FullyConnectedNetwork
with a value branch, under ONE config.  Here per iteration:

  1. `env.collect(T)`: T TTIs of B envs under the actors on the device -- slice s's rows acted by slice s's net -- with the per-slice
     log-probabilities, values, GAE advantages and value targets in columns 1 + s of the record;
  2. `env.ppo_update_per_slice(rec, ...)`: one launch of 1 + S workgroups; workgroup 0 trains the inter pair, workgroup 1 + s slice s's
     pair on the live rows of slice s, each with its own Adam state (clip 0.2, vf coefficient 0.5, entropy coefficient 0.01, gradient
     clip 0.5, lr 3e-4, gamma 0.99, lambda 0.95: the reference's defaults), written in place: the next `collect()` acts on the
     trained nets with no rebind.

`--spread [SLABS]` (default 64): the same loop under `ppo_bind(per_slice=True, spread=True, slabs=SLABS)` on the batch of
examples/train_ppo_large_batch_on_device.py -- B 4096, 64 TTIs, 4 epochs, minibatches of 8192, the row lists drawn on the device --,
which the per-slice binding refuses (`PPO_ROW_EPOCHS_CAP`: a policy is one workgroup there).  Every optimiser step of the 1 + S policies
is three launches in which each policy's minibatch is spread over up to SLABS workgroups; the policies keep their own step counts.
Prints ms per iteration and env-steps/s.

At the end the trained nets are read back per slice (`net_weights("intra", slice=s)`) and packed as an RLlib-style weights dict
(`adapters.rllib_per_slice_weights`; parity with RLlib itself is unpinned).  An example of the API, not a tuned trainer.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from intent_radio_sched_multi_slice_amd._lib import INTRA_PF, POLICY_MAPF
from intent_radio_sched_multi_slice_amd.adapters import rllib_per_slice_weights
from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload

HP = dict(lr=3e-4, clip=0.2, vf_coeff=0.5, ent_coeff=0.01, grad_clip=0.5)
GAMMA, LAMBDA = 0.99, 0.95


def mlp(n_in, n_out, width):
    return torch.nn.Sequential(torch.nn.Linear(n_in, width), torch.nn.Tanh(), torch.nn.Linear(width, width), torch.nn.Tanh(),
                               torch.nn.Linear(width, n_out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=None, help="default 64; 4096 under --spread")
    ap.add_argument("--ttis", type=int, default=None, help="TTIs per collect() call, default 32: 64 x 32 = 2048 rows per policy at the most, the reference's batch; 64 under --spread")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=None, help="default 10; 4 under --spread")
    ap.add_argument("--minibatch", type=int, default=None, help="default 64; 8192 under --spread")
    ap.add_argument("--spread", type=int, nargs="?", const=64, default=None, metavar="SLABS",
                    help="ppo_bind(per_slice=True, spread=True, slabs=SLABS): the large-batch defaults, row lists drawn on the device")
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--episode-len", type=int, default=100)
    ap.add_argument("--device-order", action="store_true", help='draw the row lists on the device: ppo_update_per_slice(..., order="device")')
    args = ap.parse_args()
    for name, small, large in (("batch", 64, 4096), ("ttis", 32, 64), ("epochs", 10, 4), ("minibatch", 64, 8192)):
        if getattr(args, name) is None:
            setattr(args, name, small if args.spread is None else large)
    args.device_order = args.device_order or args.spread is not None
    dev = torch.device("cuda", 0)
    B, T, L = args.batch, args.ttis, args.episode_len
    n_ep = 64
    wl = make_mult_slice_workload(B, dev, policy=POLICY_MAPF, intra=INTRA_PF, n_scenarios=n_ep, n_traces=n_ep, trace_len=L, max_steps=L)
    env = wl.env
    S, W = env.S, env.W
    ep = np.arange(n_ep)
    env.set_episode_table(scenario=ep, se_base=ep * L, se_len=L, trf_base=ep * L, trf_len=L)
    env.enable_autoreset(0, n_ep, random_episodes=True, seed=7, episode_numbers=np.arange(B) % n_ep)

    torch.manual_seed(0)
    pi_inter, vf_inter = mlp(10 * S, 2 * S, args.width), mlp(10 * S, 1, args.width)
    pi_intra, vf_intra = [mlp(W, 3, args.width) for _ in range(S)], [mlp(W, 1, args.width) for _ in range(S)]      # pair s: player_{s+1}
    with torch.no_grad():
        pi_inter[-1].bias[S:].fill_(-0.5)          # initial log_std
    env.set_policy_network(pi_inter, pi_intra, stochastic=True, seed=1000)
    env.set_value_network(vf_inter, vf_intra)
    if args.spread is None:
        env.ppo_bind(per_slice=True)               # (bound ONCE: from here on the nets live, act and train on the device)
    else:
        env.ppo_bind(per_slice=True, spread=True, slabs=args.spread)
    env.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(args.iters):
        rec = env.collect(T, gamma=GAMMA, lam=LAMBDA)
        st = env.ppo_update_per_slice(rec, epochs=args.epochs, minibatch=args.minibatch, seed=it, order="device" if args.device_order else None, **HP)
        r = rec["reward"][..., 0].mean().item()
        rows = st["rows"][:, 0].astype(int).tolist()
        print(f"iteration {it + 1:3d}: mean inter-slice reward {r:+.4f}; rows per policy {rows}; last epoch's policy loss "
              f"{np.array2string(st['policy_loss'][:, -1], precision=4)}, value loss {np.array2string(st['value_loss'][:, -1], precision=3)}, "
              f"kl {np.array2string(st['kl'][:, -1], precision=5)}", flush=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n = B * T * args.iters
    print(f"{B} envs x {T} TTIs x {args.iters} iterations, {args.epochs} epochs of minibatch {args.minibatch} for 1 + {S} policies: "
          f"{1e3 * dt / args.iters:.1f} ms per iteration, {n / dt / 1e3:.1f} k env-steps/s with the updates included"
          + (f" ({args.spread} slabs per policy)" if args.spread is not None else ""))
    actors, critics = [env.net_weights("intra", slice=s) for s in range(S)], [env.net_weights("v_intra", slice=s) for s in range(S)]
    weights = rllib_per_slice_weights(actors, critics)
    print(f"read back: {sorted(weights)} ({sum(v.numel() for sd in weights.values() for v in sd.values())} parameters)")
    env.close()


if __name__ == "__main__":
    main()
