"""The loop of examples/train_ppo_on_device.py with BOTH halves on the device: `collect()` records the batch, `ppo_update()` under the
spread binding trains ONE agent on it with every optimiser step spread over the chip.

    python examples/train_ppo_large_batch_on_device.py [--batch 4096] [--ttis 64] [--iters 10] [--epochs 4] [--minibatch 65536] [--slabs 64] [--bf16] [--device-order]

Per iteration:

  1. `env.collect(T)`: T TTIs of B envs under the actors on the device; the record, GAE advantages and value targets stay in HBM;
  2. `env.ppo_update(rec, ...)` under `ppo_bind(spread=True, slabs=...)`: `--epochs` passes of minibatch SGD over the 262 144 inter rows
     and the live intra rows -- clipped surrogate, value loss, entropy bonus, joint gradient clip, Adam (clip 0.2, vf coefficient 0.5,
     entropy coefficient 0.01, gradient clip 0.5, lr 3e-4, gamma 0.99, lambda 0.95: the reference's defaults) -- in place in the buffers
     the acting kernels read: the next collect() acts on the new weights, nothing is bound again.

The plain binding gives an agent to one workgroup and refuses such a batch (`PPO_ROW_EPOCHS_CAP`); the eager-torch loop of
examples/train_ppo_on_device.py spends 98 % of its time in the SGD half.  Prints env-steps/s with the updates included, the share of
collection in it, and per iteration the mean inter-slice reward and the last epoch's statistics of the inter kind.

`--bf16`: the same loop a second time with every net bound with precision="bf16" under `ppo_bind(spread=True, bf16=True)` -- acting and
learning both on the bf16 matrix cores, float32 master weights behind the acting copy -- from the same initial weights and seeds, and
the two runs' losses and rates side by side.  The runs differ from the first collect() on: the bf16 nets act on rounded weights.

`--device-order`: the minibatch row lists come from the library's own kernels (`ppo_update(..., order="device")`: a stable
compaction of the live intra rows and a keyed per-entry shuffle, no sort and no key tensor) instead of torch's generator and argsort.
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

CLIP, VF_COEFF, ENT_COEFF, GRAD_CLIP, LR, GAMMA, LAMBDA = 0.2, 0.5, 0.01, 0.5, 3e-4, 0.99, 0.95


def mlp(n_in, n_out, width=64):
    return torch.nn.Sequential(torch.nn.Linear(n_in, width), torch.nn.Tanh(), torch.nn.Linear(width, width), torch.nn.Tanh(),
                               torch.nn.Linear(width, n_out))


def main():
    args = parse()
    f32 = run(args, False)
    if args.bf16:
        bf16 = run(args, True)
        print("iteration: inter policy loss, value loss, KL -- float32 nets | bf16 nets")
        for it, (a, b) in enumerate(zip(f32["stats"], bf16["stats"])):
            print(f"{it + 1:9d}: {a[0]:+.4f} {a[1]:.4f} {a[2]:+.5f} | {b[0]:+.4f} {b[1]:.4f} {b[2]:+.5f}")
        print(f"env-steps/s with the updates included: float32 {f32['rate'] / 1e6:.2f} M, bf16 {bf16['rate'] / 1e6:.2f} M; "
              f"collection alone: float32 {f32['collect_rate'] / 1e6:.2f} M, bf16 {bf16['collect_rate'] / 1e6:.2f} M")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--ttis", type=int, default=64, help="TTIs per collect() call: the train batch is batch x ttis env-steps")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatch", type=int, default=65536)
    ap.add_argument("--slabs", type=int, default=64, help="gradient slabs: workgroups per kind that share a minibatch's tiles (1..256)")
    ap.add_argument("--episode-len", type=int, default=100)
    ap.add_argument("--se-mode", choices=("stream", "gather"), default="gather")
    ap.add_argument("--device-order", action="store_true", help='draw the row lists on the device: ppo_update(..., order="device")')
    ap.add_argument("--bf16", action="store_true", help="run the loop a second time with bf16 nets under ppo_bind(spread=True, bf16=True)")
    return ap.parse_args()


def run(args, bf16):
    dev = torch.device("cuda", 0)
    B, T, L = args.batch, args.ttis, args.episode_len
    n_ep = 64
    wl = make_mult_slice_workload(B, dev, policy=POLICY_MAPF, intra=INTRA_PF, n_scenarios=n_ep, n_traces=n_ep, trace_len=L, max_steps=L)
    env = wl.env
    S, W = env.S, env.W
    env.set_se_mode(args.se_mode)
    ep = np.arange(n_ep)
    env.set_episode_table(scenario=ep, se_base=ep * L, se_len=L, trf_base=ep * L, trf_len=L)
    env.enable_autoreset(0, n_ep, random_episodes=True, seed=7, episode_numbers=np.arange(B) % n_ep)

    torch.manual_seed(0)
    pi_inter, vf_inter, pi_intra, vf_intra = mlp(10 * S, 2 * S), mlp(10 * S, 1), mlp(W, 3), mlp(W, 1)
    with torch.no_grad():
        pi_inter[-1].bias[S:].fill_(-0.5)          # initial log_std
    precision = "bf16" if bf16 else "f32"
    env.set_policy_network(pi_inter, pi_intra, stochastic=True, seed=1000, precision=precision)
    env.set_value_network(vf_inter, vf_intra, precision=precision)
    env.ppo_bind(spread=True, slabs=args.slabs, bf16=bf16)
    env.reset()
    stats = []
    torch.cuda.synchronize()
    t_collect, t0 = 0.0, time.perf_counter()
    for it in range(args.iters):
        tc = time.perf_counter()
        rec = env.collect(T, gamma=GAMMA, lam=LAMBDA)
        torch.cuda.synchronize()
        t_collect += time.perf_counter() - tc
        out = env.ppo_update(rec, epochs=args.epochs, minibatch=args.minibatch, lr=LR, clip=CLIP, vf_coeff=VF_COEFF, ent_coeff=ENT_COEFF,
                             grad_clip=GRAD_CLIP, seed=it, order="device" if args.device_order else None)
        r = rec["reward"][..., 0].mean().item()
        last = args.epochs - 1
        stats.append((out["policy_loss"][0, 0, last], out["value_loss"][0, 0, last], out["kl"][0, 0, last]))
        print(f"{precision} iteration {it + 1:3d}: mean inter-slice reward {r:+.4f}, {int(rec['done'].sum())} episode ends; inter policy loss "
              f"{out['policy_loss'][0, 0, last]:+.4f}, value loss {out['value_loss'][0, 0, last]:.4f}, KL {out['kl'][0, 0, last]:+.5f}, "
              f"{int(out['minibatches'][0, 0, last])} + {int(out['minibatches'][0, 1, last])} steps per epoch", flush=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n = B * T * args.iters
    print(f"{precision} nets: {B} envs x {T} TTIs x {args.iters} iterations, {args.epochs} epochs of minibatch {args.minibatch} each on {args.slabs} slabs "
          f"(SE mode {args.se_mode}): {n / dt / 1e6:.2f} M env-steps/s with the updates included; collection alone "
          f"{n / t_collect / 1e6:.2f} M env-steps/s ({100 * t_collect / dt:.0f} % of the time)")
    env.close()
    return {"stats": stats, "rate": n / dt, "collect_rate": n / t_collect}


if __name__ == "__main__":
    main()
