"""The reference's headline agent, `ray_ib_sched` with `param_config_mode: "pre_computed"`, trained on the device:

    python examples/train_precomputed_on_device.py --random [--envs 8] [--steps 8] [--iterations 5] [--members 1]

`pre_computed` is the outcome of the reference's own hyper-parameter search (agents/ray_agent.py:175-189): net_arch `verybig`
[512, 512, 512], lr 6.149e-6, sgd_minibatch_size 16, train_batch_size 64, num_sgd_iter 10, gamma 0.6, lambda 0.95, entropy_coeff
0.01441, vf_loss_coeff 0.4218, clip_param 0.2, grad_clip 0.5.  Nets of that shape are beyond the LDS plan of the plain PPO binding and
train under the wide one, `ppo_bind(wide=True)`: two row buffers in LDS, the layers' rows parked in a scratch in global memory.

Per iteration: one `collect()` -- envs x steps = the train batch, 64 rows by default as in the reference, GAE under gamma 0.6 -- then
RLlib's standardisation of the advantages over the whole train batch (one torch op per column of the record) and one `ppo_update()`
launch that runs the 10 epochs of minibatches of 16 for the inter and the intra nets; the next `collect()` acts on the new weights
with no rebind.  --members G trains G independent copies of the agent (seeds) side by side in the same two launches.
--random: random initial weights -- no checkpoint is shipped; a few iterations show the plumbing, not a learning curve.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from intent_radio_sched_multi_slice_amd import _lib
from intent_radio_sched_multi_slice_amd.batched_env import ppo_lds_bytes, ppo_wide_scratch_floats
from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload

PRE_COMPUTED = {"lr": 6.1494053683206764e-06, "sgd_minibatch_size": 16, "train_batch_size": 64, "gamma": 0.6, "num_sgd_iter": 10, "lambda": 0.95,
                "net_arch": [512, 512, 512], "clip_param": 0.2, "entropy_coeff": 0.014410343410248648, "vf_loss_coeff": 0.42179598812262487,
                "grad_clip": 0.5}


def random_net(dims, seed):
    torch.manual_seed(seed)
    mods = []
    for i in range(len(dims) - 1):
        mods.append(torch.nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods)


def standardise(rec, slices):
    """RLlib's advantage standardisation over the whole train batch, per policy and per member: the inter column, and the intra
    columns over the rows of active slices"""
    for sl in slices:
        a = rec["adv"][:, sl, 0]
        a.copy_((a - a.mean()) / a.std().clamp_min(1e-4))
        live = rec["mask_inter"][:, sl] != 0
        b = rec["adv"][:, sl, 1:]
        if int(live.sum()) > 1:
            b[live] = (b[live] - b[live].mean()) / b[live].std().clamp_min(1e-4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--random", action="store_true", help="random initial weights (required: no checkpoint is shipped)")
    ap.add_argument("--envs", type=int, default=8, help="envs per member")
    ap.add_argument("--steps", type=int, default=8, help="TTIs per collected batch: envs x steps is the train batch (the reference's: 64)")
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--members", type=int, default=1, help="independent copies of the agent trained side by side (<= 64)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not args.random:
        ap.error("give --random: no checkpoint is shipped")
    hp, G, T = PRE_COMPUTED, args.members, args.steps
    B = G * args.envs
    wl = make_mult_slice_workload(B, torch.device("cuda", 0), policy=_lib.POLICY_MAPF, intra=_lib.INTRA_PF, n_scenarios=8, n_traces=8, trace_len=max(T, 64),
                                  max_steps=1000)
    env = wl.env
    S, W, h = env.S, env.W, hp["net_arch"]
    pairs = {"inter": ([10 * S] + h + [2 * S], [10 * S] + h + [1]), "intra": ([W] + h + [3], [W] + h + [1])}
    for kind, (a, c) in pairs.items():
        print(f"{kind} nets {a} / {c}: {ppo_lds_bytes(a, c)} bytes of LDS under the plain plan (limit 163840), {ppo_lds_bytes(a, c, wide=True)} under "
              f"the wide one, {ppo_wide_scratch_floats(a, c)} floats parked per workgroup")
    nets = [{"inter": random_net(pairs["inter"][0], 1000 + 10 * m), "intra": random_net(pairs["intra"][0], 1001 + 10 * m),
             "v_inter": random_net(pairs["inter"][1], 1002 + 10 * m), "v_intra": random_net(pairs["intra"][1], 1003 + 10 * m)} for m in range(G)]
    env.set_population(sizes=[args.envs] * G)
    env.set_policy_network([n["inter"] for n in nets], [n["intra"] for n in nets], stochastic=True, seed=args.seed)
    env.set_value_network([n["v_inter"] for n in nets], [n["v_intra"] for n in nets])
    env.ppo_bind(wide=True)
    env.reset()
    last = hp["num_sgd_iter"] - 1
    for it in range(args.iterations):
        rec = env.collect(T, gamma=hp["gamma"], lam=hp["lambda"])
        standardise(rec, env.population_slices())
        stats = env.ppo_update(rec, epochs=hp["num_sgd_iter"], minibatch=hp["sgd_minibatch_size"], lr=hp["lr"], clip=hp["clip_param"],
                               vf_coeff=hp["vf_loss_coeff"], ent_coeff=hp["entropy_coeff"], grad_clip=hp["grad_clip"], adv_norm=None, seed=args.seed + it)
        for m, sl in enumerate(env.population_slices()):
            reward = rec["reward"][:, sl, 0].mean().item()
            for k, kind in enumerate(("inter", "intra")):
                print(f"iteration {it} member {m} {kind}: reward {reward:+.4f}  pi loss {stats['policy_loss'][m, k, last]:+.4f}  vf loss {stats['value_loss'][m, k, last]:.4f}  "
                      f"entropy {stats['entropy'][m, k, last]:.4f}  kl {stats['kl'][m, k, last]:+.2e}  clip frac {stats['clip_frac'][m, k, last]:.3f}  "
                      f"grad norm {stats['grad_norm'][m, k, last]:.3f}  rows {int(stats['rows'][m, k, last])}  steps {int(stats['minibatches'][m, k].sum())}", flush=True)
    env.close()


if __name__ == "__main__":
    main()
