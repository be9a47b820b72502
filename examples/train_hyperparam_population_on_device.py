"""The trials of a hyper-parameter search TRAINED as one mixed population on the device: what examples/hyperparam_population.py collects,
this one also trains -- every member on its own architecture, with its own learning rate, minibatch size, SGD epochs, GAE gamma and
lambda -- and then runs PBT's exploit step across architectures:

    python examples/train_hyperparam_population_on_device.py --random [--members 8] [--envs-per-member 16] [--steps 64] [--iterations 3]

Per iteration: one `collect()` for all members (every member's advantages under its own gamma / lambda) and one `ppo_update()` launch
in which workgroup (member, kind) runs that member's whole SGD schedule on the member's own net shape (`ppo_bind(mixed=True)`).  The
architectures are drawn from those of the reference's `net_arch` choices whose 32-row activations fit the update's LDS plan
(`ppo_lds_bytes`, asked before anything is bound): [64, 64], [256, 256], [400, 300] and [256, 256, 256]; [512, 512, 512] does not.
With --wide the population is bound with `ppo_bind(mixed=True, wide=True)` -- two row buffers in LDS, the layers' rows parked in a
scratch in global memory -- and `verybig` [512, 512, 512] is drawn with the others: all five architectures of the reference's search.
Then the worst member by mean collected reward becomes a copy of the best through `set_population_member` -- trained weights into
another member's extent, whatever the two shapes; the library restarts that member's optimiser -- and training goes on.
--random: random initial weights -- no trial checkpoints are shipped; a few iterations show the plumbing, not a learning curve.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from intent_radio_sched_multi_slice_amd import _lib
from intent_radio_sched_multi_slice_amd.batched_env import ppo_lds_bytes
from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload

NET_ARCH = {"small": [64, 64], "medium": [256, 256], "big": [400, 300], "large": [256, 256, 256], "verybig": [512, 512, 512]}
PPO_LDS_MAX = 163840
# per-trial choices in the ranges a PPO search draws from
LR = [5e-5, 1e-4, 3e-4]
MINIBATCH = [32, 64, 128]
EPOCHS = [2, 4, 6]
GAMMA = [0.9, 0.95, 0.99, 0.995]
LAMBDA = [0.9, 0.95, 1.0]


def random_net(dims, seed):
    torch.manual_seed(seed)
    mods = []
    for i in range(len(dims) - 1):
        mods.append(torch.nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods)


def as_net(layers, activation):
    """(W, b) tensors as read back from the device -> a module that `set_population_member` takes"""
    mods = []
    for i, (w, b) in enumerate(layers):
        lin = torch.nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            lin.weight.copy_(w)
            lin.bias.copy_(b)
        mods.append(lin)
        if i < len(layers) - 1:
            mods.append(torch.nn.Tanh() if activation == "tanh" else torch.nn.ReLU())
    return torch.nn.Sequential(*mods)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--random", action="store_true", help="random initial weights (required: no trial checkpoints are shipped)")
    ap.add_argument("--members", type=int, default=8, help="G: trials in the batch (<= 64)")
    ap.add_argument("--envs-per-member", type=int, default=16)
    ap.add_argument("--steps", type=int, default=64, help="TTIs per collected batch")
    ap.add_argument("--iterations", type=int, default=3, help="collect + update rounds before and after the exploit step")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--wide", action="store_true", help="bind the update wide: [512, 512, 512] becomes trainable")
    args = ap.parse_args()
    if not args.random:
        ap.error("give --random: no trial checkpoints are shipped")
    G, T = args.members, args.steps
    B = G * args.envs_per_member
    wl = make_mult_slice_workload(B, torch.device("cuda", 0), policy=_lib.POLICY_MAPF, intra=_lib.INTRA_PF, n_scenarios=8, n_traces=8, trace_len=T,
                                  max_steps=1000)
    env = wl.env
    S, W = env.S, env.W

    # only architectures a member can be trained with: the LDS need of the actor / critic pair of both kinds, before any bind
    def lds_need(h):
        return max(ppo_lds_bytes([10 * S] + h + [2 * S], [10 * S] + h + [1], wide=args.wide), ppo_lds_bytes([W] + h + [3], [W] + h + [1], wide=args.wide))
    trainable = [name for name, h in NET_ARCH.items() if lds_need(h) <= PPO_LDS_MAX]
    print("LDS bytes of the update per architecture: " + ", ".join(f"{n} {lds_need(h)}" for n, h in NET_ARCH.items()) + f"; trainable: {trainable}")
    rng = np.random.default_rng(args.seed)
    pick = lambda xs: xs[int(rng.integers(len(xs)))]  # noqa: E731
    trials = [{"arch": pick(trainable), "lr": pick(LR), "minibatch": pick(MINIBATCH), "epochs": pick(EPOCHS), "gamma": pick(GAMMA), "lam": pick(LAMBDA)}
              for _ in range(G)]

    def nets_of(m, seed):
        h = NET_ARCH[trials[m]["arch"]]
        return {"inter": random_net([10 * S] + h + [2 * S], seed), "intra": random_net([W] + h + [3], seed + 1),
                "v_inter": random_net([10 * S] + h + [1], seed + 2), "v_intra": random_net([W] + h + [1], seed + 3)}
    nets = [nets_of(m, 1000 + 10 * m) for m in range(G)]
    env.set_population(sizes=[args.envs_per_member] * G)
    env.set_policy_network([n["inter"] for n in nets], [n["intra"] for n in nets], stochastic=True, seed=args.seed, mixed=True)
    env.set_value_network([n["v_inter"] for n in nets], [n["v_intra"] for n in nets], mixed=True)
    env.ppo_bind(mixed=True, wide=args.wide)
    env.reset()
    col = lambda k: [t[k] for t in trials]  # noqa: E731

    def iterate(n, label):
        reward = None
        for it in range(n):
            rec = env.collect(T, gamma=col("gamma"), lam=col("lam"))
            stats = env.ppo_update(rec, epochs=col("epochs"), minibatch=col("minibatch"), lr=col("lr"), seed=args.seed + it)
            reward = np.array([rec["reward"][:, sl, 0].mean().item() for sl in env.population_slices()])
            print(f"\n{label} iteration {it}: {'member':>6} {'net_arch':>16} {'lr':>7} {'mb':>4} {'ep':>3} {'gamma':>6} {'lam':>5} | {'reward':>9} {'pi loss':>9} {'vf loss':>9} {'kl':>9} {'steps':>6}")
            for m in range(G):
                last = trials[m]["epochs"] - 1
                print(f"{'':>{len(label) + 14}} {m:>6} {str(env.population_net('inter', m)['hidden']):>16} {trials[m]['lr']:>7} {trials[m]['minibatch']:>4} "
                      f"{trials[m]['epochs']:>3} {trials[m]['gamma']:>6} {trials[m]['lam']:>5} | {reward[m]:>9.4f} {stats['policy_loss'][m, 0, last]:>9.4f} "
                      f"{stats['value_loss'][m, 0, last]:>9.4f} {stats['kl'][m, 0, last]:>9.2e} {int(stats['minibatches'][m, 0].sum()):>6}")
        return reward

    reward = iterate(args.iterations, "before")

    # PBT's exploit step across architectures: the best member's TRAINED nets, read back from the device, into the worst member
    best, worst = int(np.argmax(reward)), int(np.argmin(reward))
    if best != worst:
        copy = {r: as_net(env.net_weights(r, best), env.net_activation(r, best)) for r in ("inter", "intra", "v_inter", "v_intra")}
        was = env.population_net("inter", worst)["hidden"]
        env.set_population_member(worst, **copy)
        trials[worst] = dict(trials[best])
        st = env.ppo_state("inter", worst)
        assert int(st["t"][0]) == 0 and not bool(st["m"].any())          # (a new net starts a new optimiser)
        print(f"\nmember {worst} ({was}) is now a copy of member {best} ({env.population_net('inter', worst)['hidden']}) with its hyper-parameters; "
              f"its optimiser starts again")
        iterate(args.iterations, "after")
    env.close()


if __name__ == "__main__":
    main()
