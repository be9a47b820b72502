"""What the tests of the head policies' PPO update share (tests/test_ppo_head_cpu.py, tests/test_gpu_ppo_head.py): the cases, their nets
and ``log_std``, a synthetic ``collect_head()`` record for the CPU, the noise that turns a real record into one with a clip fraction
strictly between 0.1 and 0.9, the layout of ``dev_grad`` (actor packed, critic packed, ``log_std``), and the comparison of a one-minibatch
call with the float64 twin, ``adapters.ppo_head_update_reference``.

The yardstick is ppo_update_ref.check_against_twin's -- per tensor e_dev <= 8 max(e_32, 1e-6), relative in the 2-norm against the float64
twin, e_32 the float32 twin's figure -- with ``log_std`` as a tensor of its own.  That function itself runs ``ppo_update_reference`` on the
IBSched kinds and their ``[members, kinds]`` outputs, so the head comparison is stated here on its constants (FACTOR, FLOOR) and on
``unpack_grad`` / ``adam_step_f32`` / ``same_state`` / ``refusal`` of that module, which are used as they are."""
from __future__ import annotations

import numpy as np
import torch

from tests import head_policy_ref as hr
from tests import head_shapes_ref as hs
from tests import ppo_update_ref as ref

B, T = 12, 8
N = B * T                                # 96 rows: three tiles
MINIBATCH = 12
T_LONG = 24                              # the long record of tests/ppo_head_shapes_ref.py: B x T_LONG = 288 rows, nine tiles, more than 256
N_LONG = B * T_LONG
LONG_MINIBATCH = 257                     # ... in minibatches of 257 and 31 rows
SEED = 0x2468_ACE0_1357
FACTOR, FLOOR = 8.0, 1e-6                # ppo_update_ref.check_against_twin's constants
ALL = ref.ALL
# name -> (S, actor widths, actor activation, critic widths, critic activation, observation, reward)
CASES = {"base": (5, [24], "relu", [40, 24], "tanh", "head", "twc"),
         "sb3": (16, [64, 64], "tanh", [64, 64], "tanh", "head", "colran"),           # SB3's default pair; the epilogue fills 16 positions
         "deg": (1, [7, 100], "relu", [96], "tanh", "head", "twc"),
         "inter": (3, [33, 160, 7, 96], "relu", [96], "tanh", "inter", "ibsched")}
ENV_SIZES = {5: "S5U25", 16: hs.ENV_SHAPES[16], 1: hs.ENV_SHAPES[1], 3: hs.ENV_SHAPES[3],
             6: hs.ENV_SHAPES[6], 8: hs.ENV_SHAPES[8], 10: "S10U100"}      # (6, 8, 10: tests/ppo_head_shapes_ref.py's grid)
HP = dict(clip=0.2, vf_coeff=0.5, ent_coeff=0.01, adv_norm=True)
NOISE = (0.05, 0.6)                      # |noise| on logp, one of the two per row: exp(0.05) is inside the clip range 0.2, exp(0.6) outside
SLIPS = ("no_entropy_gradient", "log_std_outside_norm", "stale_log_std", "short_logp", "masked_term", "cell_stride")


def spec(case):
    """A case's tuple: ``case`` a name of CASES, or such a tuple itself (tests/ppo_head_shapes_ref.py's grid)"""
    return CASES[case] if isinstance(case, str) else tuple(case)


def head_nets(case, seed=61):
    """(actor, log_std float32 [S] in [-1, 0.5], critic) of the case as torch modules / tensor"""
    S, aw, aa, cw, ca = spec(case)[:5]
    g = torch.Generator().manual_seed(seed + 1)
    log_std = (torch.rand(S, generator=g) * 1.5 - 1.0).to(torch.float32)
    return hr.mlp([10 * S] + aw + [S], aa, seed), log_std, hr.mlp([10 * S] + cw + [1], ca, seed + 2)


def layers(case, seed=61):
    """(actor layers, log_std, critic layers): lists of (W, b) float32 tensors"""
    actor, log_std, critic = head_nets(case, seed)
    return ref.layers_of(actor), log_std, ref.layers_of(critic)


def logp_noise(n, seed=7):
    """float32 [n]: +-NOISE[0] or +-NOISE[1], sign and magnitude seeded"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.where(torch.rand(n, generator=g) < 0.5, NOISE[0], NOISE[1])
    return (mag * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)).to(torch.float32)


def row_order(epochs, seed=5, n=N):
    """int32 [epochs, n]: a seeded permutation of the n first record rows per epoch, on the host"""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randperm(n, generator=g) for _ in range(epochs)]).to(torch.int32).contiguous()


def _noise_seed():
    """The first seed from 7 on whose large-noise rows number 3 .. 7 in every 12-row chunk of ``row_order(2)``.  Those rows clip
    from the start; at the sb3 case (16 positions) sixteen steps of 3e-4 move the policy far enough to clip up to three small-noise rows
    more, so the room above is theirs.  tests/test_ppo_head_cpu.py holds the twin's clip fraction of every such minibatch strictly
    inside (0.1, 0.9).  The same share -- a quarter to seven twelfths -- holds in every chunk of the long record's order
    (``row_order(2, n=N_LONG)`` in minibatches of LONG_MINIBATCH: 257 and 31 rows per epoch) and so in its 288 rows as one minibatch;
    tests/test_ppo_head_shapes_cpu.py holds the twin's clip fractions there."""
    order, long_order = row_order(2).long(), row_order(2, n=N_LONG).long()
    for seed in range(7, 1000):
        big = (logp_noise(N, seed).abs() > 0.3).to(torch.float64)[order]
        long_big = (logp_noise(N_LONG, seed).abs() > 0.3).to(torch.float64)[long_order]
        if all(3 <= int(c.sum()) <= 7 for ep in big for c in ep.split(MINIBATCH)) and all(
                3 * len(c) <= 12 * int(c.sum()) <= 7 * len(c) for ep in long_big for c in ep.split(LONG_MINIBATCH)):
            return seed
    raise AssertionError("no seed")


def with_noise(rec, seed=None):
    """A copy of a ``collect_head()`` record (device or host) whose logp is the recorded one plus ``logp_noise``"""
    out = {k: v.clone() for k, v in rec.items()}
    seed = NOISE_SEED if seed is None else seed
    out["logp"] = out["logp"] + logp_noise(out["logp"].numel(), seed).reshape(out["logp"].shape).to(out["logp"].device)
    return out


NOISE_SEED = _noise_seed()
_SYNTH = {}


def synthetic_record(case, seed=3, T=T, net_seed=61):
    """A record of ``T`` TTIs shaped as ``collect_head()`` fills it, on the CPU (computed once, shared, never modified): random observations,
    actions drawn from the case's own policy, logp that policy's log-probability plus ``logp_noise``, random adv / vtarg."""
    key = (repr(case), seed, T, net_seed)
    if key not in _SYNTH:
        S = spec(case)[0]
        actor, log_std, _ = head_nets(case, net_seed)
        g = torch.Generator().manual_seed(seed)
        obs = torch.rand((T, B, 10 * S), generator=g)
        with torch.no_grad():
            mean = actor.double()(obs.double())
        actor.float()
        sd = torch.exp(log_std.double())
        action = mean + sd * torch.randn((T, B, S), generator=g, dtype=torch.float64)
        logp = torch.distributions.Normal(mean, sd.expand_as(mean)).log_prob(action).sum(dim=-1)
        _SYNTH[key] = {"obs_head": obs, "action": action, "logp": logp.to(torch.float32) + logp_noise(T * B, NOISE_SEED).reshape(T, B),
                                "adv": torch.randn((T, B), generator=g), "vtarg": torch.randn((T, B), generator=g),
                                "vf": torch.randn((T + 1, B), generator=g)}
    return _SYNTH[key]


def twin(case, rec, order, lay=None, dtype=torch.float64, slip=None, **kw):
    from intent_radio_sched_multi_slice_amd.adapters import ppo_head_update_reference
    actor, log_std, critic = layers(case) if lay is None else lay
    return ppo_head_update_reference({k: v.cpu() for k, v in rec.items()}, actor, log_std, critic, order, act_actor=spec(case)[2],
                                     act_critic=spec(case)[4], dtype=dtype, slip=slip, **kw)


def packed_floats(net):
    return sum(ref.pad32(w.shape[0]) * ref.pad32(w.shape[1]) + ref.pad32(w.shape[0]) for w, _ in net)


def unpack_head_grad(flat, actor, critic, S, dtype=np.float64):
    """dev_grad -- actor packed, critic packed, log_std [S] -- as {"actor": [(dW, db)], "critic": [...], "log_std": [S]}; the padding
    must be exact zeros (ppo_update_ref.unpack_grad) and nothing lies behind log_std"""
    nets = packed_floats(actor) + packed_floats(critic)
    assert flat.shape == (nets + S,)
    out = ref.unpack_grad(flat[:nets], actor, critic, dtype)
    out["log_std"] = flat[nets:].astype(dtype)
    return out


def tensors(g):
    """{name: array} of a gradient (or weight) set {"actor": [(W, b)], "critic": [...], "log_std"}"""
    out = {}
    for net in ("actor", "critic"):
        for li, pair in enumerate(g[net]):
            for name, x in zip("Wb", pair):
                out[f"{net} layer {li} {name}"] = np.asarray(x.numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64)
    x = g["log_std"]
    out["log_std"] = np.asarray(x.numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float64)
    return out


def ratios(got, t64, t32, scale=1.0):
    """name -> (e / max(e_32, FLOOR), e, e_32) per tensor of ``tensors``-dicts; asserts that no tensor of the float64 twin is zero"""
    out = {}
    for k, x64 in t64.items():
        x64 = scale * x64
        n64 = np.linalg.norm(x64)
        assert n64 > 0.0, f"{k}: the twin's tensor is zero"
        e, e32 = np.linalg.norm(got[k] - x64) / n64, np.linalg.norm(scale * t32[k] - x64) / n64
        out[k] = (e / max(e32, FLOOR), e, e32)
    return out


def forward_bounds(case, rec, rows, lay, clip):
    """What ANY float32 evaluation of the actor may move of the statistics of the minibatch ``rows`` under advantages as given:
    (bound of kl, bound of policy_loss).  policy_ref.mlp64 bounds every mean by t_j; logp is sum_j -z_j^2 / 2 + .., z_j = (a_j - mean_j)
    / sigma_j, so a row's logp moves by at most E = sum_j (|z_j| + d_j / 2) d_j with d_j = t_j / sigma_j, its ratio r by r expm1(E), and
    min(r A, clamp(r) A) -- 1-Lipschitz in r A -- by |A| r expm1(E); the statistics are the rows' means."""
    from tests import policy_ref as pr
    S = spec(case)[0]
    rows = torch.as_tensor(rows).long().reshape(-1)
    x = rec["obs_head"].reshape(-1, 10 * S)[rows].cpu().numpy()
    mean, t = pr.mlp64(x, [(w.numpy(), b.numpy()) for w, b in lay[0]], spec(case)[2])
    sd = np.exp(lay[1].numpy().astype(np.float64))
    z = (rec["action"].reshape(-1, S)[rows].cpu().numpy() - mean) / sd
    d = t / sd
    E = ((np.abs(z) + 0.5 * d) * d).sum(axis=1) + 1e-12
    lp = (-0.5 * z * z - np.log(sd) - ref.HALF_LN_2PI).sum(axis=1)
    r = np.exp(lp - rec["logp"].reshape(-1)[rows].cpu().numpy().astype(np.float64))
    adv = np.abs(rec["adv"].reshape(-1)[rows].cpu().numpy().astype(np.float64))
    return float(E.mean()), float((adv * r * np.expm1(E)).mean())


def check_head_against_twin(case, rec, order, out, lay, what, hp=None, twin_order=None, scale=1.0, rows=None, forward_bound=False):
    """dev_grad and the statistics of a one-minibatch call against the float64 twin at the weights ``lay``; the float32 twin is the
    yardstick.  Asserts the gradient per tensor; returns (the worst ratio, the statistics beyond 1e-6).  ``twin_order`` / ``scale``: for
    a call whose list holds entries outside the record, the live entries and live / entries; ``rows``: the entries the call counted.
    ``forward_bound`` (minibatches of a few rows, whose means average nothing out; advantages as given): policy_loss and kl, the two
    statistics that read the actor's outputs through logp, get ``forward_bounds`` on top of the 1e-6."""
    hp = dict(HP) if hp is None else hp
    twin_order = order if twin_order is None else twin_order
    args = dict(epochs=1, minibatch=ALL, lr=0.0, grad_clip=0.0, **hp)
    t64, t32 = twin(case, rec, twin_order, lay, **args), twin(case, rec, twin_order, lay, dtype=torch.float32, **args)
    S = spec(case)[0]
    dev = tensors(unpack_head_grad(out["grad"].cpu().numpy(), lay[0], lay[2], S))
    r = ratios(dev, tensors(t64["grad"]), tensors(t32["grad"]), scale)
    worst = max(v[0] for v in r.values())
    for k, (ratio, e, e32) in r.items():
        assert ratio <= FACTOR, f"{what}: {k}: device error {e:.3g}, float32 torch {e32:.3g}"
    misses, extra = [], {}
    if forward_bound:
        assert not hp["adv_norm"]
        e_kl, e_pl = forward_bounds(case, rec, twin_order[0], lay, hp["clip"])
        extra = {"kl": scale * e_kl, "policy_loss": scale * e_pl}
        print(f"{what}: forward bounds: kl {e_kl:.3g}, policy_loss {e_pl:.3g}")
    for i, name in enumerate(("policy_loss", "value_loss", "entropy", "kl", "clip_frac")):
        got, want = out[name][0], scale * t64["stats"][0, i]
        print(f"{what} {name}: device {got:.9g} twin {want:.9g}")
        if not abs(got - want) <= 1e-6 * max(1.0, abs(want)) + extra.get(name, 0.0):
            misses.append(f"{what}: {name}: device {got:.9g}, twin {want:.9g}")
    n_entries = order.shape[1] if rows is None else rows
    assert out["rows"][0] == twin_order.shape[1] and out["minibatches"][0] == 1 and n_entries >= twin_order.shape[1]
    print(f"{what}: worst gradient error, device / float32 torch yardstick: {worst:.3g}")
    return worst, misses


# ---- GPU fixtures -------------------------------------------------------------------------------------------------------------------
def make_env(case, stochastic=True, bind=True, ppo=True, seed=SEED, net_seed=61):
    """A reset env of B envs at the case's shape under the case's head nets (head PPO state bound); returns (env, (actor layers,
    log_std, critic layers))"""
    from tests import inter_head_ref as ih
    S, _, aa, _, ca, observation, _ = spec(case)
    if observation == "inter":
        _, env, _ = ih.make_env(ENV_SIZES[S], "64x64", "gauss_clip", B, bind=False)
    else:
        _, env, _ = hr.make_env(ENV_SIZES[S], "64x64", "gauss_clip", B, bind=False)
    assert env.S == S
    lay = layers(case, net_seed)
    if bind:
        bind_nets(env, case, lay, stochastic, seed)
        if ppo:
            env.ppo_bind(head=True)
        env.reset()
    return env, lay


def bind_nets(env, case, lay, stochastic=True, seed=SEED):
    _, _, aa, _, ca, observation, _ = spec(case)
    env.set_head_policy_network(lay[0], "gauss_clip", lay[1], stochastic=stochastic, seed=seed, activation=aa, observation=observation,
                                allow_sorted=observation == "inter")
    env.set_head_value_network(lay[2], activation=ca)


def collect(env, case, T=T):
    """A private copy of ``collect_head(T)``'s record (the env reuses its tensors)"""
    return {k: v.clone() for k, v in env.collect_head(T, reward=spec(case)[6]).items()}


def head_weights(env):
    """(actor layers, log_std, critic layers) as they are on the device now, on the host"""
    host = lambda net: [(w.cpu(), b.cpu()) for w, b in net]  # noqa: E731
    return host(env.head_net_weights("actor")), env.head_log_std().cpu(), host(env.head_net_weights("critic"))


def head_state(env):
    """The whole trainable state as host bytes: weights, log_std, moments and the counter"""
    a, ls, c = head_weights(env)
    out = {"log_std": ls.numpy().copy()}
    for name, net in (("actor", a), ("critic", c)):
        for i, (w, b) in enumerate(net):
            out[f"{name}/w{i}"], out[f"{name}/b{i}"] = w.numpy().copy(), b.numpy().copy()
    for which in ("actor", "critic", "log_std"):
        for k, v in env.ppo_head_state(which).items():
            out[f"{which}/{k}"] = v.cpu().numpy().copy()
    return out
