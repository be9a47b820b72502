"""What the tests of the PPO update share (tests/test_ppo_update_cpu.py, tests/test_gpu_ppo_update.py): the cases, the members' nets,
a synthetic ``collect()`` record for the CPU, the packed-gradient layout, and the numpy float32 restatement of clip + Adam in the
operation order include/ranenv.h states.  The float64 twin itself is ``adapters.ppo_update_reference``."""
from __future__ import annotations

import numpy as np
import torch

from tests.gpu_common import make_inter_net, make_net

S, US, T = 5, 5, 8                       # the reference's native shape: 5 slices, 25 UEs, 5 UEs per slice at most
FIRST = [0, 2, 6, 12]                    # members of 2, 4, 6 envs: 16, 32, 48 inter rows -- a partial tile, a tile, a tile and a half
MINIBATCH = 12                           # every member has a short tail
SEED = 0x1357_9BDF_2468_ACE0
ROLES = ("inter", "intra", "v_inter", "v_intra")
# name -> (hidden widths, activation, intra input layout): every width off the 32 grid
CASES = {"relu24": ([24], "relu", "obs"), "tanh40x24": ([40, 24], "tanh", "mask_obs"), "tanh8x4": ([8, 8, 8, 8], "tanh", "obs")}
HALF_LN_2PI = 0.9189385332046727
LN_1E9 = 20.72326583694641


def intra_width(Us, layout):
    return 2 * Us + 9 + (Us if layout == "mask_obs" else 0)


def make_role_nets(S_, Us, widths, act, layout, seed):
    n_in = intra_width(Us, layout)
    return {"inter": make_inter_net(S_, widths, act, seed), "intra": make_net([n_in] + list(widths) + [3], act, seed + 1),
            "v_inter": make_net([10 * S_] + list(widths) + [1], act, seed + 2), "v_intra": make_net([n_in] + list(widths) + [1], act, seed + 3)}


def member_nets(case, G, seed=4100):
    """{role: [member's net]}: G distinct net sets of the case's shape"""
    widths, act, layout = CASES[case]
    per = [make_role_nets(S, US, widths, act, layout, seed + 10 * m) for m in range(G)]
    return {r: [p[r] for p in per] for r in ROLES}


def layers_of(net):
    return [(m.weight.detach().clone(), m.bias.detach().clone()) for m in net if isinstance(m, torch.nn.Linear)]


def as_torch(layers):
    return [(torch.as_tensor(w), torch.as_tensor(b)) for w, b in layers]


def as_sequential(layers, act):
    mods = []
    for i, (w, b) in enumerate(layers):
        lin = torch.nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.as_tensor(w))
            lin.bias.copy_(torch.as_tensor(b))
        mods.append(lin)
        if i < len(layers) - 1:
            mods.append(torch.nn.Tanh() if act == "tanh" else torch.nn.ReLU())
    return torch.nn.Sequential(*mods)


def pad32(x):
    return (x + 31) // 32 * 32


def unpack_grad(flat, actor, critic, dtype=np.float64):
    """dev_grad of one (member, kind) -- the packed layout, actor then critic: per layer W [np][kp] row-major, then b [np], widths padded
    to 32 -- as {"actor": [(dW, db)], "critic": [...]} in torch layout; the padding must be exact zeros."""
    out, at = {}, 0
    for name, net in (("actor", actor), ("critic", critic)):
        out[name] = []
        for w, b in net:
            N, K = w.shape
            np_, kp = pad32(N), pad32(K)
            W = flat[at:at + np_ * kp].reshape(np_, kp)
            at += np_ * kp
            bb = flat[at:at + np_]
            at += np_
            assert not W[N:].any() and not W[:, K:].any() and not bb[N:].any(), f"{name}: gradient in the padding"
            out[name].append((W[:N, :K].astype(dtype), bb[:N].astype(dtype)))
    assert not flat[at:].any()
    return out


def adam_step_f32(weights, grads, t, lr, grad_clip, betas=(0.9, 0.999), eps=1e-8, moments=False):
    """include/ranenv.h's clip + Adam on float32 numpy arrays, operation for operation, from zero moments at step ``t``:
    ``weights`` / ``grads`` lists of (W, b).  Returns ([(W', b')], the float64 joint norm), with ``moments`` also [(mW, mb)], [(vW, vb)]."""
    f = np.float32
    flat = [x for pair in grads for x in pair]
    norm = float(np.sqrt(sum(float((x.astype(np.float64) ** 2).sum()) for x in flat)))
    scale = f(min(1.0, grad_clip / (norm + 1e-6)) if grad_clip > 0 else 1.0)
    b1, omb1, b2, omb2, e = f(betas[0]), f(1.0 - betas[0]), f(betas[1]), f(1.0 - betas[1]), f(eps)
    step, sbc2 = f(lr / (1.0 - betas[0] ** t)), f(np.sqrt(1.0 - betas[1] ** t))
    out, ms, vs = [], [], []
    for (w, b), (gw, gb) in zip(weights, grads):
        new, m_new, v_new = [], [], []
        for x, g in ((w, gw), (b, gb)):
            g = g.astype(f) * scale
            mi = b1 * np.zeros_like(g) + omb1 * g
            vi = b2 * np.zeros_like(g) + (omb2 * g) * g
            new.append((x.astype(f) - step * (mi / (np.sqrt(vi) / sbc2 + e))).astype(f))
            m_new.append(mi.astype(f))
            v_new.append(vi.astype(f))
        out.append(tuple(new))
        ms.append(tuple(m_new))
        vs.append(tuple(v_new))
    return (out, norm, ms, vs) if moments else (out, norm)


def synthetic_record(B=12, seed=0, T_=T, layout="mask_obs"):
    """A record shaped as ``collect()`` fills it, on the CPU: random observations, masks with 1..S live slices (sorted position: the
    last n are active), recorded actions -1 where masked, plausible logp / adv / vtarg."""
    g = torch.Generator().manual_seed(seed)
    W = 2 * US + 9
    n_live = torch.randint(1, S + 1, (T_, B), generator=g)
    mask = torch.zeros((T_, B, S), dtype=torch.int8)
    for t in range(T_):
        for b in range(B):
            mask[t, b, torch.randperm(S, generator=g)[:n_live[t, b]]] = 1
    active = torch.arange(S)[None, None, :] >= (S - n_live)[..., None]
    action = torch.where(active, torch.randn((T_, B, S), generator=g, dtype=torch.float64) * 0.5, torch.full((T_, B, S), -1.0, dtype=torch.float64))
    return {"obs_inter": torch.rand((T_, B, 10 * S), generator=g), "obs_intra": torch.rand((T_, B, S, W), generator=g),
            "mask_inter": mask, "mask_intra": (torch.rand((T_, B, S, US), generator=g) < 0.6).to(torch.int8), "action_inter": action,
            "action_intra": torch.randint(0, 3, (T_, B, S), generator=g).to(torch.uint8),
            "logp": (torch.randn((T_, B, S + 1), generator=g) * 0.3 - 1.5).to(torch.float32),
            "adv": torch.randn((T_, B, S + 1), generator=g), "vtarg": torch.randn((T_, B, S + 1), generator=g),
            "vf": torch.randn((T_ + 1, B, S + 1), generator=g)}
