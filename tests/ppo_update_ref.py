"""What the tests of the PPO update share (tests/test_ppo_update_cpu.py, tests/test_gpu_ppo_update.py, tests/test_gpu_ppo_update_shapes.py):
the cases and the shape grid, the members' nets, a synthetic ``collect()`` record for the CPU, the packed-gradient layout, the numpy
float32 restatement of clip + Adam in the operation order include/ranenv.h states, the header's LDS formula, and the comparisons of a
handle's update with the twin that the GPU files share.  The float64 twin itself is ``adapters.ppo_update_reference``."""
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
ALL = 1 << 20                            # a minibatch size beyond every member's rows: one minibatch per epoch
# The shape grid of tests/test_gpu_ppo_update_shapes.py, name -> (S, Us, intra input layout, (actor hidden widths, activation), (critic ...)):
#   A  the edge of the LDS plan (162 304 of 163 840 bytes for both kinds), 32 x 32 blocks per dW
#   B  four hidden layers with alternating LDS strides, deep ReLU, inter input 130 -> 160, a critic shallower than the actor
#   C  2 S = 32 outputs with no padding, intra input 57, a critic deeper than the actor
#   D  S 1: i / S and i % S degenerate, j0 always 0; width 64 (stride 68 by the "+4" rule)
#   E  intra input 33, one column past a tile; odd wide widths
#   F  five layers, a 7-wide bottleneck between wide ones
SHAPES = {"A": (5, 5, "obs", ([512, 512, 32], "tanh"), ([512, 512, 32], "tanh")),
          "B": (13, 5, "mask_obs", ([33, 160, 7, 96], "relu"), ([96], "tanh")),
          "C": (16, 16, "mask_obs", ([160], "tanh"), ([33, 96, 7], "relu")),
          "D": (1, 1, "obs", ([32], "relu"), ([64, 64], "tanh")),
          "E": (5, 8, "mask_obs", ([255, 100], "tanh"), ([480], "relu")),
          "F": (10, 10, "obs", ([64, 7, 255, 33], "tanh"), ([100, 255, 64], "tanh"))}
SHAPE_SEED = 5200                        # the nets' seed: tests/test_ppo_update_cpu.py guards that no gradient tensor of the twin is zero with it
LDS_MAX = 163840


def intra_width(Us, layout):
    return 2 * Us + 9 + (Us if layout == "mask_obs" else 0)


def make_role_nets(S_, Us, widths, act, layout, seed, critic_widths=None, critic_act=None):
    """The four nets of one member; the critics take the actors' hidden widths and activation unless given their own"""
    n_in = intra_width(Us, layout)
    cw, ca = list(widths if critic_widths is None else critic_widths), act if critic_act is None else critic_act
    return {"inter": make_inter_net(S_, widths, act, seed), "intra": make_net([n_in] + list(widths) + [3], act, seed + 1),
            "v_inter": make_net([10 * S_] + cw + [1], ca, seed + 2), "v_intra": make_net([n_in] + cw + [1], ca, seed + 3)}


def shape_nets(shape, G, seed=SHAPE_SEED):
    """{role: [member's net]}: G distinct net sets of the SHAPES entry"""
    S_, Us, layout, (aw, aa), (cw, ca) = SHAPES[shape]
    per = [make_role_nets(S_, Us, aw, aa, layout, seed + 10 * m, cw, ca) for m in range(G)]
    return {r: [p[r] for p in per] for r in ROLES}


def net_ld(x):
    """The LDS row stride of a padded width (include/ranenv.h, the LDS plan)"""
    return x + (36 if x % 64 else 4)


def pair_lds_bytes(*nets):
    """The header's formula for ONE kind's pair, nets given as widths [in, hidden..., out] (None: not bound): 4096 + 128 * sum over the
    input and the layers of ld(width padded to 32), the larger of actor and critic"""
    return max(4096 + 128 * sum(net_ld(pad32(w)) for w in dims) for dims in nets if dims is not None)


def lds_bytes(S_, Us, layout, actor_widths, critic_widths):
    """... and the larger of the two kinds' pairs"""
    return max(pair_lds_bytes([n_in] + list(actor_widths) + [n_out], [n_in] + list(critic_widths) + [1])
               for n_in, n_out in ((10 * S_, 2 * S_), (intra_width(Us, layout), 3)))


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


def synthetic_record(B=12, seed=0, T_=T, layout="mask_obs", S=S, Us=US):
    """A record shaped as ``collect()`` fills it, on the CPU: random observations, masks with 1..S live slices (sorted position: the
    last n are active), recorded actions -1 where masked, plausible logp / adv / vtarg."""
    g = torch.Generator().manual_seed(seed)
    W = 2 * Us + 9
    n_live = torch.randint(1, S + 1, (T_, B), generator=g)
    mask = torch.zeros((T_, B, S), dtype=torch.int8)
    for t in range(T_):
        for b in range(B):
            mask[t, b, torch.randperm(S, generator=g)[:n_live[t, b]]] = 1
    active = torch.arange(S)[None, None, :] >= (S - n_live)[..., None]
    action = torch.where(active, torch.randn((T_, B, S), generator=g, dtype=torch.float64) * 0.5, torch.full((T_, B, S), -1.0, dtype=torch.float64))
    return {"obs_inter": torch.rand((T_, B, 10 * S), generator=g), "obs_intra": torch.rand((T_, B, S, W), generator=g),
            "mask_inter": mask, "mask_intra": (torch.rand((T_, B, S, Us), generator=g) < 0.6).to(torch.int8), "action_inter": action,
            "action_intra": torch.randint(0, 3, (T_, B, S), generator=g).to(torch.uint8),
            "logp": (torch.randn((T_, B, S + 1), generator=g) * 0.3 - 1.5).to(torch.float32),
            "adv": torch.randn((T_, B, S + 1), generator=g), "vtarg": torch.randn((T_, B, S + 1), generator=g),
            "vf": torch.randn((T_ + 1, B, S + 1), generator=g)}


# ----------------------------------------------------------------------------------------------------------------------
# a handle's update against the twin: what tests/test_gpu_ppo_update.py and tests/test_gpu_ppo_update_shapes.py share
# ----------------------------------------------------------------------------------------------------------------------
def native_workload(B, trace_len=32, seed=10):
    """The native shape (5 slices, 25 UEs, 135 RBs in groups of 5) with every env on a scenario that has an inactive slice"""
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    from tests.gpu_common import need_gpu
    need_gpu()
    wl = make_mult_slice_workload(B, torch.device("cuda", 0), policy=_lib.POLICY_MAPF, intra=_lib.INTRA_PF, n_scenarios=8, n_traces=8,
                                  trace_len=trace_len, seed=seed, n_slices=S, n_ues=25, n_rbs=135, rbs_per_rbg=5, max_ues_slice=US,
                                  max_steps=1000, min_slices=1, min_ues=1)
    n_active = (np.asarray(wl.tables.slice_active) != 0).sum(axis=1)
    partial = np.nonzero((n_active >= 1) & (n_active < S))[0]
    assert len(partial) >= 2, n_active
    env, scen = wl.env, partial[np.arange(B) % len(partial)]
    eps = env.episodes
    env.set_episodes(scenario=scen, se_base=eps["se_base"], se_len=eps["se_len"], se_offset=eps["se_offset"], trf_base=scen * trace_len,
                     trf_len=trace_len, trf_offset=eps["trf_offset"])
    return env


def _members(members):
    return range(members) if isinstance(members, int) else members


def weights(env, members, roles=ROLES):
    """Every role's read-back layers, {role: {member: list of (W, b) on the host}}; ``members``: a count G (0 .. G - 1) or a list"""
    return {r: {m: [(w.cpu().numpy().copy(), b.cpu().numpy().copy()) for w, b in env.net_weights(r, m)] for m in _members(members)} for r in roles}


def state(env, members, roles=ROLES):
    """The whole trainable state as host bytes: weights, moments and counters of every role and member"""
    out = {}
    for r in roles:
        for m in _members(members):
            for i, (w, b) in enumerate(env.net_weights(r, m)):
                out[f"{r}/{m}/w{i}"], out[f"{r}/{m}/b{i}"] = w.cpu().numpy().copy(), b.cpu().numpy().copy()
            st = env.ppo_state(r, m)
            for k, v in st.items():
                out[f"{r}/{m}/{k}"] = v.cpu().numpy().copy()
    return out


def same_state(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"


def check_against_twin(rec, order, out, weights, members, what, act_actor, act_critic, layout, hp=None, twin_order=None, scale=None):
    """dev_grad and the statistics of a one-minibatch call against the float64 twin at ``weights``; the float32 twin is the yardstick.
    Asserts the gradient; returns the worst device / yardstick ratio and the statistics beyond 1e-6 relative or absolute.
    ``twin_order``: the lists the twin runs (default ``order``, the call's own), and ``scale(kind, m)`` the factor on the twin's
    gradient and statistics 0..4 -- for a call whose lists hold entries outside the record: the twin runs the live entries, and a row's
    weight is 1 / (entries of the list), so the factor is live entries / entries."""
    from intent_radio_sched_multi_slice_amd.adapters import ppo_update_reference
    misses = []
    hp = dict(clip=0.2, vf_coeff=0.5, ent_coeff=0.01, adv_norm=True) if hp is None else hp
    twin_order = order if twin_order is None else twin_order
    host = {k: v.cpu() for k, v in rec.items()}
    worst = 0.0
    for kind_i, kind in enumerate(("inter", "intra")):
        first = twin_order["first_" + kind]
        for m in members:
            lo, hi = int(first[m]), int(first[m + 1])
            if hi == lo:
                continue
            f = 1.0 if scale is None else float(scale(kind, m))
            a, c = ("inter", "v_inter") if kind == "inter" else ("intra", "v_intra")
            critic = weights[c][m] if c in weights else None         # (a kind without a bound critic: no value term, actor gradient only)
            args = dict(rec=host, kind=kind, actor=as_torch(weights[a][m]), critic=None if critic is None else as_torch(critic), order=twin_order["order_" + kind].cpu(),
                        lo=lo, hi=hi, epochs=1, minibatch=ALL, lr=0.0, grad_clip=0.0, act_actor=act_actor, act_critic=act_critic,
                        layout=layout, **hp)
            t64, t32 = ppo_update_reference(dtype=torch.float64, **args), ppo_update_reference(dtype=torch.float32, **args)
            dev = unpack_grad(out["grad"][m, kind_i].cpu().numpy(), weights[a][m], critic or [])
            for net in ("actor", "critic"):
                for li, (g64, g32, gd) in enumerate(zip(t64["grad"][net], t32["grad"][net], dev[net])):
                    for name, x64, x32, xd in zip("Wb", g64, g32, gd):
                        x64, x32 = f * x64.numpy().astype(np.float64), f * x32.numpy().astype(np.float64)
                        n64 = np.linalg.norm(x64)
                        assert n64 > 0.0, f"{what}: {kind} member {m} {net} layer {li} {name}: the twin's gradient is zero"
                        e_dev, e_32 = np.linalg.norm(xd - x64) / n64, np.linalg.norm(x32 - x64) / n64
                        ratio = e_dev / max(e_32, 1e-6)
                        worst = max(worst, ratio)
                        assert ratio <= 8.0, f"{what}: {kind} member {m} {net} layer {li} {name}: device error {e_dev:.3g}, float32 torch {e_32:.3g}"
            for i, name in enumerate(("policy_loss", "value_loss", "entropy", "kl", "clip_frac")):
                got, want = out[name][m, kind_i, 0], f * t64["stats"][0, i]
                print(f"{what} {kind} m{m} {name}: device {got:.9g} twin {want:.9g}")
                if not abs(got - want) <= 1e-6 * max(1.0, abs(want)):
                    misses.append(f"{what}: {kind} member {m} {name}: device {got:.9g}, twin {want:.9g}")
            assert out["rows"][m, kind_i, 0] == hi - lo and out["minibatches"][m, kind_i, 0] == 1
    print(f"{what}: worst gradient error, device / float32 torch yardstick: {worst:.3g}")
    return worst, misses


def chunk_order(order, G, minibatch, ep, i):
    """The row lists of ONE call that holds, per member and kind, chunk ``i`` of epoch ``ep`` of ``order`` cut in chunks of ``minibatch``
    (a member with fewer chunks: an empty list): what the loop inside a launch works through in its step (ep, i)"""
    step = {}
    for kind in ("inter", "intra"):
        f, rows, first = order["first_" + kind], [], [0]
        for m in range(G):
            lo, hi = int(f[m]), int(f[m + 1])
            chunk = order["order_" + kind][ep, lo + i * minibatch:min(lo + (i + 1) * minibatch, hi)] if lo + i * minibatch < hi else order["order_" + kind][ep, 0:0]
            rows.append(chunk)
            first.append(first[-1] + chunk.numel())
        step["order_" + kind], step["first_" + kind] = torch.cat(rows)[None, :].contiguous(), np.array(first, dtype=np.int32)
    return step


def refusal(fn):
    """(code, text) of the RanEnvError that ``fn()`` must raise"""
    import pytest
    from intent_radio_sched_multi_slice_amd._lib import RanEnvError
    with pytest.raises(RanEnvError) as e:
        fn()
    return int(str(e.value).split("(")[1].split(")")[0]), str(e.value)


def check_adam_step(env, out, w0, w1, hp, G, what):
    """One minibatch with lr > 0 from zero moments: ``w1`` (read back behind the call) and Adam's m and v against ``adam_step_f32`` applied
    to the call's own dev_grad at ``w0``, in float32 ulp -- asserted within 4; grad_norm against the restatement's; the counters read 1;
    the padding of dev_grad, m and v exact zeros (``unpack_grad``).  ``hp``: lr [G], grad_clip [G], betas, eps.  Returns the two worst distances."""
    from tests.gpu_common import _ordered
    worst, exact, total = 0, 0, 0
    worst_mv, exact_mv, total_mv = 0, 0, 0
    for kind_i, (a, c) in enumerate((("inter", "v_inter"), ("intra", "v_intra"))):
        for m in range(G):
            g = unpack_grad(out["grad"][m, kind_i].cpu().numpy(), w0[a][m], w0[c][m], dtype=np.float32)
            want, norm, want_m, want_v = adam_step_f32(w0[a][m] + w0[c][m], g["actor"] + g["critic"], 1, float(hp["lr"][m]), float(hp["grad_clip"][m]),
                                                       hp["betas"], hp["eps"], moments=True)
            assert abs(out["grad_norm"][m, kind_i, 0] - norm) <= 1e-9 * norm
            for (ww, wb), (gw, gb) in zip(want, w1[a][m] + w1[c][m]):
                for x, y in ((ww, gw), (wb, gb)):
                    d = np.abs(_ordered(x) - _ordered(y))
                    worst, exact, total = max(worst, int(d.max())), exact + int((d == 0).sum()), total + d.size
            sa, sc = env.ppo_state(a, m), env.ppo_state(c, m)
            for name, want_x in (("m", want_m), ("v", want_v)):
                got = unpack_grad(np.concatenate([sa[name].cpu().numpy(), sc[name].cpu().numpy()]), w0[a][m], w0[c][m], dtype=np.float32)
                for (xw, xb), (yw, yb) in zip(want_x, got["actor"] + got["critic"]):
                    for x, y in ((xw, yw), (xb, yb)):
                        d = np.abs(_ordered(x) - _ordered(y))
                        worst_mv, exact_mv, total_mv = max(worst_mv, int(d.max())), exact_mv + int((d == 0).sum()), total_mv + d.size
            assert int(sa["t"].cpu()[0]) == 1
    print(f"{what}: Adam step, worst ulp distance {worst}; {exact} of {total} weights bit-equal to the numpy restatement")
    print(f"{what}: Adam moments, worst ulp distance {worst_mv}; {exact_mv} of {total_mv} bit-equal to the numpy restatement")
    assert worst <= 4
    assert worst_mv <= 4
    return worst, worst_mv
