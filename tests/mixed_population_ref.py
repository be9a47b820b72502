"""The twin of the mixed population path (ranenv_set_population_policy_mixed ...): member -> its own shape and activation -> float64
forward (tests/policy_ref.py's ``mlp64`` behind ``PolicyRef``'s ``forward`` hook, as tests/population_ref.py does for members of one
shape), per-member GAE on ``adapters.gae``, the library's packed-size rule restated, and the slips a wrong implementation could make.

The members' shapes are chosen so that each slip has somewhere to show: member 0 has one hidden layer of a width that is no multiple
of 32 and the smallest LDS need, member 2 the maximum depth; the critics are mixed differently from the actors (member 0 gets the
deepest); in the "wide" set member 2 is [512] with relu beside tanh members -- the widest LDS rows, sized from a member that is not
member 0, and an activation per member."""
from __future__ import annotations

import numpy as np

from tests import policy_ref as pr
from tests import population_ref as pop

CASE = "a-S3-32"                                   # S 3 / Us 4, B 70, members of 5 / 32 / 33 envs
S, US, FIRST = pop.CASES[CASE][0], pop.CASES[CASE][1], pop.FIRST_A
G = len(FIRST) - 1
# name -> (actors' hidden widths per member, critics' hidden widths per member, activation per member)
SETS = {"mixed": ([[24], [64, 40], [33, 32, 96, 32]], [[33, 32, 96, 32], [24], [64, 40]], ["tanh", "tanh", "tanh"]),
        "wide": ([[24], [64, 40], [512]], [[33, 32, 96, 32], [24], [512]], ["tanh", "tanh", "relu"])}
GAMMA, LAM = [0.5, 0.99, 0.9999], [1.0, 0.8, 0.95]
N_IN = 2 * US + 9


def make_nets(name, seed, members=None):
    """(inter actors, intra actors, inter critics, intra critics) of a set, member m's from seed + m; ``members``: the set's shapes
    of these members instead (e.g. [2, 2, 2]: three nets of member 2's shape)"""
    from tests.gpu_common import make_inter_net, make_net
    a_hid, c_hid, acts = SETS[name]
    ms = list(range(G)) if members is None else list(members)
    return ([make_inter_net(S, a_hid[m], acts[m], seed + i) for i, m in enumerate(ms)],
            [make_net([N_IN] + a_hid[m] + [3], acts[m], seed + 100 + i) for i, m in enumerate(ms)],
            [make_net([10 * S] + c_hid[m] + [1], acts[m], seed + 200 + i) for i, m in enumerate(ms)],
            [make_net([N_IN] + c_hid[m] + [1], acts[m], seed + 300 + i) for i, m in enumerate(ms)])


def packed_floats(dims, bf16=False):
    """The library's size rule (ranenv_packed_net_floats): every width padded to 32; per layer kp * np weights -- two per float for a
    bf16 net -- and np biases"""
    p = [pr.pad32(int(d)) for d in dims]
    return sum(k * n // (2 if bf16 else 1) + n for k, n in zip(p[:-1], p[1:]))


# ---- the slips -------------------------------------------------------------------------------------------------------------------
def truncated(layers, width):
    """A member's net as a kernel would run it that sized its rows from member 0's entry: hidden units beyond ``width`` never computed
    (their weights and biases zero: act(0) = 0 feeds nothing on)"""
    out = []
    for i, (w, b) in enumerate(layers):
        w, b = pr._np(w).copy(), pr._np(b).copy()
        if i < len(layers) - 1:
            w[width:], b[width:] = 0.0, 0.0
        if i > 0:
            w[:, width:] = 0.0
        out.append((w, b))
    return out


class MixedStack(list):
    """Per member m the (W, b) stack of ITS net, with ``acts[m]`` and the map env -> member ``member_of`` [B]"""
    member_of = acts = None


def stacks_of(nets, first, slip=None):
    """(MixedStack, None) in the place of policy_net_layers' (layers, activation).  slip "next": the member table shifted by one;
    "truncate": every member's hidden widths cut to member 0's first hidden width."""
    got = [pop.layers_of(n) for n in nets]
    ms = MixedStack(layers for layers, _ in got)
    ms.acts = [act for _, act in got]
    e = np.arange(first[-1])
    ms.member_of = pop.SLIPS["next"](first, e) if slip == "next" else pop.owner(first, e)
    if slip == "truncate":
        w0 = got[0][0][0][0].shape[0]
        for m in range(1, len(ms)):
            ms[m] = truncated(ms[m], w0)
    return ms, None


def forward(x, layers, act, t0=None):
    """``policy_ref.mlp64``; for a ``MixedStack`` on inter rows [B, K] or intra rows [B * S, K]: env b's rows through its member's net
    under its member's activation"""
    if not isinstance(layers, MixedStack):
        return pr.mlp64(x, layers, act, t0)
    x = pr._np(x)
    mem = np.repeat(layers.member_of, x.shape[0] // len(layers.member_of))
    y = t = None
    for m in np.unique(mem):
        ym, tm = pr.mlp64(x[mem == m], layers[m], layers.acts[m])
        if y is None:
            y, t = np.zeros((x.shape[0], ym.shape[1])), np.zeros((x.shape[0], ym.shape[1]))
        y[mem == m], t[mem == m] = ym, tm
    return y, t


def policy_ref(snap, inters, intras, first, stochastic, seed, slip=None):
    """``PolicyRef`` of a snapshot under the members' own nets; ``slip``: a planted slip"""
    B = snap["obs_inter"].shape[0]
    return pr.PolicyRef(snap["obs_inter"], snap["mask_inter"], stacks_of(inters, first, slip), snap["obs_intra"], snap["mask_intra"],
                        None if intras is None else stacks_of(intras, first, slip), stochastic=stochastic, seed=seed, layout="obs",
                        env_ids=np.arange(B), episode=snap["episode_number"], step=snap["step_number"], forward=forward)


def gae_ref(reward, vf, done, first, gamma, lam, slip=None):
    """(adv, vtarg) float32 [T, B, C]: ``adapters.gae`` on every member's slice with that member's pair; slip "next": the neighbouring
    member's pair"""
    from intent_radio_sched_multi_slice_amd.adapters import gae
    reward, vf, done = (np.asarray(x) for x in (reward, vf, done))
    adv, vtarg = np.empty(reward.shape, dtype=np.float32), np.empty(reward.shape, dtype=np.float32)
    n = len(first) - 1
    for m in range(n):
        k = (m + 1) % n if slip == "next" else m
        sl = slice(first[m], first[m + 1])
        adv[:, sl], vtarg[:, sl] = gae(reward[:, sl], vf[:, sl], done[:, sl], gamma[k], lam[k])
    return adv, vtarg
