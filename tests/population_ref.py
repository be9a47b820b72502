"""The twin of the population path (ranenv_set_population ...): the launch geometry restated in Python -- which workgroup holds which
rows of which member -- and tests/policy_ref.py's ``mlp64`` run per member behind ``PolicyRef``'s ``forward`` hook, env e's rows through
the nets of the member that owns e, so that the epilogue, ``check_actions`` and the bounds are the one-net path's, unchanged.

The cases are the smallest at which the env -> member map can go wrong: members of 5, 32 and 33 envs (less than a tile of 32 rows,
a tile, a tile and one row), 64 members of one and two envs (the last lane of the wave-wide search; intra tiles of S and 2 S rows),
one member."""
from __future__ import annotations

import numpy as np

from tests import policy_ref as pr

NET_ROWS = pr.NET_ROWS
FIRST_A = [0, 5, 37, 70]
FIRST_B = np.concatenate([[0], np.cumsum(np.tile([1, 2], 32))]).tolist()          # 64 members on 96 envs: 1, 2, 1, 2, ...
# name -> (S, Us, first_env, hidden widths of every net, activation, intra input layout)
CASES = {"a-S3-32": (3, 4, FIRST_A, [32], "tanh", "obs"), "a-S5-48x40": (5, 5, FIRST_A, [48, 40], "relu", "mask_obs"),
         "b-G64": (3, 4, FIRST_B, [32], "tanh", "obs"), "c-G1": (3, 4, [0, 70], [32], "tanh", "obs")}
# Every (case, seed of make_nets) that a GPU test hands to check_actions: the CPU tests hold the twin's share of decidable rows for them
TWIN_NETS = [("a-S3-32", 1500), ("a-S5-48x40", 1520)]


# ---- the geometry ------------------------------------------------------------------------------------------------------------
def owner(first, e):
    """The member that owns env e (an array of envs: an array of members)"""
    return np.searchsorted(np.asarray(first), e, side="right") - 1


def tiles(first, e0, n, rows_per_env):
    """The workgroups of a launch over envs [e0, e0 + n), in launch order: (member, first row relative to the launch's first row,
    live rows).  Member m contributes the rows of its envs inside the range, cut into tiles of NET_ROWS from ITS first row on."""
    out = []
    for m in range(len(first) - 1):
        lo, hi = max(first[m], e0), min(first[m + 1], e0 + n)
        rows = max(hi - lo, 0) * rows_per_env
        out += [(m, (lo - e0) * rows_per_env + r, min(NET_ROWS, rows - r)) for r in range(0, rows, NET_ROWS)]
    return out


# ---- the nets ----------------------------------------------------------------------------------------------------------------
def intra_width(Us, layout):
    return 2 * Us + 9 + (Us if layout == "mask_obs" else 0)


def make_member_nets(S, Us, G, widths, act, layout, seed):
    """Per role a list of G nets -- (inter actors, intra actors, inter critics, intra critics) -- member m's from seed + m"""
    from tests.gpu_common import make_inter_net, make_net
    n_in = intra_width(Us, layout)
    return ([make_inter_net(S, widths, act, seed + m) for m in range(G)], [make_net([n_in] + list(widths) + [3], act, seed + 100 + m) for m in range(G)],
            [make_net([10 * S] + list(widths) + [1], act, seed + 200 + m) for m in range(G)],
            [make_net([n_in] + list(widths) + [1], act, seed + 300 + m) for m in range(G)])


def make_nets(name, seed):
    """``make_member_nets`` of a case"""
    S, Us, first, widths, act, layout = CASES[name]
    return make_member_nets(S, Us, len(first) - 1, widths, act, layout, seed)


def layers_of(net):
    from intent_radio_sched_multi_slice_amd.batched_env import policy_net_layers
    return policy_net_layers(net)


# What a wrong map would do: env e served by member SLIPS[name](first, e) instead of its owner
SLIPS = {"next": lambda first, e: (owner(first, e) + 1) % (len(first) - 1), "first": lambda first, e: np.zeros_like(owner(first, e)),
         "boundary": lambda first, e: owner(np.asarray(first) + np.r_[0, np.ones(len(first) - 2, dtype=int), 0], e)}


class PerMember(list):
    """The (W, b) stacks of G nets of one shape, entry m for member m, with the map env -> member ``member_of`` [B]"""
    member_of = None


def stacks_of(nets, first, slip=None):
    """(PerMember of the nets' layers, their common activation)"""
    got = [layers_of(n) for n in nets]
    assert len({act for _, act in got}) == 1
    pm = PerMember(layers for layers, _ in got)
    e = np.arange(first[-1])
    pm.member_of = owner(first, e) if slip is None else SLIPS[slip](first, e)
    return pm, got[0][1]


def forward(x, layers, act, t0=None):
    """``policy_ref.mlp64``; for a ``PerMember`` stack on inter rows [B, K] or intra rows [B*S, K] (row b*S + s): env b's rows
    through its member's net."""
    if not isinstance(layers, PerMember):
        return pr.mlp64(x, layers, act, t0)
    x = pr._np(x)
    mem = np.repeat(layers.member_of, x.shape[0] // len(layers.member_of))
    y = t = None
    for m in np.unique(mem):
        ym, tm = pr.mlp64(x[mem == m], layers[m], act)
        if y is None:
            y, t = np.zeros((x.shape[0], ym.shape[1])), np.zeros((x.shape[0], ym.shape[1]))
        y[mem == m], t[mem == m] = ym, tm
    return y, t


def policy_ref(snap, inters, intras, first, stochastic, seed, layout, slip=None):
    """``PolicyRef`` of a snapshot (dict of obs_inter, obs_intra, mask_inter, mask_intra, episode_number, step_number) under the
    members' nets; ``slip``: a planted slip of the map."""
    B = snap["obs_inter"].shape[0]
    return pr.PolicyRef(snap["obs_inter"], snap["mask_inter"], stacks_of(inters, first, slip), snap["obs_intra"], snap["mask_intra"],
                        stacks_of(intras, first, slip), stochastic=stochastic, seed=seed, layout=layout, env_ids=np.arange(B),
                        episode=snap["episode_number"], step=snap["step_number"], forward=forward)


def synthetic_snapshot(name, seed):
    """A snapshot without a device: ``injected_inputs`` observations, random masks (env 0: every slice active), counters of a batch
    some TTIs into different episodes."""
    S, Us, first = CASES[name][:3]
    B = first[-1]
    rng = np.random.default_rng(seed)
    oi, oa = pr.injected_inputs(rng, B, S, Us)
    mask_inter = (rng.random((B, S)) < 0.7).astype(np.int8)
    mask_inter[0] = 1
    return {"obs_inter": oi, "obs_intra": oa, "mask_inter": mask_inter, "mask_intra": (rng.random((B, S, Us)) < 0.6).astype(np.int8),
            "episode_number": rng.integers(0, 50, B).astype(np.int32), "step_number": rng.integers(0, 30, B).astype(np.int32)}
