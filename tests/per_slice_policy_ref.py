"""The float64 twin of the non-shared intra policies (ranenv_set_intra_policy_networks / _intra_value_networks): tests/policy_ref.py's
``mlp64`` run per slice -- slice index s's rows through net s -- behind ``PolicyRef``'s ``forward`` hook, so that the epilogue
(``intra_epilogue``), ``check_actions`` and the bounds of tests/collect_ref.py are the shared path's, unchanged.

The cases are the shapes the CPU and the GPU tests share: batches of 33 and 70 are one and two full tiles of 32 envs plus a tail,
widths 48 and 40 are padded (and take the other LDS row stride), 512 is the LDS maximum."""
from __future__ import annotations

import numpy as np

from tests import policy_ref as pr

# (S, Us, B, intra hidden widths, activation of both nets, intra input layout)
CASES = [(3, 4, 70, [32], "tanh", "obs"), (5, 5, 70, [48, 40], "relu", "mask_obs"), (5, 5, 33, [512, 512], "tanh", "obs"),
         (10, 10, 33, [64, 64], "tanh", "mask_obs")]
CASE_IDS = ["S3-32", "S5-48x40", "S5-512x512", "S10-64x64"]
# Every (case, seed of make_nets) that a GPU test hands to check_actions: the CPU tests hold the twin's share of decidable rows for them
TWIN_NETS = [(case, 500 + 20 * k) for k, case in enumerate(CASES)] + [((5, 5, 70, [33], "tanh", "obs"), 980)]
# What a wrong weight base would do: slice s served by net SLIPS[name](s, S)
SLIPS = {"next": lambda s, S: (s + 1) % S, "first": lambda s, S: 0, "mirrored": lambda s, S: S - 1 - s}


class PerSlice(list):
    """The (W, b) stacks of S nets of one shape, entry s for slice index s: what ``forward`` runs per slice."""


def intra_width(Us, layout):
    return 2 * Us + 9 + (Us if layout == "mask_obs" else 0)


def make_nets(case, seed):
    """(inter actor, S intra actors, inter critic, S intra critics) of a case: the intra nets ``make_net(seed + s)`` of its widths,
    the inter nets of width 32."""
    from tests.gpu_common import make_inter_net, make_net
    S, Us, B, widths, act, layout = case
    n_in = intra_width(Us, layout)
    return (make_inter_net(S, [32], act, seed + 100), [make_net([n_in] + list(widths) + [3], act, seed + s) for s in range(S)],
            make_net([10 * S, 32, 1], act, seed + 200), [make_net([n_in] + list(widths) + [1], act, seed + 300 + s) for s in range(S)])


def layers_of(net):
    from intent_radio_sched_multi_slice_amd.batched_env import policy_net_layers
    return policy_net_layers(net)


def stacks_of(nets):
    """(PerSlice of the nets' layers, their common activation)"""
    got = [layers_of(n) for n in nets]
    assert len({act for _, act in got}) == 1
    return PerSlice(layers for layers, _ in got), got[0][1]


def forward(x, layers, act, t0=None):
    """``policy_ref.mlp64``; for a ``PerSlice`` stack on intra rows [B*S, K] (row b*S + s): slice s's rows through net s."""
    if not isinstance(layers, PerSlice):
        return pr.mlp64(x, layers, act, t0)
    S = len(layers)
    xs = pr._np(x).reshape(-1, S, np.shape(x)[-1])
    outs = [pr.mlp64(xs[:, s], layers[s], act) for s in range(S)]
    y, t = np.stack([o[0] for o in outs], axis=1), np.stack([o[1] for o in outs], axis=1)
    return y.reshape(xs.shape[0] * S, -1), t.reshape(xs.shape[0] * S, -1)


def policy_ref(snap, inter, intras, stochastic, seed, layout, env_id_base=0):
    """``PolicyRef`` of a snapshot (dict of obs_inter, obs_intra, mask_inter, mask_intra, episode_number, step_number) under the
    inter net and the S intra nets."""
    B = snap["obs_inter"].shape[0]
    return pr.PolicyRef(snap["obs_inter"], snap["mask_inter"], layers_of(inter), snap["obs_intra"], snap["mask_intra"], stacks_of(intras),
                        stochastic=stochastic, seed=seed, layout=layout, env_ids=env_id_base + np.arange(B), episode=snap["episode_number"],
                        step=snap["step_number"], forward=forward)


def synthetic_snapshot(case, seed):
    """A snapshot without a device: ``injected_inputs`` observations, random masks (env 0: every slice active), counters of a
    batch some TTIs into different episodes."""
    S, Us, B = case[:3]
    rng = np.random.default_rng(seed)
    oi, oa = pr.injected_inputs(rng, B, S, Us)
    mask_inter = (rng.random((B, S)) < 0.7).astype(np.int8)
    mask_inter[0] = 1
    return {"obs_inter": oi, "obs_intra": oa, "mask_inter": mask_inter, "mask_intra": (rng.random((B, S, Us)) < 0.6).astype(np.int8),
            "episode_number": rng.integers(0, 50, B).astype(np.int32), "step_number": rng.integers(0, 30, B).astype(np.int32)}


def check_intra_values(vf, obs_inter, obs_intra, mask_intra, v_inter, v_intras, layout, what="vf"):
    """vf [B, S+1] against the inter critic and the S intra critics: ``collect_ref.check_values`` (its bound, its message) once per
    slice on columns (0, s + 1) with slice s's rows and critic.  Returns the worst error / bound ratio."""
    from tests import collect_ref as cr
    vf, oa, mk = pr._np(vf), pr._np(obs_intra, np.float32), pr._np(mask_intra, np.float32)
    return max(cr.check_values(vf[:, [0, s + 1]], obs_inter, oa[:, s:s + 1], mk[:, s:s + 1], v_inter, v, layout, f"{what}, slice {s}")
               for s, v in enumerate(v_intras))


def check_intra_logp(rec, t, intras, layout):
    """Slot t's intra log-probabilities of the record's own choices against the S float64 actors on the recorded rows, within
    collect_ref's bound: 2 max t_logit + 1e-12 + 2^-24 |logp|.  Returns the worst error / bound ratio."""
    B, S = rec["action_intra"][t].shape
    lg, lg_t = forward(pr.intra_input(rec["obs_intra"][t], rec["mask_intra"][t], layout), *stacks_of(intras))
    lg, lg_t = lg.reshape(B, S, 3), lg_t.reshape(B, S, 3)
    ch = rec["action_intra"][t].astype(np.int64)
    assert ch.min() >= 0 and ch.max() <= 2
    mx = lg.max(axis=-1)
    lpi = np.take_along_axis(lg, ch[..., None], -1)[..., 0] - mx - np.log(np.exp(lg - mx[..., None]).sum(axis=-1))
    bound = 2.0 * lg_t.max(axis=-1) + 1e-12 + 2.0 ** -24 * np.abs(lpi)
    err = np.abs(rec["logp"][t][:, 1:].astype(np.float64) - lpi)
    assert np.all(err <= bound), f"slot {t}: intra logp outside its bound: worst {np.max(err / bound):.3g}"
    return float(np.max(err / bound))
