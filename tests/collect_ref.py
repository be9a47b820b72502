"""What the tests of ``collect()`` share: twin envs under the same nets, and the float64 reference of one recorded TTI -- values,
log-probabilities, unclamped actions -- with the error bounds of tests/policy_ref.py (``mlp64`` gives every net output ``y`` a bound
``t`` on its distance to ANY float32 evaluation):

    vf            |vf - y| <= t + 2^-24 |y|
    inter logp    sum over the active positions of t_log_std  +  1e-12 S (1 + max z^2)  +  2^-24 |logp|
    intra logp    of the device's own recorded choice: 2 max t_logit + 1e-12 + 2^-24 |logp|
                  (each l_i - max l moves by at most 2 max t; log-sum-exp is 1-Lipschitz in the sup norm)
    action_inter  policy_ref.inter_epilogue's bound without its clamp step; masked positions exactly -1

The 2^-24 terms are the record's single rounding to float32, the 1e-12 terms the double transcendental libraries (as in policy_ref).
"""
from __future__ import annotations

import numpy as np
import torch

from tests import policy_ref as pr

NETS = {"64x64": [64, 64], "512x3": [512, 512, 512]}
SIZES = {"S10U100": dict(n_slices=10, n_ues=100, n_rbs=135, rbs_per_rbg=1, max_ues_slice=10),
         "S5U25": dict(n_slices=5, n_ues=25, n_rbs=135, rbs_per_rbg=5, max_ues_slice=10)}
HALF_LN_2PI = pr.HALF_LN_2PI
LN_1E9 = 20.72326583694641
EPISODE_LENGTHS = (5, 7, 8, 12, 24, 6)      # per env, cyclic: episodes end at different TTIs, several at TTI 24 (the call's last)


def mlp(dims, act, seed):
    g = torch.Generator().manual_seed(seed)
    mods = []
    for i in range(len(dims) - 1):
        lin = torch.nn.Linear(dims[i], dims[i + 1])
        with torch.no_grad():
            bound = 1.0 / np.sqrt(dims[i])
            lin.weight.copy_((torch.rand(lin.weight.shape, generator=g) * 2 - 1) * bound)
            lin.bias.copy_((torch.rand(lin.bias.shape, generator=g) * 2 - 1) * bound)
        mods.append(lin)
        if i < len(dims) - 2:
            mods.append(torch.nn.Tanh() if act == "tanh" else torch.nn.ReLU())
    return torch.nn.Sequential(*mods)


def nets(S, Us, widths, intra_input="obs", seed=5):
    """(inter actor, intra actor, inter critic, intra critic): tanh inter nets, relu intra nets, critics of the actors' widths."""
    n_in = 2 * Us + 9 + (Us if intra_input == "mask_obs" else 0)
    return (mlp([10 * S] + widths + [2 * S], "tanh", seed), mlp([n_in] + widths + [3], "relu", seed + 1),
            mlp([10 * S] + widths + [1], "tanh", seed + 2), mlp([n_in] + widths + [1], "relu", seed + 3))


def make_env(size, net, B, stochastic=True, seed=11, autoreset=False, parts=1, se_mode="stream", intra_input="obs", intra=True,
             critics=True, intra_critic=True, trace_len=64):
    """A reset env under the policy nets (and critics) of (size, net).  autoreset: per-env episode lengths EPISODE_LENGTHS."""
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    wl = make_mult_slice_workload(B, torch.device("cuda", 0), policy=_lib.POLICY_MAPF, intra=_lib.INTRA_PF, n_scenarios=8, n_traces=8,
                                  trace_len=trace_len, max_steps=1000, **SIZES[size])
    env = wl.env
    a_inter, a_intra, v_inter, v_intra = nets(env.S, env.Us, NETS[net], intra_input)
    env.set_se_mode(se_mode)
    env.set_policy_network(a_inter, a_intra if intra else None, stochastic=stochastic, seed=seed, intra_input=intra_input)
    if critics:
        env.set_value_network(v_inter, v_intra if (intra and intra_critic) else None)
    if autoreset:
        eps = env.episodes
        env.set_episode_table(scenario=eps["scenario"], se_base=eps["se_base"], se_len=eps["se_len"], se_offset=eps["se_offset"],
                              trf_base=eps["trf_base"], trf_len=eps["trf_len"], trf_offset=eps["trf_offset"])
        env.set_max_steps(np.asarray(EPISODE_LENGTHS, dtype=np.int32)[np.arange(B) % len(EPISODE_LENGTHS)])
        env.enable_autoreset(0, B, episode_numbers=np.arange(B, dtype=np.int32))
    if parts > 1:
        env.set_partitions(parts)
    env.reset()
    return wl, env, (a_inter, a_intra if intra else None, v_inter if critics else None, v_intra if (critics and intra and intra_critic) else None)


def layers_of(net):
    from intent_radio_sched_multi_slice_amd.batched_env import policy_net_layers
    return policy_net_layers(net)


def check_values(vf, obs_inter, obs_intra, mask_intra, v_inter, v_intra, layout="obs", what="vf"):
    """vf [B, S+1] against the critics on the given observations; returns the worst error / bound ratio."""
    vf = pr._np(vf)
    B, S = vf.shape[0], vf.shape[1] - 1
    y, t = pr.mlp64(pr._np(obs_inter, np.float32), *layers_of(v_inter))
    y, t = y[:, 0], t[:, 0]
    bound = t + 2.0 ** -24 * np.abs(y)
    err = np.abs(vf[:, 0] - y)
    assert np.all(err <= bound), f"{what}: inter value outside its bound: worst {np.max(err / bound):.3g} of the bound"
    worst = float(np.max(err / bound))
    if v_intra is None:
        assert np.all(vf[:, 1:] == 0.0), f"{what}: intra columns without an intra critic are not 0"
        return worst
    y, t = pr.mlp64(pr.intra_input(obs_intra, mask_intra, layout), *layers_of(v_intra))
    y, t = y[:, 0].reshape(B, S), t[:, 0].reshape(B, S)
    bound = t + 2.0 ** -24 * np.abs(y)
    err = np.abs(vf[:, 1:] - y)
    assert np.all(err <= bound), f"{what}: intra value outside its bound: worst {np.max(err / bound):.3g} of the bound"
    return max(worst, float(np.max(err / bound)))


def check_actor_record(rec, t, a_inter, a_intra, stochastic, seed, episode, step, layout="obs"):
    """Slot t of a record (dict of numpy arrays) against the float64 actors: action_inter before the clamp, both log-probabilities.
    ``episode`` / ``step``: [B] Philox counters of that TTI.  Returns the worst error / bound ratios and the number of all-masked rows."""
    obs, mask = rec["obs_inter"][t], rec["mask_inter"][t]
    B, S = mask.shape
    out, out_t = pr.mlp64(obs, *layers_of(a_inter))
    mean, ls, t_mean, t_ls = out[:, :S], out[:, S:], out_t[:, :S], out_t[:, S:]
    active = pr.sorted_mask(mask)
    z = np.zeros_like(mean)
    bound = t_mean.copy()
    if stochastic:
        z = pr.gauss_noise(pr.POLICY_TAG, np.arange(B), episode, step, S, seed)
        sd = np.exp(ls)
        mean = mean + sd * z
        bound = bound + sd * np.abs(z) * np.expm1(t_ls) + 1e-12 * (1.0 + sd * np.abs(z))
    act = rec["action_inter"][t]
    assert np.all(act[~active] == -1.0), "a masked position of action_inter is not exactly -1"
    err = np.abs(act - mean)
    assert np.all(err[active] <= bound[active]), f"slot {t}: action_inter outside its bound"
    ratios = {"action_inter": float(np.max(err[active] / bound[active])) if active.any() else 0.0}
    # inter log-probability
    zz = np.where(active, z, 0.0)
    terms = np.where(active, -0.5 * zz * zz - ls - HALF_LN_2PI, 0.0)
    n_masked = S - active.sum(axis=1)
    lp = terms.sum(axis=1) + n_masked * (LN_1E9 - HALF_LN_2PI)
    lp_bound = np.where(active, t_ls, 0.0).sum(axis=1) + 1e-12 * S * (1.0 + np.max(zz * zz, axis=1)) + 2.0 ** -24 * np.abs(lp)
    got = rec["logp"][t][:, 0].astype(np.float64)
    err = np.abs(got - lp)
    assert np.all(err <= lp_bound), f"slot {t}: inter logp outside its bound: worst {np.max(err / lp_bound):.3g}"
    ratios["logp_inter"] = float(np.max(err / lp_bound))
    all_masked = n_masked == S
    if all_masked.any():
        assert np.all(rec["logp"][t][all_masked, 0] == np.float32(S * (LN_1E9 - HALF_LN_2PI))), "all-masked row: not the constant"
    if a_intra is None:
        assert np.all(rec["logp"][t][:, 1:] == 0.0)
        return ratios, int(all_masked.sum())
    lg, lg_t = pr.mlp64(pr.intra_input(rec["obs_intra"][t], rec["mask_intra"][t], layout), *layers_of(a_intra))
    lg, lg_t = lg.reshape(B, S, 3), lg_t.reshape(B, S, 3)
    ch = rec["action_intra"][t].astype(np.int64)
    assert ch.min() >= 0 and ch.max() <= 2
    mx = lg.max(axis=-1)
    lpi = np.take_along_axis(lg, ch[..., None], -1)[..., 0] - mx - np.log(np.exp(lg - mx[..., None]).sum(axis=-1))
    b = 2.0 * lg_t.max(axis=-1) + 1e-12 + 2.0 ** -24 * np.abs(lpi)
    err = np.abs(rec["logp"][t][:, 1:].astype(np.float64) - lpi)
    assert np.all(err <= b), f"slot {t}: intra logp outside its bound: worst {np.max(err / b):.3g}"
    ratios["logp_intra"] = float(np.max(err / b))
    return ratios, int(all_masked.sum())
