"""Fixtures of the tests of the head policy source "inter" (ranenv_set_head_policy_source, include/ranenv.h): the reference's IBSchedSB3
(agents/sb3_sched.py, agents/sb3_pf_sched.py), an SB3 actor on IBSched's own player_0 observation.  The float64 twin, the nets and
the sizes are those of tests/head_policy_ref.py, evaluated on ``env.obs_inter``; what differs is the env: SORTED scenario tables
(IBSched's default, enable_sort_slices=True -- a slip between sorted position and slice index only shows there), head outputs bound
or not, round-robin or proportional fair inside the slices."""
from __future__ import annotations

import numpy as np
import torch

from tests import head_policy_ref as hr

B = 48                    # a policy workgroup of 32 rows and a tail of 16
SIZES = hr.SIZES
NETS = ("64x64", "256x256")       # SB3's PPO (tanh) and SAC (relu) defaults
DIST_OF = {"64x64": "gauss_clip", "256x256": "gauss_tanh"}
EPISODE_LENGTHS = hr.EPISODE_LENGTHS


def make_env(size, net, dist, batch=B, stochastic=True, seed=11, autoreset=False, parts=1, se_mode="stream", critic=True, metrics=None,
             heads=False, intra=None, trace_len=64, bind=True, observation="inter"):
    """A reset env on sorted scenario tables (S = 1 has nothing to sort) under the head nets of (size, net, dist; ``size`` as for hr.size_of) with ``observation`` as their source.
    ``heads``: head outputs bound as well (enable_heads, before the nets).  ``intra``: fixed_intra (None: round-robin).
    autoreset: per-env episode lengths EPISODE_LENGTHS.  Returns (workload, env, (actor, log_std, critic))."""
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    wl = make_mult_slice_workload(batch, torch.device("cuda", 0), policy=_lib.POLICY_MAPF, intra=_lib.INTRA_RR, n_scenarios=8, n_traces=8,
                                  trace_len=trace_len, max_steps=1000, **hr.size_of(size))
    env = wl.env
    ss = np.asarray(wl.tables.sorted_slices)
    assert ss.shape[-1] == 1 or not np.array_equal(ss, np.broadcast_to(np.arange(ss.shape[-1]), ss.shape)), "the tables do not sort the slices"
    env.set_se_mode(se_mode)
    if heads or observation == "head":
        env.enable_heads(hr.usecase_of(wl.tables))
    actor, log_std, vnet = hr.head_nets(env.S, net, dist)
    if bind:
        env.set_head_policy_network(actor, dist, log_std, stochastic=stochastic, seed=seed, fixed_intra=intra, observation=observation,
                                    allow_sorted=True)
        if critic:
            env.set_head_value_network(vnet)
    if autoreset:
        eps = env.episodes
        env.set_episode_table(scenario=eps["scenario"], se_base=eps["se_base"], se_len=eps["se_len"], se_offset=eps["se_offset"],
                              trf_base=eps["trf_base"], trf_len=eps["trf_len"], trf_offset=eps["trf_offset"])
        env.set_max_steps(np.asarray(EPISODE_LENGTHS, dtype=np.int32)[np.arange(batch) % len(EPISODE_LENGTHS)])
        env.enable_autoreset(0, batch, episode_numbers=np.arange(batch, dtype=np.int32))
    if metrics is not None:
        env.enable_metrics(metrics)
    if parts > 1:
        env.set_partitions(parts)
    env.reset()
    return wl, env, (actor, log_std, vnet)


def counters(env):
    """(episode_number, step_number) of every env now, as numpy copies: the Philox counters of the next TTI's noise."""
    v = env.views()
    return v["episode_number"].cpu().numpy().copy(), v["step_number"].cpu().numpy().copy()


def outside_bound(ref: hr.HeadRef, scores):
    """bool [B]: the envs with a score outside the twin's bound at some position."""
    return (np.abs(np.asarray(scores) - ref.scores) > ref.score_bound).any(axis=1)
