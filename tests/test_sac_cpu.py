"""The off-policy (SAC) data path without a GPU: the torch restatement of ranenv_sac_targets against the float64 reference and its
derived bounds (tests/sac_ref.py), the conditions the shared test inputs must meet, planted slips, the sampler's index rule in numpy,
and the new exports of the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from intent_radio_sched_multi_slice_amd import _lib, adapters
from tests import sac_ref as sr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("ranenv_bind_replay", "ranenv_collect_replay", "ranenv_get_replay_count", "ranenv_replay_sample", "ranenv_set_sac_critics",
               "ranenv_sac_targets")
SEED, DRAW = 77, 3


@pytest.fixture(scope="module", params=sorted(sr.CASES))
def case(request):
    """One CASES entry: its inputs and nets, the stochastic reference and the torch restatement (computed once, never modified)."""
    name = request.param
    obs, reward, done = sr.sac_inputs(name)
    actor, q1, q2 = sr.sac_nets(name)
    S = sr.CASES[name][0]
    z = sr.noise(sr.N_ROWS, S, SEED, DRAW)
    ref = sr.SacRef(obs, reward, done, actor, q1, q2, sr.GAMMA, sr.ENT_COEF, z)
    got = adapters.sac_targets_torch(obs, reward, done, actor, q1, q2, sr.GAMMA, sr.ENT_COEF, True, SEED, DRAW)
    return dict(name=name, S=S, obs=obs, reward=reward, done=done, nets=(actor, q1, q2), z=z, ref=ref, got=got)


def test_torch_restatement_lies_inside_the_reference_bounds(case):
    sr.check_outputs(case["ref"], case["got"], case["name"])
    d = case["done"] != 0
    assert np.array_equal(case["got"]["target"].numpy()[d], case["reward"][d])      # terminal rows: exactly float32(reward)
    obs, reward, done = case["obs"], case["reward"], case["done"]
    mode = adapters.sac_targets_torch(obs, reward, done, *case["nets"], sr.GAMMA, sr.ENT_COEF, False)
    ref0 = sr.SacRef(obs, reward, done, *case["nets"], sr.GAMMA, sr.ENT_COEF, None)
    sr.check_outputs(ref0, mode, case["name"] + " (mode)")
    assert np.all(mode["z"].numpy() == 0.0)
    assert np.array_equal(mode["next_action"].numpy(), np.tanh(mode["mu"].numpy()).astype(np.float32))


def test_torch_restatement_agrees_with_torch_distributions(case):
    """The log-probability through torch.distributions.Normal on the kept pre-tanh sample, SB3's SquashedDiagGaussianDistribution."""
    got = case["got"]
    mu, ls, z = got["mu"], got["log_std"], got["z"]
    sd = torch.exp(ls)
    g = mu + sd * z
    a = torch.tanh(g)
    want = torch.distributions.Normal(mu, sd).log_prob(g).sum(-1) - torch.log(1 - a ** 2 + 1e-6).sum(-1)
    assert want.dtype == torch.float64
    assert torch.all(torch.abs(got["logp64"] - want) <= 1e-9 * (1.0 + torch.abs(want)))
    assert np.array_equal(got["next_logp"].numpy(), got["logp64"].numpy().astype(np.float32))


def test_conditions_on_the_test_inputs(case):
    ref = case["ref"]
    d = ref.done
    assert d.mean() >= 0.10 and (~d).mean() >= 0.10
    assert (ref.log_std_raw > 2.0).mean() >= 0.05 and (ref.log_std == 2.0).mean() >= 0.05
    assert (ref.log_std_raw < -20.0).sum() >= 1 and (ref.log_std == -20.0).sum() >= 1
    assert (np.abs(ref.next_action) > 0.999).mean() >= 0.05
    assert (ref.target_bound < 1e-3 * (1.0 + np.abs(ref.target))).mean() >= 0.99


@pytest.mark.parametrize("slip", sr.SLIPS)
def test_planted_slips_leave_the_bound(case, slip):
    """Each slip, applied to the reference, puts at least half of the rows it can touch outside the bound of the (correct) restatement."""
    ref, got = case["ref"], case["got"]
    bad = sr.SacRef(case["obs"], case["reward"], case["done"], *case["nets"], sr.GAMMA, sr.ENT_COEF, case["z"], slip=slip)
    live = ~ref.done
    eligible = {"sum_not_min": live, "no_entropy": live, "through_done": ref.done,
                # the epsilon matters where 1 - a^2 comes near it: a position with |g| > 6 has 1 - a^2 < 2.5e-5
                "no_epsilon": live & (np.abs(ref.g) > 6.0).any(axis=1),
                "unclamped_log_std": live & ((ref.log_std_raw > 2.0) | (ref.log_std_raw < -20.0)).any(axis=1)}[slip]
    assert eligible.sum() >= 4, (slip, int(eligible.sum()))
    out = sr.outside(got["target"], bad.target, bad.target_bound) | ~np.isfinite(bad.target)
    assert out[eligible].mean() >= 0.5, (slip, float(out[eligible].mean()))


def test_sampler_index_rule():
    B, C = 48, 7
    idx = adapters.replay_sample_index(1 << 16, 5, 2, written=C + 4, capacity=C, B=B)
    assert idx.min() >= 0 and idx.max() < C * B
    assert np.bincount(idx, minlength=C * B).min() >= 1                      # every cell of the full ring is hit
    part = adapters.replay_sample_index(4096, 5, 2, written=3, capacity=C, B=B)
    assert part.max() < 3 * B and (part // B).max() == 2                     # a part-filled ring: no index reaches slot `written`
    assert np.array_equal(adapters.replay_sample_index(100, 5, 2, 3, C, B), part[:100])
    assert not np.array_equal(adapters.replay_sample_index(100, 5, 3, 3, C, B), part[:100])
    # the rule itself on one row, with Python integers
    o = adapters.philox4x32_10(9, 0, 2, 0, 5, 0)
    u = int(o[1]) << 32 | int(o[0])
    assert adapters.replay_sample_index(10, 5, 2, C, C, B)[9] == (u * (C * B)) >> 64


def test_header_binding_and_library_agree_on_the_new_exports():
    from intent_radio_sched_multi_slice_amd.csrc import build as hip_build
    with open(os.path.join(REPO, "include", "ranenv.h")) as f:
        hdr = f.read()
    assert re.search(r"#define\s+RANENV_ABI_VERSION\s+10\b", hdr) and _lib.ABI_VERSION == 10
    lib = ctypes.CDLL(hip_build.build())
    for name in NEW_EXPORTS:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name
        assert name in _lib.FUNCTIONS and hasattr(lib, name), name
    assert ctypes.sizeof(_lib.Replay) == int(re.search(r"#define\s+RANENV_REPLAY_BYTES\s+(\d+)", hdr).group(1)) == 48
    assert lib.ranenv_abi_version() == 10
