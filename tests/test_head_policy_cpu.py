"""Head policies (RANENV_POLICY_HEAD_NETWORK) without a GPU: the SB3 state-dict readers, the float32 restatements against their
float64 twin (tests/head_policy_ref.py), the header / ctypes agreement, and planted slips that the twin's bound must separate."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from intent_radio_sched_multi_slice_amd import _lib, adapters
from tests import head_policy_ref as hr

S, B, SEED = 5, 77, 0x0123_4567_89AB_CDEF


# ---- 1. SB3 state-dict adapters ---------------------------------------------------------------------------------------------------
class _MlpExtractor(torch.nn.Module):
    def __init__(self, n_in, widths):
        super().__init__()
        def seq():
            mods, d = [], n_in
            for w in widths:
                mods += [torch.nn.Linear(d, w), torch.nn.Tanh()]
                d = w
            return torch.nn.Sequential(*mods)
        self.policy_net, self.value_net = seq(), seq()


class _PpoPolicy(torch.nn.Module):
    """The module layout of SB3's ActorCriticPolicy for a Box action space (separate pi / vf nets)."""

    def __init__(self, n_in, n_act, widths=(64, 64)):
        super().__init__()
        self.mlp_extractor = _MlpExtractor(n_in, widths)
        self.action_net = torch.nn.Linear(widths[-1], n_act)
        self.value_net = torch.nn.Linear(widths[-1], 1)
        self.log_std = torch.nn.Parameter(torch.linspace(-1.0, 0.5, n_act))

    def forward(self, x):
        return self.action_net(self.mlp_extractor.policy_net(x)), self.value_net(self.mlp_extractor.value_net(x))


class _SacActor(torch.nn.Module):
    def __init__(self, n_in, n_act, widths=(256, 256)):
        super().__init__()
        mods, d = [], n_in
        for w in widths:
            mods += [torch.nn.Linear(d, w), torch.nn.ReLU()]
            d = w
        self.latent_pi = torch.nn.Sequential(*mods)
        self.mu, self.log_std = torch.nn.Linear(d, n_act), torch.nn.Linear(d, n_act)


class _SacPolicy(torch.nn.Module):
    def __init__(self, n_in, n_act):
        super().__init__()
        self.actor = _SacActor(n_in, n_act)
        self.critic = torch.nn.Sequential(torch.nn.Linear(n_in + n_act, 8))      # (ignored by the reader)


def test_sb3_ppo_state_dict():
    torch.manual_seed(3)
    pol = _PpoPolicy(10 * S, S)
    actor, log_std, critic = adapters.sb3_ppo_layers(pol.state_dict())
    x = torch.randn(B, 10 * S)
    with torch.no_grad():
        mean, value = pol(x)
    torch.testing.assert_close(adapters._mlp_forward(x, actor, "tanh"), mean)
    torch.testing.assert_close(adapters._mlp_forward(x, critic, "tanh"), value)
    assert torch.equal(log_std, pol.log_std.detach())
    assert [tuple(w.shape) for w, _ in actor] == [(64, 10 * S), (64, 64), (S, 64)]
    sd = dict(pol.state_dict())
    for drop in ("log_std", "action_net.bias", "mlp_extractor.policy_net.2.weight", "value_net.weight"):
        with pytest.raises(ValueError):
            adapters.sb3_ppo_layers({k: v for k, v in sd.items() if k != drop})
    for extra in ("features_extractor.cnn.0.weight", "mlp_extractor.shared_net.0.weight", "mlp_extractor.policy_net.1.weight"):
        with pytest.raises(ValueError):
            adapters.sb3_ppo_layers({**sd, extra: torch.zeros(1)})


def test_sb3_sac_state_dict():
    torch.manual_seed(4)
    pol = _SacPolicy(10 * S, S)
    layers = adapters.sb3_sac_actor_layers(pol.state_dict())
    x = torch.randn(B, 10 * S)
    with torch.no_grad():
        lat = pol.actor.latent_pi(x)
        mu, ls = pol.actor.mu(lat), pol.actor.log_std(lat)
    out = adapters._mlp_forward(x, layers, "relu")
    torch.testing.assert_close(out[:, :S], mu)              # the stacked output is (mu | log_std)
    torch.testing.assert_close(out[:, S:], ls)
    assert [tuple(w.shape) for w, _ in layers] == [(256, 10 * S), (256, 256), (2 * S, 256)]
    sd = dict(pol.state_dict())
    for drop in ("actor.mu.weight", "actor.log_std.bias", "actor.latent_pi.0.bias"):
        with pytest.raises(ValueError):
            adapters.sb3_sac_actor_layers({k: v for k, v in sd.items() if k != drop})
    with pytest.raises(ValueError):
        adapters.sb3_sac_actor_layers({**sd, "actor.features_extractor.0.weight": torch.zeros(1)})


# ---- 2. restatements against the float64 twin -------------------------------------------------------------------------------------
def _case(net, dist, stochastic, rng_seed=7):
    rng = np.random.default_rng(rng_seed)
    obs = hr.injected_head_obs(rng, B, S)
    actor, log_std, critic = hr.head_nets(S, net, dist)
    env_ids, episode, step = np.arange(B) + 1000, rng.integers(0, 50, B), rng.integers(0, 400, B)
    z = hr.noise(env_ids, episode, step, S, SEED) if stochastic else None
    return obs, actor, log_std, critic, (env_ids, episode, step), z


@pytest.mark.parametrize("stochastic", [False, True])
@pytest.mark.parametrize("dist", ["gauss_clip", "gauss_tanh"])
@pytest.mark.parametrize("net", list(hr.NETS))
def test_restatement_within_the_twins_bound(net, dist, stochastic):
    obs, actor, log_std, _, (env_ids, episode, step), z = _case(net, dist, stochastic)
    scores, a = adapters.head_policy_actions(obs, actor, dist, log_std, stochastic, SEED, env_ids=env_ids, episode=episode, step=step)
    ref = hr.HeadRef(obs, actor, dist, log_std, z)
    worst = hr.check_scores(ref, scores, f"{net} {dist}")
    assert np.all(np.abs(a.numpy() - ref.action) <= ref.action_bound)
    # the case is what it claims: the clamp / the tanh / SAC's log_std clamp all act on a share of the entries
    assert (np.abs(ref.action) > 1.0).mean() > 0.05 and (np.abs(ref.action) < 1.0).mean() > 0.05
    if dist == "gauss_tanh":
        raw = hr.pr.mlp64(obs, *hr.layers_of(actor))[0][:, S:]
        assert (raw > 2.0).any() and (raw < 2.0).any()
    if stochastic:
        assert np.array_equal(z, adapters.head_policy_noise(env_ids, episode, step, S, SEED))
    print(f"worst error / bound {worst:.3g}")


@pytest.mark.parametrize("stochastic", [False, True])
def test_logp_restatement(stochastic):
    _, _, log_std, _, _, z = _case("64x64", "gauss_clip", stochastic)
    got = adapters.head_policy_logp(log_std, z, B=B)
    want, bound = hr.logp_ref(log_std, z, B)
    assert got.dtype == np.float32 and got.shape == (B,)
    assert np.all(np.abs(got.astype(np.float64) - want) <= bound)


def test_restatement_argument_errors():
    obs, actor, log_std, _, _, _ = _case("64x64", "gauss_clip", False)
    with pytest.raises(ValueError):
        adapters.head_policy_actions(obs, actor, "gauss_clip", None)
    with pytest.raises(ValueError):
        adapters.head_policy_actions(obs, actor, "gauss_clip", log_std, stochastic=True)      # no counters
    with pytest.raises(ValueError):
        adapters.head_policy_actions(obs, actor, "beta", log_std)
    tanh_actor = hr.head_nets(S, "64x64", "gauss_tanh")[0]
    with pytest.raises(ValueError):
        adapters.head_policy_actions(obs, tanh_actor, "gauss_tanh", log_std)


# ---- 3. header and _lib -----------------------------------------------------------------------------------------------------------
def test_header_and_bindings_agree():
    header = open(os.path.join(REPO, "include", "ranenv.h")).read()
    assert int(re.search(r"#define RANENV_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 10
    assert int(re.search(r"#define RANENV_HEAD_TRAJECTORY_BYTES (\d+)", header).group(1)) == ctypes.sizeof(_lib.HeadTrajectory)
    assert int(re.search(r"#define RANENV_TRAJECTORY_BYTES (\d+)", header).group(1)) == ctypes.sizeof(_lib.Trajectory) == 96
    assert ctypes.sizeof(_lib.Config) == 96
    body = re.search(r"typedef struct \{([^}]*)\} ranenv_head_trajectory;", header).group(1)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert tuple(names) == _lib.HEAD_TRAJECTORY_FIELDS
    assert re.search(r"RANENV_POLICY_HEAD_NETWORK = (\d+)", header).group(1) == str(_lib.POLICY_HEAD_NETWORK) == "4"
    assert re.search(r"RANENV_HEAD_DIST_GAUSS_CLIP = (\d+), RANENV_HEAD_DIST_GAUSS_TANH = (\d+)", header).groups() == \
        (str(_lib.HEAD_DIST_GAUSS_CLIP), str(_lib.HEAD_DIST_GAUSS_TANH))
    assert f"0x{adapters.HEAD_TAG:08X}" in header and adapters.HEAD_TAG == hr.HEAD_TAG
    for name in ("ranenv_set_head_policy_network", "ranenv_set_head_value_network", "ranenv_get_head_metrics", "ranenv_collect_head"):
        assert name in _lib.EXPORTS


# ---- 4. planted slips: the bound separates each of them on these inputs ------------------------------------------------------------
def _slipped_scores(slip, obs, actor, dist, log_std, z):
    """adapters.head_policy_actions with one rule broken."""
    layers, act = hr.layers_of(actor)
    out = adapters._mlp_forward(torch.as_tensor(obs), layers, act).to(torch.float64)
    if dist == "gauss_clip":
        a, ls = out, torch.as_tensor(log_std).to(torch.float64).reshape(1, S)
    else:
        a, ls = out[:, :S], out[:, S:]
        if slip != "log_std_unclamped":
            ls = ls.clamp(-20.0, 2.0)
    if z is not None:
        a = a + torch.exp(ls) * torch.from_numpy(z)
    clip = dist == "gauss_clip"
    if slip == "swapped":
        clip = not clip
    if slip == "no_clamp":
        return a.numpy()
    return (a.clamp(-1.0, 1.0) if clip else torch.tanh(a)).numpy()


SLIPS = [("no_clamp", "gauss_clip", False), ("no_clamp", "gauss_clip", True),
         ("swapped", "gauss_clip", False), ("swapped", "gauss_clip", True), ("swapped", "gauss_tanh", False), ("swapped", "gauss_tanh", True),
         ("log_std_unclamped", "gauss_tanh", True)]


@pytest.mark.parametrize("net", list(hr.NETS))
@pytest.mark.parametrize("slip,dist,stochastic", SLIPS)
def test_planted_slips_are_separated(net, slip, dist, stochastic):
    """Each slip, planted into a copy of the restatement, leaves the twin's bound on these inputs for SB3's two default shapes
    ([64, 64] tanh, [256, 256] relu: score bounds below 0.01 in the mode).  For [512] x 3 the rigorous bound is 0.27 at these
    magnitudes (three layers of 512 worst-case sums), wider than clamp and tanh ever differ (0.24), so there the slips are shown
    to leave the 1e-5 the GPU tests allow against the float32 restatement -- which every net must meet as well."""
    obs, actor, log_std, _, _, z = _case(net, dist, stochastic)
    ref = hr.HeadRef(obs, actor, dist, log_std, z)
    good = _slipped_scores(None, obs, actor, dist, log_std, z)
    assert np.all(np.abs(good - ref.scores) <= ref.score_bound)            # (the copy itself is right)
    bad = _slipped_scores(slip, obs, actor, dist, log_std, z)
    with np.errstate(invalid="ignore"):
        assert (~(np.abs(bad - good) <= 1e-5)).any(), f"{slip} stays within 1e-5 of the restatement"
        outside = ~(np.abs(bad - ref.scores) <= ref.score_bound)           # (inf - inf = nan counts as outside)
    if net != "512x3":
        assert outside.any(), f"{slip} stays within the bound"
        with pytest.raises(AssertionError):
            hr.check_scores(ref, bad)


@pytest.mark.parametrize("stochastic", [False, True])
def test_a_masked_term_in_logp_exceeds_the_bound(stochastic):
    """IBSched's masked-position term (n_masked (ln 1e9 - 0.5 ln 2 pi) in place of those positions' own terms) must not appear."""
    _, _, log_std, _, _, z = _case("64x64", "gauss_clip", stochastic)
    want, bound = hr.logp_ref(log_std, z, B)
    rng = np.random.default_rng(5)
    n_masked = rng.integers(1, S, B)
    active = np.arange(S)[None, :] >= n_masked[:, None]
    zz = np.zeros((B, S)) if z is None else z
    ls = log_std.numpy().astype(np.float64)
    slipped = np.where(active, (-0.5 * zz) * zz - ls[None, :] - adapters.HALF_LN_2PI, 0.0).sum(axis=1) + n_masked * (adapters.LN_1E9 - adapters.HALF_LN_2PI)
    assert np.all(np.abs(slipped.astype(np.float32).astype(np.float64) - want) > bound)
