"""RANENV_POLICY_NETWORK without a GPU: the net validation of set_policy_network (batched_env.policy_net_layers), the RLlib
checkpoint reader, properties of the torch restatement the device is tested against, and the library's new exports."""
from __future__ import annotations

import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from intent_radio_sched_multi_slice_amd import _lib, adapters
from intent_radio_sched_multi_slice_amd.batched_env import policy_net_layers


def _seq(dims, act=torch.nn.Tanh):
    mods = []
    for i in range(len(dims) - 1):
        mods.append(torch.nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            mods.append(act())
    return torch.nn.Sequential(*mods)


def test_layers_from_sequential_and_pairs():
    net = _seq([100, 64, 64, 20], torch.nn.ReLU)
    layers, act = policy_net_layers(net, in_dim=100, out_dim=20)
    assert act == "relu" and [tuple(w.shape) for w, _ in layers] == [(64, 100), (64, 64), (20, 64)]
    assert all(w.dtype == torch.float32 and b.dtype == torch.float32 for w, b in layers)
    pairs = [(np.ones((8, 4)), np.zeros(8)), (np.ones((3, 8)), np.zeros(3))]
    layers, act = policy_net_layers(pairs)
    assert act == "tanh" and len(layers) == 2
    assert policy_net_layers(pairs, activation="relu")[1] == "relu"
    assert len(policy_net_layers(_seq([41, 512, 512, 512, 512, 3]), in_dim=41, out_dim=3)[0]) == 5


@pytest.mark.parametrize("net, kw, msg", [
    (_seq([100, 513, 20]), {}, "hidden width 513"),
    (_seq([100, 20]), {}, "0 hidden layers"),
    (_seq([100, 8, 8, 8, 8, 8, 20]), {}, "5 hidden layers"),
    (_seq([101, 64, 20]), {"in_dim": 100}, "input width 101"),
    (_seq([100, 64, 21]), {"out_dim": 20}, "output width 21"),
    ([(np.ones((8, 4)), np.zeros(8)), (np.ones((3, 8)), np.zeros(3))], {"activation": "gelu"}, "unknown activation"),
    ([(np.ones((8, 4)), np.zeros(8)), (np.ones((3, 7)), np.zeros(3))], {}, "input width 7"),
    ([(np.ones((8, 4)), np.zeros(7)), (np.ones((3, 8)), np.zeros(3))], {}, "bias"),
    (torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.GELU(), torch.nn.Linear(8, 3)), {}, "unexpected module GELU"),
    (torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.Tanh(), torch.nn.Linear(8, 8), torch.nn.ReLU(), torch.nn.Linear(8, 3)), {},
     "one activation"),
    (torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.Tanh()), {}, "ends with a Linear"),
])
def test_layers_validation(net, kw, msg):
    with pytest.raises(ValueError, match=msg):
        policy_net_layers(net, **kw)


def _fcnet_state_dict(dims, prefix="internal_model."):
    sd = {}
    for i in range(len(dims) - 2):
        sd[f"{prefix}_hidden_layers.{i}._model.0.weight"] = torch.randn(dims[i + 1], dims[i])
        sd[f"{prefix}_hidden_layers.{i}._model.0.bias"] = torch.randn(dims[i + 1])
    sd[f"{prefix}_logits._model.0.weight"] = torch.randn(dims[-1], dims[-2])
    sd[f"{prefix}_logits._model.0.bias"] = torch.randn(dims[-1])
    return sd


def test_rllib_fcnet_loader():
    sd = _fcnet_state_dict([100, 256, 256, 20])
    sd["internal_model._value_branch._model.0.weight"] = torch.randn(1, 256)      # not the actor: skipped
    sd["internal_model._value_branch._model.0.bias"] = torch.randn(1)
    sd["other_model.whatever"] = torch.randn(3)                                     # outside the prefix: ignored
    layers = adapters.rllib_fcnet_layers(sd)
    assert [tuple(w.shape) for w, _ in layers] == [(256, 100), (256, 256), (20, 256)]
    assert torch.equal(layers[1][0], sd["internal_model._hidden_layers.1._model.0.weight"])
    assert torch.equal(layers[2][1], sd["internal_model._logits._model.0.bias"])
    policy_net_layers(layers, in_dim=100, out_dim=20)
    assert len(adapters.rllib_fcnet_layers(_fcnet_state_dict([41, 64, 3], prefix=""), prefix="")) == 2
    bad = dict(_fcnet_state_dict([100, 64, 20]))
    bad["internal_model._append_free_log_std.log_std"] = torch.zeros(10)
    with pytest.raises(ValueError, match="not a FullyConnectedNetwork key"):
        adapters.rllib_fcnet_layers(bad)
    sd = _fcnet_state_dict([100, 64, 64, 20])
    del sd["internal_model._hidden_layers.0._model.0.bias"]
    with pytest.raises(ValueError, match="incomplete"):
        adapters.rllib_fcnet_layers(sd)
    with pytest.raises(ValueError, match="no FullyConnectedNetwork"):
        adapters.rllib_fcnet_layers({"internal_model._hidden_layers.0._model.0.weight": torch.zeros(2, 2)})


def _inputs(B=64, S=5, Us=10, seed=0):
    g = torch.Generator().manual_seed(seed)
    obs_inter = torch.rand(B, 10 * S, generator=g) * 2 - 1
    mask = (torch.rand(B, S, generator=g) > 0.4).to(torch.int8)
    obs_intra = torch.rand(B, S, 2 * Us + 9, generator=g)
    mask_intra = (torch.rand(B, S, Us, generator=g) > 0.5).to(torch.int8)
    return obs_inter, mask, obs_intra, mask_intra


@pytest.mark.parametrize("stochastic", [False, True])
def test_restatement_scores_masked_and_bounded(stochastic):
    B, S = 64, 5
    obs_inter, mask, obs_intra, mask_intra = _inputs(B, S)
    inter = _seq([10 * S, 64, 64, 2 * S])
    with torch.no_grad():
        inter[-1].weight.mul_(20.0)              # means and log-stds far outside [-1, 1]: the clamp must hold
        inter[-1].bias.fill_(0.5)
    scores, intra = adapters.ibsched_policy_actions(obs_inter, mask, inter, stochastic=stochastic, seed=4, env_ids=np.arange(B),
                                                    episode=np.zeros(B), step=np.full(B, 3))
    assert intra is None and scores.dtype == torch.float64 and scores.shape == (B, S)
    smask = adapters.sorted_action_mask(mask)
    assert torch.all(scores[smask == 0] == -1.0)
    assert torch.all(scores.abs() <= 1.0)
    assert (scores[smask != 0].abs() < 1.0).any()
    n = mask.to(torch.int64).sum(1)
    for b in range(B):                           # the sorted mask: the last n_active positions
        assert smask[b].tolist() == [0] * (S - int(n[b])) + [1] * int(n[b])


def test_restatement_argmax_ties_go_to_lowest_index():
    B, S, Us = 4, 5, 10
    obs_inter, mask, obs_intra, mask_intra = _inputs(B, S, Us)
    inter = _seq([10 * S, 64, 2 * S])
    intra = _seq([2 * Us + 9, 8, 3])
    with torch.no_grad():                        # logits = the output bias: [1, 1, 0] then [0, 2, 2] then [3, 3, 3]
        intra[-1].weight.zero_()
        for bias, want in (([1.0, 1.0, 0.0], 0), ([0.0, 2.0, 2.0], 1), ([3.0, 3.0, 3.0], 0), ([0.0, 1.0, 5.0], 2)):
            intra[-1].bias.copy_(torch.tensor(bias))
            _, ch = adapters.ibsched_policy_actions(obs_inter, mask, inter, obs_intra, mask_intra, intra)
            assert ch.dtype == torch.uint8 and torch.all(ch == want), (bias, ch)


def test_restatement_intra_layouts_and_draws():
    B, S, Us = 32, 5, 10
    obs_inter, mask, obs_intra, mask_intra = _inputs(B, S, Us)
    inter = _seq([10 * S, 64, 2 * S])
    intra = _seq([3 * Us + 9, 64, 3])
    kw = dict(env_ids=np.arange(B), episode=np.arange(B) % 3, step=np.full(B, 7))
    _, ch = adapters.ibsched_policy_actions(obs_inter, mask, inter, obs_intra, mask_intra, intra, intra_input="mask_obs")
    x = torch.cat([mask_intra.float(), obs_intra], dim=-1)
    with torch.no_grad():
        assert torch.equal(ch.long(), intra(x).argmax(-1))
    a = adapters.ibsched_policy_actions(obs_inter, mask, inter, obs_intra, mask_intra, intra, True, 5, "mask_obs", **kw)
    b = adapters.ibsched_policy_actions(obs_inter, mask, inter, obs_intra, mask_intra, intra, True, 5, "mask_obs", **kw)
    c = adapters.ibsched_policy_actions(obs_inter, mask, inter, obs_intra, mask_intra, intra, True, 6, "mask_obs", **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    with pytest.raises(ValueError, match="intra_input"):
        adapters.ibsched_policy_actions(obs_inter, mask, inter, obs_intra, mask_intra, intra, intra_input="dict")


def test_restatement_noise_is_the_documented_philox_box_muller():
    """z and the categorical uniform restated with the oracle's own Philox-4x32-10 (include/ranenv.h)."""
    from oracle import pyoracle
    B, S = 16, 5
    obs_inter, mask, _, _ = _inputs(B, S)
    mask[:] = 1
    inter = _seq([10 * S, 64, 2 * S])
    with torch.no_grad():
        inter[-1].weight.zero_()
        inter[-1].bias.copy_(torch.tensor([0.0] * S + [-3.0] * S))      # mean 0, std e^-3: no clamp
    seed = (9 << 32) | 77
    ep, st = np.arange(B) % 4, np.arange(B) + 2
    scores, _ = adapters.ibsched_policy_actions(obs_inter, mask, inter, stochastic=True, seed=seed, env_ids=np.arange(B) + 100,
                                                episode=ep, step=st)
    o = pyoracle.philox4x32_10((np.arange(B) + 100)[:, None], ep[:, None], st[:, None], 0x504F4C00 + np.arange(S)[None, :], 77, 9)
    u1 = (np.asarray(o[0], dtype=np.float64) + 1.0) / 2.0 ** 32
    u2 = np.asarray(o[1], dtype=np.float64) / 2.0 ** 32
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2 * np.pi * u2)
    np.testing.assert_allclose(scores.numpy(), np.exp(-3.0) * z, rtol=1e-12, atol=1e-15)


def test_exports_and_constants():
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "ranenv.h")).read()
    for name in ("ranenv_set_policy_network", "ranenv_get_policy_actions"):
        assert name + "(" in hdr and name in _lib.EXPORTS
    assert re.search(r"RANENV_POLICY_NETWORK = 3", hdr) and _lib.POLICY_NETWORK == 3
    assert _lib.C.sizeof(_lib.Mlp) == 16 + 24 + 80


def test_policy_kernel_resources():
    """The rebuilt library holds the policy kernel: MFMA accumulators in VGPRs (no AGPRs), no scratch, no spills."""
    from intent_radio_sched_multi_slice_amd.csrc import build as hip_build
    sys.path.insert(0, os.path.join(os.path.dirname(_lib._HERE), "tools"))
    import kernel_resources
    hip_build.build()
    ks = [k for k in kernel_resources.kernel_resources() if "ranenv_policy_kernel" in k["name"]]
    assert len(ks) == 1, [k["name"] for k in ks]
    k = ks[0]
    assert k.get("agpr_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0 and k.get("vgpr_spill_count", 0) == 0, k
