"""SAC's soft Bellman target on the device (ranenv_set_sac_critics / ranenv_sac_targets, include/ranenv.h) against the float64
reference and its derived bounds (tests/sac_ref.py; tests/test_sac_cpu.py holds the shared inputs to their conditions), the exact
properties -- terminal rows, the mode, prefixes, optional outputs, independent weight buffers -- and the error rules through the C ABI."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import head_policy_ref as hr
from tests import sac_ref as sr
from tests.gpu_common import need_gpu, to_host

pytestmark = pytest.mark.gpu

SEED, DRAW = 77, 3
SIZE_OF = {5: "S5U25", 10: "S10U100"}


def _env(case, B=8):
    """A small env of the case's S (the targets do not touch its state) with the case's actor and critics bound."""
    S = sr.CASES[case][0]
    _, env, _ = hr.make_env(SIZE_OF[S], "64x64", "gauss_tanh", B, bind=False)
    actor, q1, q2 = sr.sac_nets(case)
    env.set_head_policy_network(actor, "gauss_tanh", stochastic=True, seed=1)
    env.set_sac_critics(q1, q2)
    return env, (actor, q1, q2)


@pytest.mark.parametrize("stochastic", [True, False])
@pytest.mark.parametrize("case", sorted(sr.CASES))
def test_targets_lie_inside_the_float64_bounds(case, stochastic):
    need_gpu()
    env, nets = _env(case)
    obs, reward, done = sr.sac_inputs(case)
    n, S = sr.N_ROWS, env.S
    z = sr.noise(n, S, SEED, DRAW) if stochastic else None
    ref = sr.SacRef(obs, reward, done, *nets, sr.GAMMA, sr.ENT_COEF, z)
    args = (torch.as_tensor(obs), torch.as_tensor(reward), torch.as_tensor(done))
    kw = dict(gamma=sr.GAMMA, ent_coef=sr.ENT_COEF, stochastic=stochastic, seed=SEED, draw=DRAW)
    got = to_host(env.sac_targets(*args, **kw))
    assert got["target"].shape == (n,) and got["next_action"].shape == (n, S) and got["next_logp"].shape == (n,) and got["q"].shape == (n, 2)
    for k in ("next_action", "next_logp", "q", "target"):
        v, want, bound = got[k].astype(np.float64), getattr(ref, k), getattr(ref, k + "_bound")
        print(f"{case} stochastic={stochastic} {k}: worst error / bound {np.max(np.abs(v - want) / bound):.3g}, largest bound {bound.max():.3g}")
    sr.check_outputs(ref, got, case)
    d = done != 0
    assert np.array_equal(got["target"][d], reward[d])                      # terminal rows: exactly float32(reward)
    if not stochastic:                                                        # the noise is exactly zero: a' = tanh(mu)
        mu = ref.mu
        assert np.all(np.abs(got["next_action"] - np.tanh(mu)) <= ref.next_action_bound)
        assert np.array_equal(ref.z, np.zeros_like(ref.z))
    # the prefix property: rows are independent
    m = 33
    part = to_host(env.sac_targets(*(a[:m] for a in args), **kw))
    assert all(np.array_equal(part[k], got[k][:m]) for k in got), "prefix"
    # optional outputs set to NULL leave the target as it is
    only = to_host(env.sac_targets(*args, outputs=("target",), **kw))
    assert set(only) == {"target"} and np.array_equal(only["target"], got["target"])
    # another draw / seed: other noise (stochastic), the same values (mode)
    other = to_host(env.sac_targets(*args, **dict(kw, draw=DRAW + 1)))
    assert np.array_equal(other["next_action"], got["next_action"]) != stochastic
    env.close()


@pytest.mark.parametrize("case", ["odd", "256x256"])
def test_the_target_and_the_head_policy_share_one_squashed_gaussian_epilogue(case):
    """The mode of the SAC target's a' on an observation IS the score a deterministic "gauss_tanh" head policy steps with on it: the
    same weights through the same layers, tanh of the same double.  B = 40: one full workgroup of rows and a tail of 8."""
    need_gpu()
    B = 40
    env, _ = _env(case, B)
    env.set_head_policy_network(sr.sac_nets(case)[0], "gauss_tanh", stochastic=False)
    env.reset()
    snapshot = env.head_obs.clone()
    env.step()
    zeros = torch.zeros(B, dtype=torch.float32, device=env.device)
    got = env.sac_targets(snapshot, zeros, zeros.to(torch.uint8), stochastic=False)["next_action"]
    scores = env.policy_actions()["scores"].to(torch.float32)
    torch.cuda.synchronize()
    assert got.shape == (B, env.S) and bool(torch.any(got != 0))
    assert np.array_equal(got.cpu().numpy(), scores.cpu().numpy())
    env.close()


def test_actor_and_critics_keep_buffers_of_their_own():
    need_gpu()
    case = "64x64"
    env, (actor, q1, q2) = _env(case)
    obs, reward, done = sr.sac_inputs(case)
    S = env.S
    args = (torch.as_tensor(obs), torch.as_tensor(reward), torch.as_tensor(done))
    kw = dict(gamma=sr.GAMMA, ent_coef=sr.ENT_COEF, stochastic=True, seed=SEED, draw=DRAW)
    first = to_host(env.sac_targets(*args, **kw))
    # a larger actor (its packed buffer grows): the critics still answer as the reference says
    wide = hr.mlp([10 * S, 128, 128, 2 * S], "tanh", 99, sr.OUT_SCALE)
    env.set_head_policy_network(wide, "gauss_tanh", stochastic=True, seed=1)
    ref = sr.SacRef(obs, reward, done, wide, q1, q2, sr.GAMMA, sr.ENT_COEF, sr.noise(sr.N_ROWS, S, SEED, DRAW))
    got = to_host(env.sac_targets(*args, **kw))
    sr.check_outputs(ref, got, "wide actor")
    assert not np.array_equal(got["q"], first["q"])
    # back to the first actor: bit for bit the first answer; rebinding the critics (swapped) leaves the actor's part as it is
    env.set_head_policy_network(actor, "gauss_tanh", stochastic=True, seed=1)
    back = to_host(env.sac_targets(*args, **kw))
    assert all(np.array_equal(back[k], first[k]) for k in first)
    env.set_sac_critics(q2, q1)
    swapped = to_host(env.sac_targets(*args, **kw))
    assert np.array_equal(swapped["q"], first["q"][:, ::-1]) and np.array_equal(swapped["target"], first["target"])
    assert np.array_equal(swapped["next_action"], first["next_action"]) and np.array_equal(swapped["next_logp"], first["next_logp"])
    env.close()


def test_error_rules():
    need_gpu()
    from intent_radio_sched_multi_slice_amd import _lib
    E_INVALID, E_STATE = -1, -3
    case = "64x64"
    S = sr.CASES[case][0]
    _, env, _ = hr.make_env(SIZE_OF[S], "64x64", "gauss_tanh", 8, bind=False)
    actor, q1, q2 = sr.sac_nets(case)
    lib, h, stream = env._lib, env._h, env._stream()
    keep = []
    mlp = lambda net: env._mlp_struct(*hr.layers_of(net), _lib.NET_IN_OBS, keep)  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    n = 40
    obs, reward, done = (torch.as_tensor(a[:n]).to(env.device) for a in sr.sac_inputs(case))
    target = torch.full((n,), -7.0, dtype=torch.float32, device=env.device)

    def targets(n_=n, o=obs, r=reward, d=done, t=target):
        ptr = lambda x: None if x is None else p(x)  # noqa: E731
        return lib.ranenv_sac_targets(h, n_, ptr(o), ptr(r), ptr(d), 0.99, 0.2, 1, 5, 6, ptr(t), None, None, None, stream)

    # nothing bound; a PPO (GAUSS_CLIP) actor; a SAC actor but no critics
    assert targets() == E_STATE
    clip_actor, log_std, _ = hr.head_nets(S, "64x64", "gauss_clip")
    env.set_head_policy_network(clip_actor, "gauss_clip", log_std)
    assert lib.ranenv_set_sac_critics(h, C.byref(mlp(q1)), C.byref(mlp(q2)), stream) == 0
    assert targets() == E_STATE and b"GAUSS_TANH" in lib.ranenv_last_error(h)
    env.close()
    _, env, _ = hr.make_env(SIZE_OF[S], "64x64", "gauss_tanh", 8, bind=False)
    lib, h, stream = env._lib, env._h, env._stream()
    env.set_head_policy_network(actor, "gauss_tanh")
    assert targets() == E_STATE and b"critics" in lib.ranenv_last_error(h)
    # the critics' shapes
    assert lib.ranenv_set_sac_critics(h, None, C.byref(mlp(q2)), stream) == E_INVALID
    assert lib.ranenv_set_sac_critics(h, C.byref(mlp(q1)), None, stream) == E_INVALID
    obs_only = hr.mlp([10 * S, 64, 64, 1], "tanh", 3)                        # (a value net's input: no action columns)
    two_out = hr.mlp([11 * S, 64, 64, 2], "tanh", 3)
    narrow = hr.mlp([11 * S, 64, 32, 1], "tanh", 3)
    shallow = hr.mlp([11 * S, 64, 1], "tanh", 3)
    relu = hr.mlp([11 * S, 64, 64, 1], "relu", 3)
    wide = [(torch.zeros(1024, 11 * S), torch.zeros(1024)), (torch.zeros(1, 1024), torch.zeros(1))]
    for a, b in ((obs_only, obs_only), (two_out, two_out), (q1, narrow), (q1, shallow), (q1, relu)):
        assert lib.ranenv_set_sac_critics(h, C.byref(mlp(a)), C.byref(mlp(b)), stream) == E_INVALID
    wide_m = env._mlp_struct(wide, "tanh", _lib.NET_IN_OBS, keep)
    assert lib.ranenv_set_sac_critics(h, C.byref(wide_m), C.byref(wide_m), stream) == E_INVALID
    assert targets() == E_STATE                                                # (no refused binding bound anything)
    assert lib.ranenv_set_sac_critics(h, C.byref(mlp(q1)), C.byref(mlp(q2)), stream) == 0
    # the call's arguments
    assert targets(n_=0) == E_INVALID and targets(n_=-3) == E_INVALID
    assert targets(o=None) == E_INVALID and targets(r=None) == E_INVALID and targets(d=None) == E_INVALID and targets(t=None) == E_INVALID
    torch.cuda.synchronize()
    assert bool((target == -7.0).all())                                        # no refusal wrote anything
    assert targets() == 0
    torch.cuda.synchronize()
    want = env.sac_targets(obs, reward, done, gamma=0.99, ent_coef=0.2, stochastic=True, seed=5, draw=6)["target"]
    assert torch.equal(target, want)
    env.close()
