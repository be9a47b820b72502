"""Off-policy collection on the device (ranenv_collect_replay / ranenv_replay_sample, include/ranenv.h): the replay ring against a
per-TTI step() loop on a twin env -- wrap-around, terminal observations, partitions, both distributions, both SE modes -- the state
a rollout leaves, the sampler against the numpy index rule, and the error rules straight through the C ABI.  All comparisons exact."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import head_policy_ref as hr
from tests.gpu_common import HEAD_OUTPUTS, LOOSE_WINDOWS_AND_SE, OUTPUTS, assert_same_state, need_gpu

pytestmark = pytest.mark.gpu

B, CAP, T = 48, 7, 5          # a 16-row tail workgroup; two calls of 5 TTIs: the second wraps
SEED = 0x1234_5678_9ABC
SENTINEL = {"obs": -7.0, "next_obs": -7.0, "action": -7.0, "reward_head": -7.0, "done": 255}
# (size, dist, stochastic, autoreset, se_mode)
CONFIGS = [(size, dist, True, ar, "stream") for size in hr.SIZES for dist in ("gauss_clip", "gauss_tanh") for ar in (False, True)]
CONFIGS += [("S5U25", "gauss_tanh", True, True, "gather"), ("S5U25", "gauss_tanh", False, True, "stream")]


_state_equal = functools.partial(assert_same_state, loose=LOOSE_WINDOWS_AND_SE, outputs=OUTPUTS + HEAD_OUTPUTS, actions=("scores",),
                                 metrics={"head_episode_metrics": ("running", "episode_log"), "episode_metrics": ("running", "episode_log")})


def _bound_ring(env, cap=CAP):
    ring = env.bind_replay(cap)
    for k, t in ring.items():
        t.fill_(SENTINEL[k])
    return ring


def _step_loop(ref, n):
    """The transitions of ``n`` step() calls on ``ref``: what the ring must hold, TTI by TTI."""
    want = {k: [] for k in SENTINEL}
    for _ in range(n):
        want["obs"].append(ref.head_obs.clone())
        ref.step()
        done = ref.done.clone()
        want["action"].append(ref.policy_actions()["scores"].clone())
        want["reward_head"].append(ref.head_reward.clone())
        want["done"].append(done)
        # behind the step: the terminal observation ranenv_autoreset handed out where the episode ended, else the row as it stands
        term = ref.term_head_obs if ref.term_head_obs is not None else ref.head_obs
        want["next_obs"].append(torch.where(done[:, None] != 0, term, ref.head_obs).clone())
    return {k: torch.stack(x) for k, x in want.items()}


@pytest.mark.parametrize("size,dist,stochastic,autoreset,se_mode", CONFIGS)
def test_ring_is_the_step_loop_and_state_is_the_rollouts(size, dist, stochastic, autoreset, se_mode):
    need_gpu()
    kw = dict(stochastic=stochastic, seed=SEED, autoreset=autoreset, se_mode=se_mode, metrics=8, critic=False)
    wl, ref, _ = hr.make_env(size, "64x64", dist, B, **kw)
    want = _step_loop(ref, 2 * T)
    d = want["done"].cpu().numpy()
    if autoreset:       # episodes end inside both calls, at several different TTIs, and never for all envs at once
        assert d[:T].any() and d[T:].any() and not d.all(axis=1).any() and len(set(np.nonzero(d)[0])) >= 4
        assert not torch.equal(want["next_obs"][:-1][want["done"][:-1] != 0], want["obs"][1:][want["done"][:-1] != 0])
    else:
        assert not d.any()
    live = want["done"][:-1] == 0
    assert torch.equal(want["next_obs"][:-1][live], want["obs"][1:][live])
    for parts in (1, 3):
        _, env, _ = hr.make_env(size, "64x64", dist, B, parts=parts, **kw)
        _, roll, _ = hr.make_env(size, "64x64", dist, B, parts=parts, **kw)
        ring = _bound_ring(env)
        assert env.replay_count() == 0
        for call in (1, 2):
            env.collect_replay(T)
            roll.rollout(T)
            torch.cuda.synchronize()
            n = call * T
            assert env.replay_count() == n
            for slot in range(CAP):
                ks = [k for k in range(n) if k % CAP == slot]
                for f, t in ring.items():
                    if ks:      # the latest TTI that went to the slot (the second call's, where it wrapped)
                        assert torch.equal(t[slot], want[f][ks[-1]]), (f, slot, parts, call)
                    else:       # not yet written
                        assert bool((t[slot] == SENTINEL[f]).all()), (f, slot, parts, call)
            _state_equal(env, roll, wl.tables, (parts, call))
        env.step()
        roll.step()
        _state_equal(env, roll, wl.tables, (parts, "one more step"))
        env.close()
        roll.close()
    ref.close()


def test_sampler_follows_the_index_rule_and_gathers_the_rows():
    need_gpu()
    from intent_radio_sched_multi_slice_amd import adapters
    _, env, _ = hr.make_env("S5U25", "64x64", "gauss_tanh", B, stochastic=True, seed=SEED, autoreset=True, critic=False)
    ring = _bound_ring(env)
    n, S = 100, env.S
    for steps, written in ((3, 3), (5, 8)):                     # part-filled, then full (and wrapped)
        env.collect_replay(steps)
        torch.cuda.synchronize()
        assert env.replay_count() == written
        flat = {k: t.reshape((CAP * B,) + t.shape[2:]) for k, t in ring.items()}
        for col, name in enumerate(("twc", "colran")):
            got = {k: t.clone() for k, t in env.replay_sample(n, seed=9, draw=4, reward=name).items()}
            idx = adapters.replay_sample_index(n, 9, 4, written, CAP, B)
            assert np.array_equal(got["index"].cpu().numpy(), idx)
            assert idx.max() < min(written, CAP) * B
            ix = torch.as_tensor(idx, device=env.device)
            assert torch.equal(got["obs"], flat["obs"][ix]) and torch.equal(got["next_obs"], flat["next_obs"][ix])
            assert torch.equal(got["done"], flat["done"][ix])
            assert torch.equal(got["action"], flat["action"][ix].to(torch.float32))
            assert torch.equal(got["reward"], flat["reward_head"][ix, col].to(torch.float32))
            assert not bool((got["obs"] == SENTINEL["obs"]).any()) and got["action"].shape == (n, S)
        again = env.replay_sample(n, seed=9, draw=4, reward="colran")
        assert all(torch.equal(again[k], got[k]) for k in got)
        other = {k: t.clone() for k, t in env.replay_sample(n, seed=9, draw=5, reward="colran").items()}
        assert not torch.equal(other["index"], got["index"])
        assert not torch.equal(env.replay_sample(n, seed=10, draw=4, reward="colran")["index"], got["index"])
    env.close()


def test_error_rules():
    need_gpu()
    from intent_radio_sched_multi_slice_amd import _lib
    E_INVALID, E_STATE = -1, -3
    wl, env, (actor, log_std, critic) = hr.make_env("S5U25", "64x64", "gauss_tanh", B, bind=False)
    lib, h, S = env._lib, env._h, env.S
    stream = env._stream()
    keep = []
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    collect = lambda n=T: lib.ranenv_collect_replay(h, n, *env._p_out, stream)  # noqa: E731
    out = {k: torch.zeros(s, dtype=dt, device=env.device) for k, (s, dt) in dict(
        obs=((4, 10 * S), torch.float32), action=((4, S), torch.float32), reward=((4,), torch.float32), next_obs=((4, 10 * S), torch.float32),
        done=((4,), torch.uint8)).items()}
    sample = lambda n=4, col=0: lib.ranenv_replay_sample(h, n, 1, 2, col, *(p(out[k]) for k in ("obs", "action", "reward", "next_obs", "done")),  # noqa: E731
                                                         None, stream)
    torch.cuda.synchronize()
    before = {k: x.clone() for k, x in env.views().items()}

    def ring_struct(tensors, cap=CAP, drop=None):
        st = _lib.Replay()
        st.capacity = cap
        for f, t in tensors.items():
            setattr(st, f, None if f == drop else t.data_ptr())
        return st

    tensors = {f: torch.zeros((CAP,) + shape(B, S), dtype=dt, device=env.device) for f, (dt, shape) in env.REPLAY_SHAPES.items()}
    # no ring: collect and sample refuse
    assert lib.ranenv_set_policy(h, _lib.POLICY_HEAD_NETWORK, _lib.INTRA_RR) == 0
    assert collect() == E_STATE and b"ring" in lib.ranenv_last_error(h)
    assert sample() == E_STATE
    # the ring's own rules
    assert lib.ranenv_bind_replay(h, C.byref(ring_struct(tensors, cap=1))) == E_INVALID
    for f in tensors:
        assert lib.ranenv_bind_replay(h, C.byref(ring_struct(tensors, drop=f))) == E_INVALID, f
    assert collect() == E_STATE                                                                       # (a refused binding binds nothing)
    assert lib.ranenv_bind_replay(h, C.byref(ring_struct(tensors))) == 0
    n = C.c_int64(-1)
    assert lib.ranenv_get_replay_count(h, C.byref(n)) == 0 and n.value == 0
    # bound, but no head net / another policy / no head outputs
    assert collect() == E_STATE and b"head policy network" in lib.ranenv_last_error(h)
    layers, act = hr.layers_of(actor)
    m = env._mlp_struct(layers, act, _lib.NET_IN_OBS, keep)
    assert lib.ranenv_set_head_policy_network(h, C.byref(m), _lib.HEAD_DIST_GAUSS_TANH, None, 1, 7, stream) == 0
    assert lib.ranenv_set_policy(h, _lib.POLICY_MAPF, _lib.INTRA_RR) == 0
    assert collect() == E_STATE and b"HEAD_NETWORK" in lib.ranenv_last_error(h)
    assert lib.ranenv_set_policy(h, _lib.POLICY_HEAD_NETWORK, _lib.INTRA_RR) == 0
    assert lib.ranenv_bind_head_outputs(h, None, None) == 0
    assert collect() == E_STATE and b"dev_obs_head" in lib.ranenv_last_error(h)
    assert lib.ranenv_bind_head_outputs(h, p(env.head_obs), p(env.head_reward)) == 0
    # n_steps
    assert collect(0) == E_INVALID and collect(CAP + 1) == E_INVALID
    # the sampler: nothing recorded yet; then its arguments
    assert sample() == E_STATE
    torch.cuda.synchronize()
    assert all(torch.equal(x, env.views()[k]) for k, x in before.items())                             # no refusal stepped anything
    assert not any(bool(t.any()) for t in tensors.values())
    assert collect(CAP) == 0
    assert lib.ranenv_get_replay_count(h, C.byref(n)) == 0 and n.value == CAP
    assert sample(col=2) == E_INVALID and sample(col=-1) == E_INVALID and sample(n=0) == E_INVALID
    assert sample() == 0
    # SAC policies still do not collect PPO batches
    traj = _lib.HeadTrajectory()
    assert lib.ranenv_collect_head(h, 4, C.byref(traj), 0, 0.99, 0.95, *env._p_out, stream) == E_INVALID
    # NULL unbinds and zeroes the count
    assert lib.ranenv_bind_replay(h, None) == 0
    assert lib.ranenv_get_replay_count(h, C.byref(n)) == 0 and n.value == 0
    assert collect() == E_STATE and sample() == E_STATE
    torch.cuda.synchronize()
    assert int(env.views()["step_number"].min()) == CAP
    env.close()
