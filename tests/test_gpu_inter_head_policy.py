"""The head policy source "inter" on the device (ranenv_set_head_policy_source, include/ranenv.h): the reference's IBSchedSB3
(agents/sb3_sched.py, agents/sb3_pf_sched.py), an SB3 actor on IBSched's own player_0 observation.  Everything through the C ABI via the
Python layer, on SORTED scenario tables: which rows the actor reads, env parity with the CPU oracle under the device's own scores,
rollout against a step loop, acting without head outputs, collect_head and the replay ring against a step loop on a twin, the SAC
targets of a sampled minibatch, evaluate(), the error rules, and the way back to the head source."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import head_policy_ref as hr
from tests import inter_head_ref as ih
from tests import sac_ref as sr
from tests.gpu_common import HEAD_OUTPUTS, LOOSE_WINDOWS_AND_SE, OUTPUTS, assert_matches_oracle, assert_same_state, need_gpu, to_host

pytestmark = pytest.mark.gpu

B = ih.B
T = 24
SEED = 0x1234_5678_9ABC
E_INVALID, E_STATE = -1, -3
EP_SUMS = {"episode_metrics": ("running", "episode_log", "episodes_done")}


def _state_equal(a, b, tables, what, heads=False, metrics=None):
    assert_same_state(a, b, tables, what, loose=LOOSE_WINDOWS_AND_SE, outputs=OUTPUTS + (HEAD_OUTPUTS if heads else ()), actions=("scores",),
                      metrics=metrics)


# ---- 1. the scores read the right rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [False, True])
@pytest.mark.parametrize("stochastic", [False, True])
@pytest.mark.parametrize("net", list(ih.NETS))
@pytest.mark.parametrize("size", list(ih.SIZES))
def test_scores_are_the_actors_on_obs_inter(size, net, stochastic, heads):
    """After the reset and after each of three steps: every (env, position) of the device's scores lies within the float64 twin's bound
    on the obs_inter rows the step found, and within 1e-5 of the float32 restatement.  With head outputs bound as well the two
    observations differ on every env, and the scores are NOT the twin's on the head rows for most envs."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd import adapters
    dist = ih.DIST_OF[net]
    _, env, (actor, log_std, _) = ih.make_env(size, net, dist, stochastic=stochastic, seed=SEED, heads=heads)
    assert env.head_observation == "inter" and (getattr(env, "head_obs", None) is not None) == heads
    worst = 0.0
    for t in range(4):
        torch.cuda.synchronize()
        obs = env.obs_inter.cpu().numpy().copy()
        head = env.head_obs.cpu().numpy().copy() if heads else None
        episode, step = ih.counters(env)
        env.step()
        dev = env.policy_actions()["scores"].cpu().numpy()
        z = hr.noise(np.arange(B), episode, step, env.S, SEED) if stochastic else None
        ref = hr.HeadRef(obs, actor, dist, log_std, z)
        worst = max(worst, hr.check_scores(ref, dev, f"TTI {t}"))
        want, _ = adapters.head_policy_actions(obs, actor, dist, log_std, stochastic, SEED, env_ids=np.arange(B), episode=episode, step=step)
        print(f"TTI {t}: max |device - restatement| = {np.abs(dev - want.numpy()).max():.3g}")
        np.testing.assert_allclose(dev, want.numpy(), rtol=0, atol=1e-5)
        assert np.all(np.abs(dev) <= 1.0)
        if heads:
            assert (obs != head).any(axis=1).all(), f"TTI {t}: obs_inter equals head_obs on some env"
            wrong = ih.outside_bound(hr.HeadRef(head, actor, dist, log_std, z), dev)
            print(f"TTI {t}: {int(wrong.sum())} of {B} envs outside the twin's bound on the head rows")
            assert wrong.mean() > 0.5, f"TTI {t}: the scores fit the head rows on {B - int(wrong.sum())} of {B} envs"
    print(f"worst error / bound: {worst:.3g}")
    env.close()


# ---- 2. the env under its own scores equals the CPU oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("size,net,intra", [("S5U25", "64x64", "rr"), ("S10U100", "256x256", "pf"), ("S10U100", "64x64", "rr"),
                                            ("S5U25", "256x256", "pf")])
def test_env_parity_with_oracle_under_its_own_scores(size, net, intra):
    """The device's scores -- by sorted position, on sorted tables -- fed into the CPU oracle as external scores with the same fixed
    intra scheduler, 20 TTIs: packet counts and buffers exact, observations 1e-5, rewards 1e-9 (tests/gpu_common.py)."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd import _lib
    from oracle import pyoracle
    code = {"rr": _lib.INTRA_RR, "pf": _lib.INTRA_PF}[intra]
    wl, env, _ = ih.make_env(size, net, ih.DIST_OF[net], stochastic=True, seed=3, intra=code)
    assert env.fixed_intra == code
    cfg = pyoracle.make_cfg(env.S, env.U, env.R, env.G, env.Us, max_steps=1000)
    se_host = wl.se_pool.transpose(1, 2).contiguous().cpu().numpy()
    trf_host = wl.traffic_pool.cpu().numpy().astype(np.float64)
    eps = env.episodes
    oenvs = []
    for b in range(B):
        e = pyoracle.OracleEnv(cfg)
        e.set_scenario(wl.tables, int(wl.scenario[b]))
        e.reset(se_host[int(eps["se_base"][b] + eps["se_offset"][b] % wl.trace_len)])
        oenvs.append(e)
    choice = np.full(env.S, code, dtype=np.int32)
    for t in range(20):
        obs, rew, _ = env.step()
        sc = env.policy_actions()["scores"].cpu().numpy()
        for b, e in enumerate(oenvs):
            tile = int(eps["se_base"][b] + (eps["se_offset"][b] + t) % wl.trace_len)
            row = int(eps["trf_base"][b] + (eps["trf_offset"][b] + t) % wl.trace_len)
            e.step(sc[b].copy(), choice, se_host[tile], trf_host[row])
        assert_matches_oracle(env, obs, rew, oenvs, (size, intra, t))
    env.close()


# ---- 3. rollout(n) = n x step() -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [False, True])
@pytest.mark.parametrize("se_mode", ["stream", "gather"])
@pytest.mark.parametrize("size", list(ih.SIZES))
def test_rollout_is_the_step_loop(size, se_mode, heads):
    """rollout(T) with 1 and 3 partitions under auto-reset leaves env state, outputs, scores and the eight episode sums bit for bit as
    T calls of step() do, episodes ending inside the rollout; without head outputs bound and with them."""
    need_gpu()
    kw = dict(stochastic=True, seed=SEED, autoreset=True, se_mode=se_mode, metrics=8, heads=heads)
    wl, ref, _ = ih.make_env(size, "64x64", "gauss_clip", **kw)
    ends = 0
    for _ in range(T):
        ref.step()
        ends += int(ref.done.sum())
    assert ends > B
    for parts in (1, 3):
        _, env, _ = ih.make_env(size, "64x64", "gauss_clip", parts=parts, **kw)
        env.rollout(T)
        _state_equal(env, ref, wl.tables, (parts,), heads, EP_SUMS)
        assert bool(env.episode_metrics()["episode_log"][:, :, 1].any())
        env.close()
    ref.close()


# ---- 4. acting without enable_heads() -------------------------------------------------------------------------------------------------
def test_acting_needs_no_head_outputs_but_the_head_source_still_does():
    need_gpu()
    from intent_radio_sched_multi_slice_amd import _lib
    _, env, _ = ih.make_env("S5U25", "64x64", "gauss_clip", stochastic=True, seed=SEED)
    assert getattr(env, "head_obs", None) is None
    lib, h, stream = env._lib, env._h, env._stream()
    step = lambda: lib.ranenv_step(h, None, None, None, None, *env._p_out, stream)  # noqa: E731
    assert step() == 0 and lib.ranenv_rollout(h, 3, *env._p_out, stream) == 0
    torch.cuda.synchronize()
    assert int(env.views()["step_number"].min()) == 4 and bool(env.policy_actions()["scores"].any())
    # the head source on the same handle: no dev_obs_head, so the refusal of today, word for word
    assert lib.ranenv_set_head_policy_source(h, _lib.HEAD_SRC_HEAD) == 0
    assert step() == E_STATE
    assert lib.ranenv_last_error(h) == b"the head policy network reads dev_obs_head: none is bound (ranenv_bind_head_outputs)"
    assert lib.ranenv_rollout(h, 3, *env._p_out, stream) == E_STATE
    assert lib.ranenv_set_head_policy_source(h, _lib.HEAD_SRC_INTER) == 0
    assert step() == 0
    torch.cuda.synchronize()
    assert int(env.views()["step_number"].min()) == 5
    env.close()


# ---- 5. collect_head against the step loop's record on a twin -------------------------------------------------------------------------
@pytest.mark.parametrize("heads", [False, True])
@pytest.mark.parametrize("size", list(ih.SIZES))
def test_record_is_the_step_loop_and_state_is_the_rollouts(size, heads):
    """collect_head(T) records, TTI by TTI, what a step() loop on a twin sees: the obs_inter rows in front of each step, the unclamped
    action, the step's [B, S + 1] reward rows and done bit for bit; logp and vf (slot T on the observation left behind the last
    auto-reset) within the float64 bounds; adv / vtarg equal adapters.gae on column 0 bit for bit; the state is rollout(T)'s; the
    critic fused behind the actor and in a launch of its own give one record."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd import adapters
    kw = dict(stochastic=True, seed=SEED, autoreset=True, metrics=8, heads=heads)
    wl, ref, (actor, log_std, critic) = ih.make_env(size, "64x64", "gauss_clip", **kw)
    S = ref.S
    want = {k: [] for k in ("obs_head", "scores", "reward_head", "done")}
    counters = []
    for _ in range(T):
        counters.append(ih.counters(ref))
        want["obs_head"].append(ref.obs_inter.clone())
        ref.step()
        for k, x in (("scores", ref.policy_actions()["scores"]), ("reward_head", ref.reward), ("done", ref.done)):
            want[k].append(x.clone())
    want = {k: torch.stack(x) for k, x in want.items()}
    d = want["done"].cpu().numpy()
    assert d[-1].any() and not d.all(axis=1).any() and len({int(np.argmax(d[:, b])) for b in range(B) if d[:, b].any()}) >= 4
    assert want["reward_head"].shape == (T, B, S + 1)
    records = {}
    for parts, split in ((1, 0), (3, -1), (1, 1)):
        _, env, _ = ih.make_env(size, "64x64", "gauss_clip", parts=parts, **kw)
        _, roll, _ = ih.make_env(size, "64x64", "gauss_clip", parts=parts, **kw)
        if split >= 0:
            env.set_option("collect_split", split)
        rec = env.collect_head(T, reward="ibsched", gamma=0.97, lam=0.9)
        roll.rollout(T)
        torch.cuda.synchronize()
        for k in ("obs_head", "reward_head", "done"):
            assert rec[k].shape == want[k].shape and torch.equal(rec[k], want[k]), (k, parts, split)
        assert torch.equal(rec["action"].clamp(-1.0, 1.0), want["scores"]) and bool((rec["action"].abs() > 1.0).any()), (parts, split)
        r = to_host(rec)
        worst = {"logp": 0.0, "vf": 0.0, "action": 0.0}
        for t in range(T + 1):
            obs = r["obs_head"][t] if t < T else env.obs_inter.cpu().numpy()
            y, bound = hr.value_ref(obs, critic)
            err = np.abs(r["vf"][t] - y)
            assert np.all(err <= bound), f"vf[{t}]: worst {np.max(err / bound):.3g} of the bound"
            worst["vf"] = max(worst["vf"], float(np.max(err / bound)))
            if t == T:
                break
            z = hr.noise(np.arange(B), counters[t][0], counters[t][1], S, SEED)
            a = hr.HeadRef(obs, actor, "gauss_clip", log_std, z)
            err = np.abs(r["action"][t] - a.action)
            assert np.all(err <= a.action_bound), f"action[{t}]"
            worst["action"] = max(worst["action"], float(np.max(err / a.action_bound)))
            lp, lb = hr.logp_ref(log_std, z, B)
            err = np.abs(r["logp"][t].astype(np.float64) - lp)
            assert np.all(err <= lb), f"logp[{t}]: worst {np.max(err / lb):.3g} of the bound"
            worst["logp"] = max(worst["logp"], float(np.max(err / lb)))
        print(f"parts {parts} split {split}: worst error / bound {worst}")
        adv, vtarg = adapters.gae(r["reward_head"][:, :, 0:1], r["vf"][:, :, None], r["done"], 0.97, 0.9)
        assert np.array_equal(r["adv"], adv[:, :, 0]) and np.array_equal(r["vtarg"], vtarg[:, :, 0]), (parts, split)
        _state_equal(env, roll, wl.tables, (parts, split), heads, EP_SUMS)
        records[(parts, split)] = r
        env.close()
        roll.close()
    for k in records[(1, 0)]:
        assert np.array_equal(records[(1, 0)][k], records[(1, 1)][k]), ("fused against split", k)
    ref.close()


# ---- 6. the ring against the step loop on a twin --------------------------------------------------------------------------------------
CAP, TR = 7, 5                # two calls of 5 TTIs into 7 slots: the second wraps
SENTINEL = {"obs": -7.0, "next_obs": -7.0, "action": -7.0, "reward_head": -7.0, "done": 255}


def _bound_ring(env, cap=CAP):
    ring = env.bind_replay(cap)
    for k, t in ring.items():
        t.fill_(SENTINEL[k])
    return ring


def _step_loop(ref, n):
    """The transitions of ``n`` step() calls on ``ref``: what the ring must hold, TTI by TTI."""
    want = {k: [] for k in SENTINEL}
    for _ in range(n):
        want["obs"].append(ref.obs_inter.clone())
        ref.step()
        done = ref.done.clone()
        want["action"].append(ref.policy_actions()["scores"].clone())
        want["reward_head"].append(ref.reward.clone())
        want["done"].append(done)
        # behind the step: the terminal row ranenv_autoreset handed out where the episode ended, else the row as it stands
        want["next_obs"].append(torch.where(done[:, None] != 0, ref.term_obs_inter, ref.obs_inter).clone())
    return {k: torch.stack(x) for k, x in want.items()}


@pytest.mark.parametrize("heads", [False, True])
@pytest.mark.parametrize("net", list(ih.NETS))
@pytest.mark.parametrize("size", list(ih.SIZES))
def test_ring_is_the_step_loop(size, net, heads):
    need_gpu()
    kw = dict(stochastic=True, seed=SEED, autoreset=True, metrics=8, critic=False, heads=heads)
    wl, ref, _ = ih.make_env(size, net, ih.DIST_OF[net], **kw)
    want = _step_loop(ref, 2 * TR)
    d = want["done"].cpu().numpy()
    assert d[:TR].any() and d[TR:].any() and not d.all(axis=1).any() and len(set(np.nonzero(d)[0])) >= 4
    ended, live = want["done"][:-1] != 0, want["done"][:-1] == 0
    assert (want["next_obs"][:-1][ended] != want["obs"][1:][ended]).any(dim=1).all()      # the terminal rows are not the next episode's first
    assert torch.equal(want["next_obs"][:-1][live], want["obs"][1:][live])
    assert want["reward_head"].shape == (2 * TR, B, ref.S + 1)
    for parts in (1, 3):
        _, env, _ = ih.make_env(size, net, ih.DIST_OF[net], parts=parts, **kw)
        _, roll, _ = ih.make_env(size, net, ih.DIST_OF[net], parts=parts, **kw)
        ring = _bound_ring(env)
        assert ring["reward_head"].shape == (CAP, B, env.S + 1) and env.replay_count() == 0
        for call in (1, 2):
            env.collect_replay(TR)
            roll.rollout(TR)
            torch.cuda.synchronize()
            n = call * TR
            assert env.replay_count() == n
            for slot in range(CAP):
                ks = [k for k in range(n) if k % CAP == slot]
                for f, t in ring.items():
                    if ks:      # the latest TTI that went to the slot (the second call's, where it wrapped)
                        assert torch.equal(t[slot], want[f][ks[-1]]), (f, slot, parts, call)
                    else:       # not yet written
                        assert bool((t[slot] == SENTINEL[f]).all()), (f, slot, parts, call)
            _state_equal(env, roll, wl.tables, (parts, call), heads, EP_SUMS)
        env.close()
        roll.close()
    ref.close()


def test_sampler_gathers_the_rows_and_column_0():
    need_gpu()
    from intent_radio_sched_multi_slice_amd import adapters
    _, env, _ = ih.make_env("S5U25", "256x256", "gauss_tanh", stochastic=True, seed=SEED, autoreset=True, critic=False)
    ring = _bound_ring(env)
    n, S = 100, env.S
    for steps, written in ((3, 3), (5, 8)):                     # part-filled, then full (and wrapped)
        env.collect_replay(steps)
        torch.cuda.synchronize()
        assert env.replay_count() == written
        flat = {k: t.reshape((CAP * B,) + t.shape[2:]) for k, t in ring.items()}
        got = {k: t.clone() for k, t in env.replay_sample(n, seed=9, draw=4, reward="ibsched").items()}
        idx = adapters.replay_sample_index(n, 9, 4, written, CAP, B)
        assert np.array_equal(got["index"].cpu().numpy(), idx) and idx.max() < min(written, CAP) * B
        ix = torch.as_tensor(idx, device=env.device)
        assert torch.equal(got["obs"], flat["obs"][ix]) and torch.equal(got["next_obs"], flat["next_obs"][ix])
        assert torch.equal(got["done"], flat["done"][ix])
        assert torch.equal(got["action"], flat["action"][ix].to(torch.float32))
        assert torch.equal(got["reward"], flat["reward_head"][ix, 0].to(torch.float32))
        assert not torch.equal(got["reward"], flat["reward_head"][ix, 1].to(torch.float32))
        assert not bool((got["obs"] == SENTINEL["obs"]).any()) and got["action"].shape == (n, S)
        assert all(torch.equal(t, got[k]) for k, t in env.replay_sample(n, seed=9, draw=4).items())      # (None = "ibsched")
    env.close()


# ---- 7. the SAC targets of a sampled minibatch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,size", [("64x64", "S5U25"), ("256x256", "S10U100")])
def test_sac_targets_of_a_sampled_minibatch(case, size):
    need_gpu()
    _, env, _ = ih.make_env(size, "256x256", "gauss_tanh", autoreset=True, bind=False)
    actor, q1, q2 = sr.sac_nets(case)
    env.set_head_policy_network(actor, "gauss_tanh", stochastic=True, seed=SEED, observation="inter")
    env.set_sac_critics(q1, q2)
    env.bind_replay(CAP)
    env.collect_replay(TR)
    n, seed, draw = 400, 77, 3
    mb = env.replay_sample(n, seed=9, draw=4, reward="ibsched")
    got = to_host(env.sac_targets(mb["next_obs"], mb["reward"], mb["done"], gamma=sr.GAMMA, ent_coef=sr.ENT_COEF, stochastic=True, seed=seed,
                                  draw=draw))
    rows = to_host(mb)
    ref = sr.SacRef(rows["next_obs"], rows["reward"], rows["done"], actor, q1, q2, sr.GAMMA, sr.ENT_COEF, sr.noise(n, env.S, seed, draw))
    for k in ("next_action", "next_logp", "q", "target"):
        bound = getattr(ref, k + "_bound")
        print(f"{case} {k}: worst error / bound {np.max(np.abs(got[k].astype(np.float64) - getattr(ref, k)) / bound):.3g}, largest bound {bound.max():.3g}")
    sr.check_outputs(ref, got, case)
    done = rows["done"] != 0
    assert done.any() and not done.all()
    assert np.array_equal(got["target"][done], rows["reward"][done])           # terminal rows: exactly the reward
    env.close()


# ---- 8. evaluate() --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,net", [("S5U25", "64x64"), ("S10U100", "256x256")])
def test_evaluate_sums_reward_column_0(size, net):
    """evaluate(n): metric column [1] of every episode is the sum, in TTI order in float64, of reward[:, 0] from a step loop on a twin."""
    need_gpu()
    n_ep, slots = 2, 12
    kw = dict(stochastic=True, seed=SEED, autoreset=True, metrics=slots)
    _, env, _ = ih.make_env(size, net, ih.DIST_OF[net], **kw)
    _, twin, _ = ih.make_env(size, net, ih.DIST_OF[net], **kw)
    out = env.evaluate(n_ep)
    run, log, n_done = np.zeros(B), np.zeros((B, slots)), np.zeros(B, dtype=np.int64)
    for _ in range(n_ep * max(ih.EPISODE_LENGTHS)):
        twin.step()
        r, d = twin.reward[:, 0].cpu().numpy(), twin.done.cpu().numpy()
        run = run + r
        for b in np.nonzero(d)[0]:
            if n_done[b] < slots:
                log[b, n_done[b]] = run[b]
            n_done[b] += 1
            run[b] = 0.0
    assert n_done.min() >= n_ep and np.any(log[:, :n_ep] != 0)
    assert env.METRIC_NAMES[1] == "reward" and out["reward"].shape == (B, n_ep)
    assert np.array_equal(out["reward"], log[:, :n_ep])
    assert np.array_equal(out["ttis"], np.asarray(ih.EPISODE_LENGTHS, dtype=np.float64)[np.arange(B) % 6][:, None].repeat(n_ep, 1))
    env.close()
    twin.close()


# ---- 9. the error rules, through the C ABI --------------------------------------------------------------------------------------------
def test_error_rules():
    need_gpu()
    from intent_radio_sched_multi_slice_amd import _lib
    wl, env, _ = ih.make_env("S5U25", "64x64", "gauss_clip", stochastic=True, seed=SEED, heads=True)
    lib, h, S, stream = env._lib, env._h, env.S, env._stream()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    INTER, HEAD = _lib.HEAD_SRC_INTER, _lib.HEAD_SRC_HEAD
    torch.cuda.synchronize()
    before = {k: x.clone() for k, x in env.views().items()}
    traj = _lib.HeadTrajectory()
    collect_head = lambda col: lib.ranenv_collect_head(h, 4, C.byref(traj), col, 0.99, 0.95, *env._p_out, stream)  # noqa: E731
    collect_replay = lambda: lib.ranenv_collect_replay(h, TR, *env._p_out, stream)  # noqa: E731
    out = {k: torch.zeros(s, dtype=dt, device=env.device) for k, (s, dt) in dict(
        obs=((4, 10 * S), torch.float32), action=((4, S), torch.float32), reward=((4,), torch.float32), next_obs=((4, 10 * S), torch.float32),
        done=((4,), torch.uint8)).items()}
    sample = lambda col: lib.ranenv_replay_sample(h, 4, 1, 2, col, *(p(out[k]) for k in ("obs", "action", "reward", "next_obs", "done")),  # noqa: E731
                                                  None, stream)
    # a bad source value changes nothing
    for bad in (2, -1, 255):
        assert lib.ranenv_set_head_policy_source(h, bad) == E_INVALID and b"source" in lib.ranenv_last_error(h)
    assert lib.ranenv_set_head_policy_source(None, INTER) == E_INVALID
    # the inter source without dev_obs_inter: the NETWORK path's refusal
    no_obs = (None,) + env._p_out[1:]
    msg = b"the policy network reads obs_inter: the step needs that buffer"
    assert lib.ranenv_step(h, None, None, None, None, *no_obs, stream) == E_INVALID and lib.ranenv_last_error(h) == msg
    assert lib.ranenv_step_range(h, 0, 16, None, None, None, None, *no_obs, stream) == E_INVALID and lib.ranenv_last_error(h) == msg
    assert lib.ranenv_rollout(h, 3, *no_obs, stream) == E_INVALID and lib.ranenv_last_error(h) == msg
    # reward_col: 0..S under the inter source, 0 / 1 under the head source
    assert collect_head(S + 1) == E_INVALID and collect_head(-1) == E_INVALID
    env.bind_replay(CAP)
    torch.cuda.synchronize()
    assert all(torch.equal(x, env.views()[k]) for k, x in before.items())                # no refusal stepped anything
    assert collect_replay() == 0 and env.replay_count() == TR
    assert sample(S + 1) == E_INVALID and sample(-1) == E_INVALID and sample(S) == 0 and sample(0) == 0
    # setting the source it has keeps the ring; changing it unbinds the ring
    assert lib.ranenv_set_head_policy_source(h, INTER) == 0 and env.replay_count() == TR
    assert lib.ranenv_set_head_policy_source(h, HEAD) == 0
    assert env.replay_count() == 0
    assert collect_replay() == E_STATE and b"ring" in lib.ranenv_last_error(h)
    assert sample(0) == E_STATE
    assert collect_head(2) == E_INVALID and lib.ranenv_last_error(h) == b"reward_col 2 (0 = SchedTWC, 1 = SchedColORAN)"
    assert collect_head(1) == 0                                  # (an empty record under the head source: the envs step)
    torch.cuda.synchronize()
    assert int(env.views()["step_number"].min()) == TR + 4
    env.close()


# ---- 10. switching back ---------------------------------------------------------------------------------------------------------------
def test_back_to_the_head_source_is_a_fresh_head_envs_run():
    """One handle: inter source, a rollout, back to the head source, a rollout.  A fresh head-source env that was stepped through the
    first TTIs with the same scores (a third env's, from a step loop under the inter source) then runs the same second rollout: state,
    outputs, head buffers and scores bit for bit."""
    need_gpu()
    n = 6
    kw = dict(stochastic=True, seed=SEED, heads=True)
    wl, env, (actor, log_std, _) = ih.make_env("S5U25", "64x64", "gauss_clip", **kw)
    _, loop, _ = ih.make_env("S5U25", "64x64", "gauss_clip", **kw)
    _, fresh, _ = ih.make_env("S5U25", "64x64", "gauss_clip", observation="head", **kw)
    assert (env.head_observation, fresh.head_observation) == ("inter", "head")
    env.rollout(n)
    for _ in range(n):
        loop.step()
        fresh.step(loop.policy_actions()["scores"].clone())
    _state_equal(env, loop, wl.tables, "inter rollout", True)
    env.set_head_policy_network(actor, "gauss_clip", log_std, stochastic=True, seed=SEED, allow_sorted=True)
    assert env.head_observation == "head"
    env.rollout(T)
    fresh.rollout(T)
    _state_equal(env, fresh, wl.tables, "head rollout", True)
    assert not torch.equal(env.policy_actions()["scores"], loop.policy_actions()["scores"])
    for e in (env, loop, fresh):
        e.close()
