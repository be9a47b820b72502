"""Head policies on the device (RANENV_POLICY_HEAD_NETWORK, include/ranenv.h): the actor's forward against the float64 twin of
tests/head_policy_ref.py and the float32 restatement, env parity with the CPU oracle under the device's own scores, rollout against
a step loop, noise, the episode sums of the head rewards, collect_head, and the error paths straight through the C ABI."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import head_policy_ref as hr
from tests.common import OBS_TOL, REW_TOL
from tests.gpu_common import HEAD_OUTPUTS, LOOSE_WINDOWS_AND_SE, OUTPUTS, assert_same_state, need_gpu

pytestmark = pytest.mark.gpu

T = 24
SEED = 0x1234_5678_9ABC
_state_equal = functools.partial(assert_same_state, loose=LOOSE_WINDOWS_AND_SE, outputs=OUTPUTS + HEAD_OUTPUTS, actions=("scores",))


# ---- 1. forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stochastic", [False, True])
@pytest.mark.parametrize("dist", ["gauss_clip", "gauss_tanh"])
@pytest.mark.parametrize("size", list(hr.SIZES))
@pytest.mark.parametrize("net", list(hr.NETS))
def test_forward_within_the_float64_bound(net, size, dist, stochastic):
    """Injected head observations written into the bound buffer before a step: every (env, position) of the device's scores lies
    within the twin's bound, and within 1e-5 of the float32 restatement."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd import adapters
    B = 70                                                   # (not a multiple of the 32 rows of a workgroup)
    _, env, (actor, log_std, _) = hr.make_env(size, net, dist, B, stochastic=stochastic, seed=SEED)
    rng = np.random.default_rng(17)
    worst = 0.0
    for t in range(3):
        obs = hr.injected_head_obs(rng, B, env.S)
        env.head_obs.copy_(torch.from_numpy(obs))
        v = env.views()
        episode, step = v["episode_number"].cpu().numpy().copy(), v["step_number"].cpu().numpy().copy()
        env.step()
        dev = env.policy_actions()["scores"].cpu().numpy()
        z = hr.noise(np.arange(B), episode, step, env.S, SEED) if stochastic else None
        ref = hr.HeadRef(obs, actor, dist, log_std, z)
        worst = max(worst, hr.check_scores(ref, dev, f"TTI {t}"))
        want, _ = adapters.head_policy_actions(obs, actor, dist, log_std, stochastic, SEED, env_ids=np.arange(B), episode=episode, step=step)
        print(f"TTI {t}: max |device - restatement| = {np.abs(dev - want.numpy()).max():.3g}")
        np.testing.assert_allclose(dev, want.numpy(), rtol=0, atol=1e-5)
        assert np.all(np.abs(dev) <= 1.0)
        assert (np.abs(ref.action) > 1.0).any() and (np.abs(ref.action) < 1.0).any()
    print(f"worst error / bound: {worst:.3g}")
    env.close()


# ---- 2. env parity with the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,net,dist,unsorted", [("S5U25", "64x64", "gauss_clip", True), ("S10U100", "256x256", "gauss_tanh", True),
                                                    ("S10U100", "64x64", "gauss_clip", False), ("S5U25", "256x256", "gauss_tanh", False)])
def test_env_parity_with_oracle(size, net, dist, unsorted):
    """The device's own scores (round-robin inside the slices) fed into the CPU oracle along 50 TTIs: integers exact, obs_inter
    1e-5, rewards 1e-9, head observation and head rewards at the tolerances of the reference-agent tests."""
    need_gpu()
    from oracle import pyoracle
    B, steps = 9, 50
    wl, env, _ = hr.make_env(size, net, dist, B, stochastic=True, seed=3, unsorted=unsorted)
    uc = hr.usecase_of(wl.tables)
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
    rr = np.zeros(env.S, dtype=np.int32)
    saw_neg = saw_col = False
    for t in range(steps):
        obs, rew, done = env.step()
        sc = env.policy_actions()["scores"].cpu().numpy()
        v = {k: x.cpu().numpy() for k, x in env.views().items()}
        oi, rw = obs["obs_inter"].cpu().numpy(), rew.cpu().numpy()
        ho, hrw = env.head_obs.cpu().numpy(), env.head_reward.cpu().numpy()
        for b, e in enumerate(oenvs):
            tile = int(eps["se_base"][b] + (eps["se_offset"][b] + t) % wl.trace_len)
            row = int(eps["trf_base"][b] + (eps["trf_offset"][b] + t) % wl.trace_len)
            e.step(sc[b].copy(), rr, se_host[tile], trf_host[row])
            raw, o = e.raw(), e.obs()
            for k in ("pkt_effective_thr", "dropped_pkts", "pkt_throughputs"):
                assert np.array_equal(v[k][b], raw[k]), (k, t, b)
            np.testing.assert_allclose(oi[b], o["obs_inter"], rtol=0, atol=OBS_TOL)
            np.testing.assert_allclose(rw[b], o["reward"], rtol=0, atol=REW_TOL)
            h_obs, r_twc, r_col = e.heads(uc[int(wl.scenario[b])])
            np.testing.assert_allclose(ho[b], h_obs, rtol=2e-6, atol=OBS_TOL, err_msg=str((t, b)))
            np.testing.assert_allclose(hrw[b], [r_twc, r_col], rtol=0, atol=REW_TOL, err_msg=str((t, b)))
            saw_neg |= r_twc < 0
            saw_col |= r_col != 0
    assert saw_neg and saw_col
    env.close()


# ---- 3. rollout(n) = n x step() ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("se_mode", ["stream", "gather"])
@pytest.mark.parametrize("autoreset", [False, True])
@pytest.mark.parametrize("size", list(hr.SIZES))
def test_rollout_is_the_step_loop(size, autoreset, se_mode):
    """rollout(T) with 1, 2 and 3 partitions leaves env state, outputs, head buffers, scores and the head rewards' episode sums bit
    for bit as T calls of step() do, with episode ends inside the rollout."""
    need_gpu()
    B = 50
    kw = dict(stochastic=True, seed=SEED, autoreset=autoreset, se_mode=se_mode, metrics=8)
    wl, ref, _ = hr.make_env(size, "64x64", "gauss_clip", B, **kw)
    ends = 0
    for _ in range(T):
        ref.step()
        ends += int(ref.done.sum())
    assert (ends > B) if autoreset else ends == 0
    for parts in (1, 2, 3):
        _, env, _ = hr.make_env(size, "64x64", "gauss_clip", B, parts=parts, **kw)
        env.rollout(T)
        _state_equal(env, ref, wl.tables, (parts,))
        ma, mb = env.head_episode_metrics(), ref.head_episode_metrics()
        assert torch.equal(ma["running"], mb["running"]) and torch.equal(ma["episode_log"], mb["episode_log"]), parts
        assert torch.equal(env.episode_metrics()["episode_log"], ref.episode_metrics()["episode_log"])
        env.close()
    ref.close()


# ---- 4. noise -----------------------------------------------------------------------------------------------------------------------
def test_noise_depends_on_the_counters_alone():
    """Stochastic runs with one seed are identical across partition counts and step_range splits; another seed differs."""
    need_gpu()
    B, n = 70, 6
    runs = {}
    for name, parts, seed in (("whole", 1, 5), ("parts3", 3, 5), ("ranges", 1, 5), ("other", 1, 6)):
        wl, env, _ = hr.make_env("S5U25", "64x64", "gauss_tanh", B, stochastic=True, seed=seed, parts=parts)
        hist = []
        for _ in range(n):
            if name == "ranges":
                for lo, cnt in ((0, 17), (17, 32), (49, 21)):
                    env._check(env._lib.ranenv_step_range(env._h, lo, cnt, None, None, None, None, *env._p_out, env._stream()), "ranenv_step_range")
            else:
                env.step()
            hist.append(env.policy_actions()["scores"].clone())
        torch.cuda.synchronize()
        runs[name] = (wl, env, torch.stack(hist))
    wl, whole, sc = runs["whole"]
    for name in ("parts3", "ranges"):
        assert torch.equal(runs[name][2], sc), name
        _state_equal(runs[name][1], whole, wl.tables, name)
    assert not torch.equal(runs["other"][2], sc)
    assert float((runs["other"][2] - sc).abs().max()) > 1e-3
    for _, env, _ in runs.values():
        env.close()


# ---- 5. episode sums of the head rewards ----------------------------------------------------------------------------------------------
def _episode_sums(env, n_ttis, slots):
    """A step loop that adds the head reward rows read back every TTI, sequentially in float64: (running [B, 2], log [B, slots, 2])."""
    B = env.B
    run, log, n_done = np.zeros((B, 2)), np.zeros((B, slots, 2)), np.zeros(B, dtype=np.int64)
    for _ in range(n_ttis):
        env.step()
        r, d = env.head_reward.cpu().numpy(), env.done.cpu().numpy()
        run = run + r
        for b in np.nonzero(d)[0]:
            if n_done[b] < slots:
                log[b, n_done[b]] = run[b]
            n_done[b] += 1
            run[b] = 0.0
    return run, log, n_done


@pytest.mark.parametrize("size", list(hr.SIZES))
def test_head_reward_sums_equal_a_sequential_sum(size):
    need_gpu()
    B, slots, n = 50, 12, 52                                 # the longest episodes (24 TTIs) end twice
    _, env, _ = hr.make_env(size, "64x64", "gauss_clip", B, stochastic=True, seed=SEED, autoreset=True, metrics=slots)
    run, log, n_done = _episode_sums(env, n, slots)
    assert n_done.min() >= 2 and np.abs(log).max() > 0 and np.any(log[:, :, 0] != 0) and np.any(log[:, :, 1] != 0)
    m = env.head_episode_metrics()
    torch.cuda.synchronize()
    assert np.array_equal(m["running"].cpu().numpy(), run)
    assert np.array_equal(m["episode_log"].cpu().numpy(), log)
    assert np.array_equal(env.episode_metrics()["episodes_done"].cpu().numpy(), n_done)
    # a reset zeroes the running pair; enable_metrics zeroes the log
    env.reset()
    torch.cuda.synchronize()
    assert not m["running"].any()
    env.enable_metrics(slots)
    torch.cuda.synchronize()
    assert not m["episode_log"].any()
    env.close()


def test_evaluate_fills_the_head_log_with_the_same_episodes():
    need_gpu()
    B, n_ep, slots = 48, 2, 12
    kw = dict(stochastic=True, seed=SEED, autoreset=True, metrics=slots)
    _, env, _ = hr.make_env("S5U25", "64x64", "gauss_clip", B, **kw)
    _, twin, _ = hr.make_env("S5U25", "64x64", "gauss_clip", B, **kw)
    out = env.evaluate(n_ep)
    _, log, n_done = _episode_sums(twin, n_ep * max(hr.EPISODE_LENGTHS), slots)
    assert n_done.min() >= n_ep
    got = env.head_episode_metrics()["episode_log"].cpu().numpy()
    assert np.array_equal(got[:, :n_ep], log[:, :n_ep])
    assert out["ttis"].shape == (B, n_ep)
    assert np.array_equal(out["ttis"], np.asarray(hr.EPISODE_LENGTHS, dtype=np.float64)[np.arange(B) % 6][:, None].repeat(n_ep, 1))
    env.close()
    twin.close()


def test_head_sums_exist_only_with_metrics_and_heads():
    need_gpu()
    from intent_radio_sched_multi_slice_amd._lib import RanEnvError
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload

    def pointers(env):
        run, log, slots = C.c_void_p(), C.c_void_p(), C.c_int32(-1)
        assert env._lib.ranenv_get_head_metrics(env._h, C.byref(run), C.byref(log), C.byref(slots)) == 0
        return run.value, log.value, slots.value

    for first in ("metrics", "heads"):
        env = make_mult_slice_workload(16, torch.device("cuda", 0), n_scenarios=4, n_traces=4, trace_len=16, **hr.SIZES["S5U25"]).env
        assert pointers(env) == (None, None, 0)
        env.enable_metrics(3) if first == "metrics" else env.enable_heads()
        assert pointers(env) == (None, None, 0)                 # one half of the pair: nothing is allocated
        with pytest.raises(RanEnvError):
            env.head_episode_metrics()
        env.enable_heads() if first == "metrics" else env.enable_metrics(3)
        run, log, slots = pointers(env)
        assert run and log and slots == 3
        assert tuple(env.head_episode_metrics()["episode_log"].shape) == (16, 3, 2)
        env.close()
    env = make_mult_slice_workload(16, torch.device("cuda", 0), n_scenarios=4, n_traces=4, trace_len=16, **hr.SIZES["S5U25"]).env
    env.enable_heads()
    env.enable_metrics(0)
    run, log, slots = pointers(env)
    assert run and log is None and slots == 0 and "episode_log" not in env.head_episode_metrics()
    env.close()


# ---- 6. collect_head --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("autoreset", [False, True])
@pytest.mark.parametrize("stochastic", [False, True])
@pytest.mark.parametrize("size", list(hr.SIZES))
def test_record_is_the_step_loop_and_state_is_the_rollouts(size, stochastic, autoreset):
    """collect_head(T) over 1 and 3 partitions records, TTI by TTI, what a step() loop on a twin sees; logp and vf lie within the
    float64 bounds; adv / vtarg equal adapters.gae on the recorded column bit for bit for both columns; everything else is as after
    rollout(T), and one more step() keeps it so."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd import adapters
    B = 50
    kw = dict(stochastic=stochastic, seed=SEED, autoreset=autoreset, metrics=8)
    wl, ref, (actor, log_std, critic) = hr.make_env(size, "64x64", "gauss_clip", B, **kw)
    want = {k: [] for k in ("obs_head", "scores", "reward_head", "done")}
    counters = []
    for _ in range(T):
        v = ref.views()
        counters.append((v["episode_number"].cpu().numpy().copy(), v["step_number"].cpu().numpy().copy()))
        want["obs_head"].append(ref.head_obs.clone())
        ref.step()
        for k, x in (("scores", ref.policy_actions()["scores"]), ("reward_head", ref.head_reward), ("done", ref.done)):
            want[k].append(x.clone())
    want = {k: torch.stack(x) for k, x in want.items()}
    if autoreset:
        d = want["done"].cpu().numpy()
        assert d[-1].any() and not d[-1].all() and len({int(np.argmax(d[:, b])) for b in range(B) if d[:, b].any()}) >= 4
    for parts in (1, 3):
        _, env, _ = hr.make_env(size, "64x64", "gauss_clip", B, parts=parts, **kw)
        _, roll, _ = hr.make_env(size, "64x64", "gauss_clip", B, parts=parts, **kw)
        rec = env.collect_head(T, reward="twc", gamma=0.97, lam=0.9)
        roll.rollout(T)
        torch.cuda.synchronize()
        for k in ("obs_head", "reward_head", "done"):
            assert rec[k].shape == want[k].shape and torch.equal(rec[k], want[k]), (k, parts)
        assert torch.equal(rec["action"].clamp(-1.0, 1.0), want["scores"]), parts
        r = {k: x.cpu().numpy().copy() for k, x in rec.items()}
        worst = {"logp": 0.0, "vf": 0.0, "action": 0.0}
        for t in range(T + 1):
            obs = r["obs_head"][t] if t < T else env.head_obs.cpu().numpy()
            y, bound = hr.value_ref(obs, critic)
            err = np.abs(r["vf"][t] - y)
            assert np.all(err <= bound), f"vf[{t}]"
            worst["vf"] = max(worst["vf"], float(np.max(err / bound)))
            if t == T:
                break
            z = hr.noise(np.arange(B), counters[t][0], counters[t][1], env.S, SEED) if stochastic else None
            a = hr.HeadRef(obs, actor, "gauss_clip", log_std, z)
            err = np.abs(r["action"][t] - a.action)
            assert np.all(err <= a.action_bound), f"action[{t}]"
            worst["action"] = max(worst["action"], float(np.max(err / a.action_bound)))
            lp, lb = hr.logp_ref(log_std, z, B)
            err = np.abs(r["logp"][t].astype(np.float64) - lp)
            assert np.all(err <= lb), f"logp[{t}]: worst {np.max(err / lb):.3g} of the bound"
            worst["logp"] = max(worst["logp"], float(np.max(err / lb)))
        print(f"parts {parts}: worst error / bound {worst}")
        adv, vtarg = adapters.gae(r["reward_head"][:, :, 0:1], r["vf"][:, :, None], r["done"], 0.97, 0.9)
        assert np.array_equal(r["adv"], adv[:, :, 0]) and np.array_equal(r["vtarg"], vtarg[:, :, 0]), parts
        for extra in (0, 1):
            if extra:
                env.step()
                roll.step()
            _state_equal(env, roll, wl.tables, (parts, extra))
            ma, mb = env.head_episode_metrics(), roll.head_episode_metrics()
            assert torch.equal(ma["running"], mb["running"]) and torch.equal(ma["episode_log"], mb["episode_log"]), (parts, extra)
            assert torch.equal(env.episode_metrics()["running"], roll.episode_metrics()["running"])
        env.close()
        roll.close()
    ref.close()


@pytest.mark.parametrize("autoreset", [False, True])
def test_gae_on_the_other_column_null_fields_and_split_launches(autoreset):
    """reward="colran" runs GAE on column 1; fields left out of the record are not written and change nothing else; the critic fused
    behind the actor and in a launch of its own (option collect_split) give the same record bit for bit."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd import adapters
    B = 50
    kw = dict(stochastic=True, seed=SEED, autoreset=autoreset)
    recs = {}
    for split in (0, 1):
        _, env, _ = hr.make_env("S10U100", "256x256", "gauss_clip", B, **kw)
        env.set_option("collect_split", split)
        recs[split] = {k: x.cpu().numpy().copy() for k, x in env.collect_head(T, reward="colran").items()}
        env.close()
    for k in recs[0]:
        assert np.array_equal(recs[0][k], recs[1][k]), k
    r = recs[0]
    assert np.any(r["reward_head"][:, :, 1] != 0)
    adv, vtarg = adapters.gae(r["reward_head"][:, :, 1:2], r["vf"][:, :, None], r["done"])
    assert np.array_equal(r["adv"], adv[:, :, 0]) and np.array_equal(r["vtarg"], vtarg[:, :, 0])
    adv0, _ = adapters.gae(r["reward_head"][:, :, 0:1], r["vf"][:, :, None], r["done"])
    assert not np.array_equal(r["adv"], adv0[:, :, 0])
    # a record of three fields: the same values, the bound buffers as after the full record
    _, env, _ = hr.make_env("S10U100", "256x256", "gauss_clip", B, **kw)
    _, full, _ = hr.make_env("S10U100", "256x256", "gauss_clip", B, **kw)
    part = env.collect_head(T, reward="colran", record=("action", "logp", "done"))
    full.collect_head(T, reward="colran")
    torch.cuda.synchronize()
    assert sorted(part) == ["action", "done", "logp"]
    for k in part:
        assert np.array_equal(part[k].cpu().numpy(), r[k]), k
    for k in ("head_obs", "head_reward", "done", "reward", "obs_inter"):
        assert torch.equal(getattr(env, k), getattr(full, k)), k
    env.close()
    full.close()


def test_a_critic_wider_and_deeper_than_its_actor():
    """Actor [48] (padded to 64: the other branch of the LDS row stride) under a critic [96, 96], so that the workgroup's LDS buffers are
    sized by the critic and not by the actor; B = 40 (two workgroups, a tail of 8), T = 3 with episodes ending at its last TTI.
    Fused and split give one record; vf (the bootstrap slot included), logp and the unclamped action lie within the float64 bounds."""
    need_gpu()
    B, n = 40, 3
    lengths = np.asarray((3, 2, 5, 1), dtype=np.int32)[np.arange(B) % 4]

    def make():
        _, env, (_, log_std, _) = hr.make_env("S5U25", "64x64", "gauss_clip", B, stochastic=True, seed=SEED, autoreset=True)
        actor = hr.mlp([10 * env.S, 48, env.S], "tanh", 41, hr.OUT_SCALE)
        critic = hr.mlp([10 * env.S, 96, 96, 1], "tanh", 43)
        env.set_head_policy_network(actor, "gauss_clip", log_std, stochastic=True, seed=SEED)
        env.set_head_value_network(critic)
        env.set_max_steps(lengths)
        env.reset()
        return env, (actor, log_std, critic)

    ref, _ = make()                # the Philox counters of every TTI, from a step() loop
    counters = []
    for _ in range(n):
        v = ref.views()
        counters.append((v["episode_number"].cpu().numpy().copy(), v["step_number"].cpu().numpy().copy()))
        ref.step()
    ref.close()
    recs = []
    for split in (0, 1):
        env, (actor, log_std, critic) = make()
        env.set_option("collect_split", split)
        r = {k: x.cpu().numpy().copy() for k, x in env.collect_head(n).items()}
        recs.append(r)
        assert r["done"][-1].any() and not r["done"][-1].all()
        worst = {"logp": 0.0, "vf": 0.0, "action": 0.0}
        for t in range(n + 1):
            obs = r["obs_head"][t] if t < n else env.head_obs.cpu().numpy()
            y, bound = hr.value_ref(obs, critic)
            err = np.abs(r["vf"][t] - y)
            assert np.all(err <= bound), f"vf[{t}]: worst {np.max(err / bound):.3g} of the bound"
            worst["vf"] = max(worst["vf"], float(np.max(err / bound)))
            if t == n:
                break
            z = hr.noise(np.arange(B), counters[t][0], counters[t][1], env.S, SEED)
            a = hr.HeadRef(obs, actor, "gauss_clip", log_std, z)
            err = np.abs(r["action"][t] - a.action)
            assert np.all(err <= a.action_bound), f"action[{t}]"
            worst["action"] = max(worst["action"], float(np.max(err / a.action_bound)))
            lp, lb = hr.logp_ref(log_std, z, B)
            err = np.abs(r["logp"][t].astype(np.float64) - lp)
            assert np.all(err <= lb), f"logp[{t}]: worst {np.max(err / lb):.3g} of the bound"
            worst["logp"] = max(worst["logp"], float(np.max(err / lb)))
        print(f"split {split}: worst error / bound {worst}")
        env.close()
    for k in recs[0]:
        assert np.array_equal(recs[0][k], recs[1][k]), k


# ---- 7. error paths, through the C ABI ------------------------------------------------------------------------------------------------
def test_error_paths():
    need_gpu()
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd._lib import RanEnvError
    E_INVALID, E_STATE = -1, -3
    B = 16
    wl, env, (actor, log_std, critic) = hr.make_env("S5U25", "64x64", "gauss_clip", B, bind=False, unsorted=False)
    lib, h, S = env._lib, env._h, env.S
    keep = []
    layers, act = hr.layers_of(actor)
    mlp = lambda ls=layers, a=act: env._mlp_struct(ls, a, _lib.NET_IN_OBS, keep)  # noqa: E731
    ls_dev = log_std.to(env.device)
    stream = env._stream()
    step = lambda: lib.ranenv_step(h, None, None, None, None, *env._p_out, stream)  # noqa: E731
    traj = _lib.HeadTrajectory()
    collect = lambda t=traj, col=0: lib.ranenv_collect_head(h, 4, C.byref(t), col, 0.99, 0.95, *env._p_out, stream)  # noqa: E731

    def snapshot():
        torch.cuda.synchronize()
        return {k: x.clone() for k, x in env.views().items()}, env.head_obs.clone(), env.head_reward.clone()

    def unchanged(before):
        torch.cuda.synchronize()
        views, ho, hrw = before
        return all(torch.equal(x, env.views()[k]) for k, x in views.items()) and torch.equal(ho, env.head_obs) and torch.equal(hrw, env.head_reward)

    before = snapshot()
    # the sorted tables are refused by the Python layer (SchedTWC runs unsorted) unless overridden
    with pytest.raises(RanEnvError):
        env.set_head_policy_network(actor, "gauss_clip", log_std)
    # set_policy accepts HEAD_NETWORK = 4 and nothing beyond
    assert lib.ranenv_set_policy(h, 5, _lib.INTRA_RR) == E_INVALID
    assert lib.ranenv_set_policy(h, _lib.POLICY_HEAD_NETWORK, _lib.INTRA_RR) == 0
    assert step() == E_STATE and b"head policy network" in lib.ranenv_last_error(h)                 # no head net bound
    assert lib.ranenv_rollout(h, 3, *env._p_out, stream) == E_STATE
    assert collect() == E_STATE
    # shapes and arguments of ranenv_set_head_policy_network
    bad_in = mlp([(torch.zeros(64, 10 * S + 1), layers[0][1])] + layers[1:])
    bad_out = mlp(layers[:-1] + [(torch.zeros(2 * S, 64), torch.zeros(2 * S))])
    wide = mlp([(torch.zeros(2048, 10 * S), torch.zeros(2048)), (torch.zeros(S, 2048), torch.zeros(S))])
    CLIP, TANH = _lib.HEAD_DIST_GAUSS_CLIP, _lib.HEAD_DIST_GAUSS_TANH
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for m, dist, lsp in ((bad_in, CLIP, p(ls_dev)), (bad_out, CLIP, p(ls_dev)), (wide, CLIP, p(ls_dev)), (mlp(), CLIP, None),
                         (mlp(), TANH, p(ls_dev)), (mlp(), TANH, None), (mlp(), 2, p(ls_dev)), (bad_out, TANH, p(ls_dev))):
        assert lib.ranenv_set_head_policy_network(h, C.byref(m), dist, lsp, 0, 0, stream) == E_INVALID
    assert lib.ranenv_set_head_policy_network(h, None, CLIP, p(ls_dev), 0, 0, stream) == E_INVALID
    assert step() == E_STATE                                                                          # still nothing bound
    vbad = mlp(layers)                                                                                # (S outputs: not a critic)
    assert lib.ranenv_set_head_value_network(h, C.byref(vbad), stream) == E_INVALID
    assert lib.ranenv_set_head_value_network(h, None, stream) == E_INVALID
    # a bound net but no head observation
    assert lib.ranenv_set_head_policy_network(h, C.byref(mlp()), CLIP, p(ls_dev), 1, 7, stream) == 0
    assert lib.ranenv_bind_head_outputs(h, None, None) == 0
    assert step() == E_STATE and b"dev_obs_head" in lib.ranenv_last_error(h)
    assert lib.ranenv_bind_head_outputs(h, p(env.head_obs), p(env.head_reward)) == 0
    # collect_head: no critic; bad arguments; the wrong policy on either side
    assert collect() == E_STATE and b"value" in lib.ranenv_last_error(h)
    vl, va = hr.layers_of(critic)
    assert lib.ranenv_set_head_value_network(h, C.byref(mlp(vl, va)), stream) == 0
    assert collect(col=2) == E_INVALID
    assert lib.ranenv_collect_head(h, 0, C.byref(traj), 0, 0.99, 0.95, *env._p_out, stream) == E_INVALID
    assert lib.ranenv_collect_head(h, 4, None, 0, 0.99, 0.95, *env._p_out, stream) == E_INVALID
    adv_only = _lib.HeadTrajectory()
    scratch = torch.zeros((5, B), dtype=torch.float32, device=env.device)
    adv_only.adv = scratch.data_ptr()
    assert collect(adv_only) == E_INVALID
    ctraj = _lib.Trajectory()
    assert lib.ranenv_collect(h, 4, C.byref(ctraj), 0.99, 0.95, *env._p_out, stream) == E_STATE      # ranenv_collect under HEAD_NETWORK
    assert lib.ranenv_set_policy(h, _lib.POLICY_NETWORK, _lib.INTRA_RR) == 0
    assert collect() == E_STATE                                                                       # ranenv_collect_head under NETWORK
    assert lib.ranenv_set_policy(h, _lib.POLICY_HEAD_NETWORK, _lib.INTRA_RR) == 0
    # SAC policies do not collect
    tanh_actor = hr.head_nets(S, "64x64", "gauss_tanh")[0]
    tl, ta = hr.layers_of(tanh_actor)
    assert lib.ranenv_set_head_policy_network(h, C.byref(mlp(tl, ta)), TANH, None, 1, 7, stream) == 0
    assert collect() == E_INVALID
    assert not scratch.any()
    assert unchanged(before)                                                                          # no refusal stepped or wrote anything
    # the heads refuse RANENV_F_NO_RAW_OUTPUT already
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    raw = make_mult_slice_workload(8, torch.device("cuda", 0), n_scenarios=4, n_traces=4, trace_len=16, flags=_lib.F_NO_RAW_OUTPUT,
                                   **hr.SIZES["S5U25"]).env
    with pytest.raises(RanEnvError):
        raw.enable_heads()
    raw.close()
    # ... and after all that the handle works
    assert step() == 0 and collect() == E_INVALID
    assert lib.ranenv_set_head_policy_network(h, C.byref(mlp()), CLIP, p(ls_dev), 1, 7, stream) == 0
    assert collect() == 0
    torch.cuda.synchronize()
    assert int(env.views()["step_number"].min()) == 5
    env.close()
