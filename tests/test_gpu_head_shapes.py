"""The head / off-policy kernel family on the device across the shape grid of tests/head_shapes_ref.py -- S 1, 3, 6, 8 and 16, Us up to
16, net widths off the 32 grid, depths 1 to 4, actor and critics differing: ranenv_sac_target_kernel, the head policies
(policy_body<HEAD>), ranenv_head_kernel against the CPU oracle, the replay ring and the sampler.

Beside the rigorous float64 bounds every numeric comparison carries the yardstick of ppo_update_ref.check_against_twin: per output
tensor, device error <= 8 x max(error of the float32 torch restatement, 1e-6), both relative in the 2-norm against the float64 reference.

Measured device / yardstick ratios (one MI355X; printed by the tests, worst over both modes; the bound is 8):
    case                    next_action  next_logp  q     target  head scores
    S1_7x100_96             2.11         1.49       0.77  0.86    0.20
    S3_96x160_33            0.11         0.03       0.13  0.03    0.36
    S6_40x24_160x7x96       0.09         0.03       0.10  0.02    0.18
    S8_255_511x1            0.28         0.03       0.01  0.03    0.38
    S16_256x256_480x33      0.18         0.03       0.36  0.03    0.47
    S16_64x4_100x7x255x32   0.06         0.03       0.28  0.02    0.19
    S16_512x512             0.51         0.03       0.28  0.02    0.60
    "inter" source, scores: 0.12 (S 1), 0.03 (S 16)
The floor 1e-6 is the denominator nearly everywhere (the restatement's own error is 2e-8 to 3e-7); S 1's log_std row is scaled up, so
its restatement errs by up to 3e-6 and the device by up to 6e-6.  Nothing comes near 8: the kernels' summation order is no finding.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import head_policy_ref as hr
from tests import head_shapes_ref as hs
from tests import inter_head_ref as ih
from tests import sac_ref as sr
from tests.common import OBS_TOL, REW_TOL
from tests.gpu_common import HEAD_OUTPUTS, LOOSE_WINDOWS_AND_SE, OUTPUTS, assert_same_state, need_gpu, to_host
from tests.test_gpu_replay import SENTINEL, _bound_ring, _step_loop

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9ABC
LENGTHS = (3, 2, 5, 1, 6, 4)                  # per env, cyclic: episodes end at every TTI of a 6-TTI record
RECORD_CASES = ("S1_7x100_96", "S16_256x256_480x33")
CASE_OF_S = {1: "S1_7x100_96", 3: "S3_96x160_33", 16: "S16_64x4_100x7x255x32"}
_state_equal = functools.partial(assert_same_state, loose=LOOSE_WINDOWS_AND_SE, outputs=OUTPUTS + HEAD_OUTPUTS, actions=("scores",))
_p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731


def _head_env(case, dist, B, stochastic=True, autoreset=False, parts=1, critic=True, observation="head", metrics=None):
    """head_policy_ref.make_env (inter_head_ref's under the "inter" source) at the case's environment shape, with the case's head nets
    bound in place of the named ones; autoreset: per-env episode lengths LENGTHS.  Returns (workload, env, (actor, log_std, critic))."""
    S = hs.CASES[case][0]
    kw = dict(stochastic=stochastic, seed=SEED, autoreset=autoreset, parts=parts, metrics=metrics, bind=False)
    if observation == "inter":
        wl, env, _ = ih.make_env(hs.ENV_SHAPES[S], "64x64", dist, B, **kw)
    else:
        wl, env, _ = hr.make_env(hs.ENV_SHAPES[S], "64x64", dist, B, **kw)
    assert env.S == S and env.Us == hs.ENV_SHAPES[S]["max_ues_slice"]
    actor, log_std, vnet = hs.head_nets(case, dist)
    env.set_head_policy_network(actor, dist, log_std, stochastic=stochastic, seed=SEED, observation=observation, allow_sorted=observation == "inter")
    if critic:
        env.set_head_value_network(vnet)
    if autoreset:
        env.set_max_steps(np.asarray(LENGTHS, dtype=np.int32)[np.arange(B) % len(LENGTHS)])
    env.reset()
    return wl, env, (actor, log_std, vnet)


# ---- 2. SAC targets -----------------------------------------------------------------------------------------------------------------
def _sac_env(case, B=8):
    c = hs.sac_case(case)
    _, env, _ = hr.make_env(hs.ENV_SHAPES[c["S"]], "64x64", "gauss_tanh", B, bind=False)
    actor, q1, q2 = c["nets"]
    env.set_head_policy_network(actor, "gauss_tanh", stochastic=True, seed=1)
    env.set_sac_critics(q1, q2)
    return env, c


def _targets_into(env, c, n, stochastic, extra=1, fill=-7.0):
    """ranenv_sac_targets on the first n rows into buffers ``extra`` rows longer, pre-filled: (outputs as numpy, with the extra rows)."""
    S, dev = env.S, env.device
    obs, reward, done = (torch.as_tensor(a[:n]).to(dev).contiguous() for a in (c["obs"], c["reward"], c["done"]))
    out = {k: torch.full(shape, fill, dtype=torch.float32, device=dev) for k, shape in (
        ("target", (n + extra,)), ("next_action", (n + extra, S)), ("next_logp", (n + extra,)), ("q", (n + extra, 2)))}
    st = env._lib.ranenv_sac_targets(env._h, n, _p(obs), _p(reward), _p(done), hs.GAMMA, hs.ENT_COEF, 1 if stochastic else 0, hs.SEED, hs.DRAW,
                                     *(_p(out[k]) for k in ("target", "next_action", "next_logp", "q")), env._stream())
    assert st == 0, env._lib.ranenv_last_error(env._h)
    torch.cuda.synchronize()
    return to_host(out)


@pytest.mark.parametrize("stochastic", [True, False])
@pytest.mark.parametrize("case", list(hs.CASES))
def test_sac_targets_bound_yardstick_and_exact_properties(case, stochastic):
    need_gpu()
    env, c = _sac_env(case)
    n, S = hs.N_ROWS, env.S
    ref, f32 = c["ref"][stochastic], c["got"][stochastic]
    args = (torch.as_tensor(c["obs"]), torch.as_tensor(c["reward"]), torch.as_tensor(c["done"]))
    got = to_host(env.sac_targets(*args, gamma=hs.GAMMA, ent_coef=hs.ENT_COEF, stochastic=stochastic, seed=hs.SEED, draw=hs.DRAW))
    assert got["target"].shape == (n,) and got["next_action"].shape == (n, S) and got["next_logp"].shape == (n,) and got["q"].shape == (n, 2)
    for k in hs.SAC_OUTPUTS:
        v, want, bound = got[k].astype(np.float64), getattr(ref, k), getattr(ref, k + "_bound")
        print(f"{case} stochastic={stochastic} {k}: worst error / bound {np.max(np.abs(v - want) / bound):.3g}, largest bound {bound.max():.3g}")
    sr.check_outputs(ref, got, case)                                                      # a. the rigorous bound
    hs.check_yardstick(got, ref, f32, f"{case} stochastic={stochastic}")                  # b. the yardstick
    d = c["done"] != 0                                                                    # c. exact properties
    assert d.any() and np.array_equal(got["target"][d], c["reward"][d])
    if not stochastic:
        assert np.all(np.abs(got["next_action"] - np.tanh(ref.mu)) <= ref.next_action_bound)
        assert np.array_equal(ref.z, np.zeros_like(ref.z))
    env.close()


@pytest.mark.parametrize("case", hs.TAIL_CASES)
def test_sac_target_row_tails(case):
    """n = 1, 31, 32, 33, 64, 65 rows: bit for bit the n-row prefix of the 80-row call, and the row behind the call's last keeps its
    sentinel in every output."""
    need_gpu()
    env, c = _sac_env(case)
    full = _targets_into(env, c, hs.N_ROWS, True)
    hs.check_yardstick({k: v[:hs.N_ROWS] for k, v in full.items()}, c["ref"][True], c["got"][True], f"{case} 80 rows")
    for n in hs.TAILS + (hs.N_ROWS,):
        part = _targets_into(env, c, n, True)
        for k, v in part.items():
            assert v.shape[0] == n + 1 and np.all(v[n] == -7.0), (k, n, "the row behind the call was written")
            assert np.array_equal(v[:n], full[k][:n]), (k, n, "not the prefix of the 80-row call")
    env.close()


# ---- 3. the head policies -------------------------------------------------------------------------------------------------------------
def _check_scores(env, obs, nets, dist, stochastic, counters, what):
    from intent_radio_sched_multi_slice_amd import adapters
    actor, log_std, _ = nets
    B = obs.shape[0]
    episode, step = counters
    dev = env.policy_actions()["scores"].cpu().numpy()
    z = hr.noise(np.arange(B), episode, step, env.S, SEED) if stochastic else None
    ref = hr.HeadRef(obs, actor, dist, log_std, z)
    worst = hr.check_scores(ref, dev, what)
    want, _ = adapters.head_policy_actions(obs, actor, dist, log_std, stochastic, SEED, env_ids=np.arange(B), episode=episode, step=step)
    hs.check_yardstick({"scores": dev}, {"scores": ref.scores}, {"scores": want.numpy()}, what, names=("scores",))
    assert np.all(np.abs(dev) <= 1.0)
    return ref, worst


@pytest.mark.parametrize("stochastic", [False, True])
@pytest.mark.parametrize("dist", ["gauss_clip", "gauss_tanh"])
@pytest.mark.parametrize("case", list(hs.CASES))
def test_head_forward_bound_and_yardstick(case, dist, stochastic):
    """Injected head observations, B = 70 (two workgroups and a tail of 6), two TTIs: every score inside HeadRef's bound, and the
    scores' error within the yardstick of adapters.head_policy_actions."""
    need_gpu()
    B = 70
    _, env, nets = _head_env(case, dist, B, stochastic=stochastic, critic=False)
    rng = np.random.default_rng(17)
    for t in range(2):
        obs = hr.injected_head_obs(rng, B, env.S)
        env.head_obs.copy_(torch.from_numpy(obs))
        counters = ih.counters(env)
        env.step()
        ref, worst = _check_scores(env, obs, nets, dist, stochastic, counters, f"{case} {dist} stochastic={stochastic} TTI {t}")
        print(f"TTI {t}: worst error / bound {worst:.3g}")
        assert (np.abs(ref.action) > 1.0).any() and (np.abs(ref.action) < 1.0).any()
    env.close()


@pytest.mark.parametrize("dist", ["gauss_clip", "gauss_tanh"])
@pytest.mark.parametrize("S", [1, 16])
def test_inter_source_forward(S, dist):
    """The head policy source "inter" at S 1 and S 16: the scores are the actor's on the obs_inter rows the step found (sorted tables)."""
    need_gpu()
    case = CASE_OF_S[S]
    _, env, nets = _head_env(case, dist, ih.B, stochastic=True, critic=False, observation="inter")
    assert env.head_observation == "inter" and getattr(env, "head_obs", None) is None
    for t in range(3):
        torch.cuda.synchronize()
        obs = env.obs_inter.cpu().numpy().copy()
        counters = ih.counters(env)
        env.step()
        _check_scores(env, obs, nets, dist, True, counters, f"inter {case} {dist} TTI {t}")
    env.close()


@pytest.mark.parametrize("stochastic", [False, True])
@pytest.mark.parametrize("case", RECORD_CASES)
def test_head_record_is_the_step_loop(case, stochastic):
    """collect_head(6) under auto-reset over 1 and 3 partitions at S 1 and S 16 records what a step() loop on a twin sees, as
    test_gpu_head_policy asserts it: observations, rewards and done bit for bit, the clamped action the loop's scores; logp and vf
    inside logp_ref / value_ref; adv / vtarg adapters.gae on the recorded column bit for bit; the state is rollout(6)'s."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd import adapters
    B, T = 50, 6
    kw = dict(stochastic=stochastic, autoreset=True, metrics=8)
    wl, ref, (actor, log_std, critic) = _head_env(case, "gauss_clip", B, **kw)
    want = {k: [] for k in ("obs_head", "scores", "reward_head", "done")}
    counters = []
    for _ in range(T):
        counters.append(ih.counters(ref))
        want["obs_head"].append(ref.head_obs.clone())
        ref.step()
        for k, x in (("scores", ref.policy_actions()["scores"]), ("reward_head", ref.head_reward), ("done", ref.done)):
            want[k].append(x.clone())
    want = {k: torch.stack(x) for k, x in want.items()}
    d = want["done"].cpu().numpy()
    assert d[-1].any() and not d.all(axis=1).any() and len({int(np.argmax(d[:, b])) for b in range(B) if d[:, b].any()}) >= 4
    for parts in (1, 3):
        _, env, _ = _head_env(case, "gauss_clip", B, parts=parts, **kw)
        _, roll, _ = _head_env(case, "gauss_clip", B, parts=parts, **kw)
        rec = env.collect_head(T, reward="twc", gamma=0.97, lam=0.9)
        roll.rollout(T)
        torch.cuda.synchronize()
        for k in ("obs_head", "reward_head", "done"):
            assert rec[k].shape == want[k].shape and torch.equal(rec[k], want[k]), (k, parts)
        assert torch.equal(rec["action"].clamp(-1.0, 1.0), want["scores"]), parts
        r = to_host(rec)
        worst = {"logp": 0.0, "vf": 0.0, "action": 0.0}
        for t in range(T + 1):
            obs = r["obs_head"][t] if t < T else env.head_obs.cpu().numpy()
            y, bound = hr.value_ref(obs, critic)
            err = np.abs(r["vf"][t] - y)
            assert np.all(err <= bound), f"vf[{t}]: worst {np.max(err / bound):.3g} of the bound"
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
        print(f"{case} parts {parts}: worst error / bound {worst}")
        adv, vtarg = adapters.gae(r["reward_head"][:, :, 0:1], r["vf"][:, :, None], r["done"], 0.97, 0.9)
        assert np.array_equal(r["adv"], adv[:, :, 0]) and np.array_equal(r["vtarg"], vtarg[:, :, 0]), parts
        _state_equal(env, roll, wl.tables, (case, parts))
        env.close()
        roll.close()
    ref.close()


# ---- 4. the head kernel against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3, 16])
def test_head_kernel_matches_the_oracle_on_directed_member_counts(S):
    """20 TTIs of 9 envs on scenario tables whose slices hold 0, 1, 7, 8, 9, 15 and 16 UEs (Us 16): one head wave at S 1 and S 3, four
    at S 16; the slice means run np_sum16_lds through a partial block, one block, one block and a tail, and two blocks without a
    tail.  The device's own scores drive the CPU oracle: integers exact, the head observation and both head rewards at
    test_gpu_head_policy.test_env_parity_with_oracle's tolerances."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.batched_env import BatchedRanEnv
    from intent_radio_sched_multi_slice_amd.workloads import mimic_quadriga_pool, poisson_traffic_pool
    from oracle import pyoracle
    B, steps, R, n_traces, L = 9, 20, 25, 4, 24
    U, Us = hs.ENV_SHAPES[S]["n_ues"], 16
    tables, scen_counts = hs.directed_tables(S, U, Us)
    n_scen = len(scen_counts)
    dev = torch.device("cuda", 0)
    env = BatchedRanEnv(batch=B, n_slices=S, n_ues=U, n_rbs=R, rbs_per_rbg=1, max_ues_slice=Us, n_scenarios=n_scen, max_steps=1000, device=dev)
    env.load_scenarios(tables)
    se_pool = mimic_quadriga_pool(n_traces, L, U, R, 77 + S, env.device)
    trf = poisson_traffic_pool(tables, L, 9)
    env.bind_se_pool(se_pool)
    env.bind_traffic_pool(torch.from_numpy(trf).to(env.device))
    rng = np.random.default_rng(5 + S)
    scen, trace = np.arange(B) % n_scen, np.arange(B) % n_traces
    se_off, trf_off = rng.integers(0, L, B), rng.integers(0, L, B)
    env.set_episodes(scenario=scen, se_base=trace * L, se_len=L, se_offset=se_off, trf_base=scen * L, trf_len=L, trf_offset=trf_off)
    env.set_policy(_lib.POLICY_MAPF, _lib.INTRA_RR)
    uc = hr.usecase_of(tables)
    env.enable_heads(uc)
    played = np.asarray(scen_counts)[scen]
    assert (played == 16).any() and (S == 1 or (played == 0).any()), "no 16-UE slice / no empty slice among the envs' scenarios"
    assert set(played.reshape(-1).tolist()) == set(hs.MEMBER_COUNTS) - ({0} if S == 1 else set())
    actor = hr.mlp([10 * S, 33, S], "tanh", 41, hr.OUT_SCALE)
    log_std = torch.linspace(-1.0, 0.5, S).to(torch.float32)
    env.set_head_policy_network(actor, "gauss_clip", log_std, stochastic=True, seed=3)
    env.reset()
    cfg = pyoracle.make_cfg(env.S, env.U, env.R, env.G, env.Us, max_steps=1000)
    se_host = se_pool.transpose(1, 2).contiguous().cpu().numpy()
    trf_host = trf.astype(np.float64)
    oenvs = []
    for b in range(B):
        e = pyoracle.OracleEnv(cfg)
        e.set_scenario(tables, int(scen[b]))
        e.reset(se_host[int(trace[b] * L + se_off[b] % L)])
        oenvs.append(e)
    rr = np.zeros(S, dtype=np.int32)
    saw_twc = saw_col = False
    for t in range(steps):
        obs, rew, _ = env.step()
        sc = env.policy_actions()["scores"].cpu().numpy()
        v = {k: x.cpu().numpy() for k, x in env.views().items()}
        oi, rw = obs["obs_inter"].cpu().numpy(), rew.cpu().numpy()
        ho, hrw = env.head_obs.cpu().numpy(), env.head_reward.cpu().numpy()
        for b, e in enumerate(oenvs):
            e.step(sc[b].copy(), rr, se_host[int(trace[b] * L + (se_off[b] + t) % L)], trf_host[int(scen[b] * L + (trf_off[b] + t) % L)])
            raw, o = e.raw(), e.obs()
            for k in ("pkt_effective_thr", "dropped_pkts", "pkt_throughputs"):
                assert np.array_equal(v[k][b], raw[k]), (k, t, b)
            np.testing.assert_allclose(oi[b], o["obs_inter"], rtol=0, atol=OBS_TOL)
            np.testing.assert_allclose(rw[b], o["reward"], rtol=0, atol=REW_TOL)
            h_obs, r_twc, r_col = e.heads(uc[int(scen[b])])
            np.testing.assert_allclose(ho[b], h_obs, rtol=2e-6, atol=OBS_TOL, err_msg=str((t, b)))
            np.testing.assert_allclose(hrw[b], [r_twc, r_col], rtol=0, atol=REW_TOL, err_msg=str((t, b)))
            saw_twc |= r_twc != 0
            saw_col |= r_col != 0
    assert saw_twc and saw_col
    env.close()


# ---- 5. the replay ring and the sampler -----------------------------------------------------------------------------------------------
RING_B, RING_CAP, RING_T = 40, 5, 3           # two calls of 3 TTIs into 5 slots: the second wraps


def _sample_into(env, n, seed, draw, col):
    """ranenv_replay_sample into buffers one row longer, pre-filled with sentinels: dict of device tensors (n + 1 rows)."""
    S, dev = env.S, env.device
    out = {"obs": torch.full((n + 1, 10 * S), -7.0, device=dev), "action": torch.full((n + 1, S), -7.0, device=dev),
           "reward": torch.full((n + 1,), -7.0, device=dev), "next_obs": torch.full((n + 1, 10 * S), -7.0, device=dev),
           "done": torch.full((n + 1,), 255, dtype=torch.uint8, device=dev), "index": torch.full((n + 1,), -7, dtype=torch.int64, device=dev)}
    st = env._lib.ranenv_replay_sample(env._h, n, seed, draw, col, *(_p(out[k]) for k in ("obs", "action", "reward", "next_obs", "done", "index")),
                                       env._stream())
    assert st == 0, env._lib.ranenv_last_error(env._h)
    torch.cuda.synchronize()
    return out


def _check_samples(env, ring, written, cols):
    from intent_radio_sched_multi_slice_amd import adapters
    B = env.B
    flat = {k: t.reshape((RING_CAP * B,) + t.shape[2:]) for k, t in ring.items()}
    for n in (1, 15, 16, 17, 100):
        for col in cols:
            got = _sample_into(env, n, 9, 4 + n, col)
            idx = adapters.replay_sample_index(n, 9, 4 + n, written, RING_CAP, B)
            assert idx.max() < min(written, RING_CAP) * B
            assert np.array_equal(got["index"][:n].cpu().numpy(), idx), (n, col)
            ix = torch.as_tensor(idx, device=env.device)
            assert torch.equal(got["obs"][:n], flat["obs"][ix]) and torch.equal(got["next_obs"][:n], flat["next_obs"][ix]), (n, col)
            assert torch.equal(got["done"][:n], flat["done"][ix]), (n, col)
            assert torch.equal(got["action"][:n], flat["action"][ix].to(torch.float32)), (n, col)
            assert torch.equal(got["reward"][:n], flat["reward_head"][ix, col].to(torch.float32)), (n, col)
            assert not bool((got["obs"][:n] == SENTINEL["obs"]).any())
            for k, t in got.items():                           # the row behind the call's last keeps its sentinel
                assert bool((t[n] == (255 if k == "done" else -7)).all()), (k, n, col)


@pytest.mark.parametrize("S", [1, 16])
def test_ring_is_the_step_loop_and_the_sampler_gathers_its_rows(S):
    """S 1 (an observation row of 5 words, fewer than the sampler's 16 lanes) and S 16 (80 words: five passes); B = 40."""
    need_gpu()
    case = CASE_OF_S[S]
    kw = dict(stochastic=True, autoreset=True, critic=False)
    _, ref, _ = _head_env(case, "gauss_tanh", RING_B, **kw)
    want = _step_loop(ref, 2 * RING_T)
    d = want["done"].cpu().numpy()
    assert d[:RING_T].any() and d[RING_T:].any() and not d.all(axis=1).any()
    _, env, _ = _head_env(case, "gauss_tanh", RING_B, **kw)
    ring = _bound_ring(env, RING_CAP)
    assert ring["obs"].shape == (RING_CAP, RING_B, 10 * S) and env.replay_count() == 0
    for call in (1, 2):
        env.collect_replay(RING_T)
        torch.cuda.synchronize()
        n = call * RING_T
        assert env.replay_count() == n
        for slot in range(RING_CAP):
            ks = [k for k in range(n) if k % RING_CAP == slot]
            for f, t in ring.items():
                if ks:
                    assert torch.equal(t[slot], want[f][ks[-1]]), (f, slot, call)
                else:
                    assert bool((t[slot] == SENTINEL[f]).all()), (f, slot, call)
        _check_samples(env, ring, n, cols=(0, 1))
    env.close()
    ref.close()


def test_sampler_reward_columns_under_the_inter_source_at_S16():
    """The ring's reward rows have S + 1 = 17 columns under the "inter" source: the sampler reads column 0 and column S."""
    need_gpu()
    S = 16
    _, env, _ = _head_env(CASE_OF_S[S], "gauss_tanh", RING_B, stochastic=True, autoreset=True, critic=False, observation="inter")
    ring = _bound_ring(env, RING_CAP)
    assert ring["reward_head"].shape == (RING_CAP, RING_B, S + 1)
    env.collect_replay(RING_T)
    env.collect_replay(RING_T)
    torch.cuda.synchronize()
    assert env.replay_count() == 2 * RING_T
    assert not torch.equal(ring["reward_head"][:, :, 0], ring["reward_head"][:, :, S])
    _check_samples(env, ring, 2 * RING_T, cols=(0, S))
    env.close()
