"""SE gather mode (ranenv_set_se_mode), range stepping for a learner in the loop (ranenv_step_range: step_async /
step_wait), and the regressions of the round-2 advisor findings: head rewards at an auto-reset, device policy with a
per-step intra-slice choice.  All through the C ABI, against the oracle; integers bit-exact, observations 1e-5, rewards 1e-9.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.common import OBS_TOL, REW_TOL, oracle_envs, poisson_traffic_rows, rb_major
from tests.gpu_common import LOOSE_SE_MEAN, assert_same_state, bench_like, comparable_views, need_gpu, short_episode_setup
from tests.synth import se_tile

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", [dict(U=7, R=5), dict(U=37, R=100), dict(U=100, R=135), dict(U=128, R=300),
                                   dict(U=64, R=408), dict(U=256, R=64)])
def test_gather_sidecars_are_numpy_means_and_the_transposed_pool(shape):
    """row_mean[tile][u] must be np.mean(SE[u, :]) of the float32 tile in float64 -- numpy's pairwise order, every
    shape of it -- bit for bit (the oracle's orc_np_sum is the checker); ue_major is the tile transposed, rows
    zero-padded to a multiple of 8."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd.batched_env import BatchedRanEnv
    from oracle import pyoracle
    U, R = shape["U"], shape["R"]
    S, Us = 4, 4
    n_tiles = 9
    pool = np.stack([se_tile(11, t, U, R) for t in range(n_tiles)])          # [tiles, U, R]
    env = BatchedRanEnv(batch=2, n_slices=S, n_ues=U, n_rbs=R, rbs_per_rbg=1, max_ues_slice=Us, n_scenarios=1, max_steps=4)
    env.bind_se_pool(torch.as_tensor(rb_major(pool), device=env.device))
    env.set_se_mode("gather")
    sc = env.se_sidecars()
    mean, um = sc["row_mean"].cpu().numpy(), sc["ue_major"].cpu().numpy()
    Rp = (R + 7) // 8 * 8
    assert um.shape == (n_tiles, U, Rp)
    assert np.array_equal(um[:, :, :R], pool) and not um[:, :, R:].any()
    for t in range(n_tiles):
        for u in range(U):
            assert mean[t, u] == pyoracle.np_sum(pool[t, u].astype(np.float64)) / R, (t, u)
    # numpy itself, where its pairwise blocking is the documented one (contiguous float64 rows)
    np.testing.assert_array_equal(mean, pool.astype(np.float64).mean(axis=2))
    env.close()


def test_gather_equals_stream_at_full_size():
    """BASELINE configs[2] (B 4096, S 10 / U 100 / R 135, MAPF + PF) stepped 40 TTIs in both SE modes -- step by step and
    as a rollout over 3 partitions: every state array, observation and reward must be bit-identical."""
    need_gpu()
    B, T = 4096, 40
    a, b, c = bench_like(B, False), bench_like(B, True), bench_like(B, True)
    assert (a.env.se_mode, b.env.se_mode) == ("stream", "gather")
    a.env.reset(); b.env.reset(); c.env.reset()
    assert torch.equal(a.env.obs_inter, b.env.obs_inter) and torch.equal(a.env.obs_intra, b.env.obs_intra)
    for t in range(T):
        a.env.step(); b.env.step()
        if t in (0, 1, 9, T - 1):
            vb = comparable_views(b)
            for k, x in comparable_views(a).items():
                assert torch.equal(x, vb[k]), (t, k)
            assert torch.equal(a.env.obs_inter, b.env.obs_inter) and torch.equal(a.env.obs_intra, b.env.obs_intra), t
            assert torch.equal(a.env.reward, b.env.reward), t
    c.env.set_partitions(3)
    c.env.rollout(T)
    torch.cuda.synchronize()
    vc = comparable_views(c)
    for k, x in comparable_views(a).items():
        assert torch.equal(x, vc[k]), k
    assert torch.equal(a.env.obs_inter, c.env.obs_inter) and torch.equal(a.env.reward, c.env.reward)
    # an allocation that hands one UE many RBs and others none did occur (ranges of 0 RBs and ranges across several 8-groups both walked)
    cnt = a.env.views()["rb_count"]
    assert int(cnt.max()) > 8 and int((cnt == 0).sum()) > 0
    for w in (a, b, c):
        w.env.close()


def test_gather_mode_keeps_streaming_for_explicit_tiles_and_dense_steps():
    """In gather mode a step with explicit se_tiles and a dense step still read whole rows (streaming kernel): same
    results as an env in stream mode; rebinding a pool falls back to stream."""
    need_gpu()
    B = 6
    a, b = bench_like(B, False, steps=8), bench_like(B, True, steps=8)
    U, R, S = a.env.U, a.env.R, a.env.S
    rng = np.random.default_rng(3)
    a.env.set_policy(0, 255); b.env.set_policy(0, 255)
    a.env.reset(); b.env.reset()
    for t in range(6):
        sc = torch.as_tensor(rng.uniform(-1, 1, (B, S)), device=a.env.device)
        ic = torch.as_tensor(rng.integers(0, 3, (B, S)).astype(np.uint8), device=a.env.device)
        if t % 3 == 0:      # pooled tile
            a.env.step(sc, ic); b.env.step(sc, ic)
        elif t % 3 == 1:    # explicit tile
            se = torch.as_tensor(np.stack([rb_major(se_tile(77 + t, e, U, R)) for e in range(B)]), device=a.env.device)
            a.env.step(sc, ic, se_tiles=se); b.env.step(sc, ic, se_tiles=se)
        else:               # dense decision made from the pooled tile's allocation of the other env
            st, cn = a.env.views()["rb_start"].cpu().numpy(), a.env.views()["rb_count"].cpu().numpy()
            dense = np.zeros((B, U, R), dtype=np.uint8)
            for e in range(B):
                for u in range(U):
                    dense[e, u, st[e, u]:st[e, u] + cn[e, u]] = 1
            a.env.step_dense(dense); b.env.step_dense(dense)
        vb = comparable_views(b)
        for k, x in comparable_views(a).items():
            assert torch.equal(x, vb[k]), (t, k)
        assert torch.equal(a.env.obs_intra, b.env.obs_intra) and torch.equal(a.env.reward, b.env.reward), t
    b.env.bind_se_pool(b.se_pool)
    assert b.env.se_mode == ("gather" if os.environ.get("RANENV_SE_MODE") == "gather" else "stream")
    a.env.close(); b.env.close()


@pytest.mark.parametrize("se_mode,policy_on", [("stream", "caller"), ("gather", "caller"), ("stream", "range"), ("gather", "range")])
def test_two_halves_stepped_alternately_with_scores_from_the_callers_stream(se_mode, policy_on):
    """A learner in the loop: the batch as two halves on two streams (set_ranges / step_async / step_wait).  The scores
    of a half are produced from that half's last observation (a stand-in policy: a function of the observation, so any
    ordering slip between the streams changes the numbers) -- on the caller's one stream (events join the streams) or on
    the half's own stream (range_stream: stream order alone) --, 30 TTIs, against the oracle."""
    need_gpu()
    import contextlib
    from intent_radio_sched_multi_slice_amd.scenario import generate_scaled_scenarios
    S, U, R, G, Us, B, steps = 10, 100, 135, 1, 10, 48, 30
    tabs = generate_scaled_scenarios(6, seed=4)
    rng = np.random.default_rng(17)
    scen = rng.integers(0, tabs.n_scenarios, B)
    trace_len, n_traces = 32, 5
    se_pool = np.stack([se_tile(60 + i // trace_len, i % trace_len, U, R) for i in range(n_traces * trace_len)])
    trf = np.concatenate([poisson_traffic_rows(tabs, int(scen[b]), rng, trace_len) for b in range(B)])
    se_trace, se_off = rng.integers(0, n_traces, B), rng.integers(0, trace_len, B)
    from intent_radio_sched_multi_slice_amd.batched_env import BatchedRanEnv
    env = BatchedRanEnv(batch=B, n_slices=S, n_ues=U, n_rbs=R, rbs_per_rbg=G, max_ues_slice=Us,
                        n_scenarios=tabs.n_scenarios, max_steps=steps)
    env.load_scenarios(tabs)
    env.bind_se_pool(torch.as_tensor(rb_major(se_pool), device=env.device))
    env.bind_traffic_pool(torch.as_tensor(trf.astype(np.int32), device=env.device))
    env.set_episodes(scenario=scen, se_base=se_trace * trace_len, se_len=trace_len, se_offset=se_off,
                     trf_base=np.arange(B) * trace_len, trf_len=trace_len)
    env.set_policy(0, 1)                      # caller's inter-slice scores, PF inside the slices
    if se_mode == "gather":
        env.set_se_mode("gather")
    ranges = env.set_ranges(2)
    assert ranges == [(0, 24), (24, 48)]
    on = (lambda k: torch.cuda.stream(env.range_stream(k))) if policy_on == "range" else (lambda k: contextlib.nullcontext())
    oenvs = oracle_envs(tabs, scen, (S, U, R, G, Us), steps)
    for b, o in enumerate(oenvs):
        o.reset(se_pool[se_trace[b] * trace_len + se_off[b]])
    env.reset()

    def policy_dev(obs_inter):               # [n, S*10] float32 -> [n, S] float64 in [-1, 1], on the current stream
        x = obs_inter.view(-1, S, 10).to(torch.float64)
        return torch.tanh(x[:, :, 0] + 0.5 * x[:, :, 1] - x[:, :, 2] + 0.25 * x[:, :, 9])

    def policy_host(o):                      # the same function on the oracle's observation (float32-rounded like the device's)
        x = o["obs_inter"].astype(np.float32).astype(np.float64).reshape(S, 10)
        return np.tanh(x[:, 0] + 0.5 * x[:, 1] - x[:, 2] + 0.25 * x[:, 9])

    scores = torch.zeros((B, S), dtype=torch.float64, device=env.device)
    ic = np.ones(S, dtype=np.int32)
    # prime the pipeline: both halves get their first TTI from the reset observation
    in_flight = [None, None]                  # the scores a half's TTI in flight was launched with (host copy: exact)
    torch.cuda.synchronize()                  # the reset ran on the caller's stream
    for k, (lo, hi) in enumerate(ranges):
        with on(k):
            scores[lo:hi] = policy_dev(env.obs_inter[lo:hi])
            in_flight[k] = scores[lo:hi].cpu().numpy()
            env.step_async(k, scores, None)   # intra-slice scheduler fixed by set_policy
    host_obs = [o.obs() for o in oenvs]
    for k, (lo, hi) in enumerate(ranges):
        for j, b in enumerate(range(lo, hi)):
            np.testing.assert_allclose(in_flight[k][j], policy_host(host_obs[b]), rtol=0, atol=1e-5)
    t_of = [0, 0]
    for it in range(2 * (steps - 1)):
        k = it % 2
        lo, hi = ranges[k]
        with on(k):
            obs, rew, done = env.step_wait(k)
            # this half's next scores from its new observation; what the host checks below is copied out before the
            # next TTI of the half is enqueued
            scores[lo:hi] = policy_dev(obs["obs_inter"])
            got_sc = scores[lo:hi].cpu().numpy()
            g = {n: x[lo:hi].cpu().numpy() for n, x in env.views().items() if x.shape[0] == B}
            goi, goa, grw = obs["obs_inter"].cpu().numpy(), obs["obs_intra"].cpu().numpy(), rew.cpu().numpy()
            env.step_async(k, scores, None)
        # oracle: the TTI that was in flight for this half, with the very scores the device used
        sc_host = in_flight[k]
        for j, b in enumerate(range(lo, hi)):
            o = oenvs[b]
            tile = se_trace[b] * trace_len + (se_off[b] + t_of[k]) % trace_len
            o.step(sc_host[j], ic, se_pool[tile], trf[b * trace_len + t_of[k] % trace_len])
            host_obs[b] = o.obs()
        t_of[k] += 1
        in_flight[k] = got_sc
        for j, b in enumerate(range(lo, hi)):
            raw, oo = oenvs[b].raw(), host_obs[b]
            for name in ("pkt_incoming", "pkt_throughputs", "pkt_effective_thr", "dropped_pkts"):
                assert np.array_equal(g[name][j].astype(np.float64), raw[name]), (it, b, name)
            np.testing.assert_allclose(goi[j], oo["obs_inter"], rtol=0, atol=OBS_TOL)
            np.testing.assert_allclose(goa[j], oo["obs_intra"], rtol=0, atol=OBS_TOL)
            np.testing.assert_allclose(grw[j], oo["reward"], rtol=0, atol=REW_TOL)
            np.testing.assert_allclose(got_sc[j], policy_host(oo), rtol=0, atol=1e-5)
    for k in range(2):
        with on(k):
            env.step_wait(k)
    torch.cuda.synchronize()
    env.close()


def test_step_range_argument_checks():
    need_gpu()
    from intent_radio_sched_multi_slice_amd._lib import RanEnvError
    wl = bench_like(8, False, steps=4)
    env = wl.env
    with pytest.raises(RanEnvError, match="set_ranges"):
        env.step_async(0)
    env.set_ranges(2)
    with pytest.raises(RanEnvError, match="contiguous"):
        env.step_async(0, inter_scores=torch.zeros((4, env.S), dtype=torch.float64, device=env.device))
    st = env._lib.ranenv_step_range(env._h, 6, 4, None, None, None, None, None, None, None, None, None)
    assert st == -1 and b"outside the batch" in env._lib.ranenv_last_error(env._h)
    st = env._lib.ranenv_step_part(env._h, 2, None, None, None, None, None, None, None, None, None)
    assert st == -1 and b"partition 2 outside" in env._lib.ranenv_last_error(env._h)
    assert env._lib.ranenv_wait_part(env._h, -1, None) == -1
    # ranenv_step_range itself (any range, the caller's own stream): the second half alone moves on, the first stays
    before = env.views()["step_number"].clone()
    st = env._lib.ranenv_step_range(env._h, 4, 4, None, None, None, None, *env._p_out, None)
    assert st == 0
    torch.cuda.synchronize()
    assert (env.views()["step_number"] - before).cpu().tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    env.close()


def test_device_policy_with_a_random_intra_choice_every_step():
    """ranenv_step(scores = NULL, intra_choice = X_t) with fixed_intra = PER_SLICE: MAPF scores on the device, the
    caller picks every slice's scheduler anew every TTI.  An allocation made ahead at the end of TTI t would have used
    X_t for TTI t+1."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd.batched_env import BatchedRanEnv
    from intent_radio_sched_multi_slice_amd.scenario import generate_scaled_scenarios
    S, U, R, G, Us, B, steps = 5, 25, 135, 5, 5, 32, 24
    tabs = generate_scaled_scenarios(6, seed=3, n_slices=S, n_ues=U, max_ues_slice=Us, min_slices=3, min_ues=2)
    rng = np.random.default_rng(5)
    scen = rng.integers(0, tabs.n_scenarios, B)
    se_pool = np.stack([se_tile(41, t, U, R) for t in range(B * steps)])
    trf = np.concatenate([poisson_traffic_rows(tabs, int(scen[b]), rng, steps) for b in range(B)])
    for policy in (1, 2):
        env = BatchedRanEnv(batch=B, n_slices=S, n_ues=U, n_rbs=R, rbs_per_rbg=G, max_ues_slice=Us,
                            n_scenarios=tabs.n_scenarios, max_steps=steps)
        env.load_scenarios(tabs)
        env.bind_se_pool(torch.as_tensor(rb_major(se_pool), device=env.device))
        env.bind_traffic_pool(torch.as_tensor(trf.astype(np.int32), device=env.device))
        env.set_episodes(scenario=scen, se_base=np.arange(B) * steps, se_len=steps, trf_base=np.arange(B) * steps, trf_len=steps)
        env.set_policy(policy, 255)
        oenvs = oracle_envs(tabs, scen, (S, U, R, G, Us), steps)
        for b, o in enumerate(oenvs):
            o.reset(se_pool[b * steps])
        env.reset()
        for t in range(steps):
            ic = rng.integers(0, 3, (B, S)).astype(np.uint8)
            obs, rew, done = env.step(None, ic)
            g = {k: x.cpu().numpy() for k, x in env.views().items()}
            for b, o in enumerate(oenvs):
                sc = o.policy_marr() if policy == 1 else o.policy_mapf()
                _, count, _ = o.action_format(sc, ic[b], want_dense=False)
                assert np.array_equal(g["rb_count"][b], count), (policy, t, b)
                o.step(sc, ic[b], se_pool[b * steps + t], trf[b * steps + t])
                raw = o.raw()
                for name in ("pkt_throughputs", "pkt_effective_thr", "dropped_pkts"):
                    assert np.array_equal(g[name][b].astype(np.float64), raw[name]), (policy, t, b, name)
                np.testing.assert_allclose(rew[b].cpu().numpy(), o.obs()["reward"], rtol=0, atol=REW_TOL)
        env.close()


def test_head_reward_of_the_terminal_transition_survives_the_device_autoreset():
    """HeadVecEnv with device auto-reset must hand SB3 the reward of the terminal transition, not the reward of the
    freshly reset state: same rewards (and dones) as the host-side reset path at every step, including `done` steps."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd.adapters import HeadVecEnv
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload

    def make():
        wl = make_mult_slice_workload(8, torch.device("cuda", 0), policy=2, intra=1, n_scenarios=6, n_traces=12, trace_len=10,
                                      n_slices=5, n_ues=25, n_rbs=135, rbs_per_rbg=5, max_ues_slice=10, max_steps=6)
        ep_no = np.arange(0, 6)
        wl.env.set_episode_table(scenario=ep_no % 6, se_base=ep_no * 10, se_len=10, trf_base=(ep_no % 6) * 10, trf_len=10)
        start = np.arange(8) % 6
        t = wl.env.episode_table[start]
        wl.env.set_episodes(scenario=t["scenario"], se_base=t["se_base"], se_len=t["se_len"], se_offset=t["se_offset"],
                            trf_base=t["trf_base"], trf_len=t["trf_len"], trf_offset=t["trf_offset"])
        return wl, start
    for reward in ("twc", "colran"):
        wa, start = make()
        wb, _ = make()
        uc = np.tile(np.array([1, 2, 1, 3, 0], dtype=np.int32), (6, 1))
        va, vb = HeadVecEnv(wa.env, reward=reward, slice_usecase=uc), HeadVecEnv(wb.env, reward=reward, slice_usecase=uc)
        va.enable_device_autoreset(0, 6, episode_numbers=start)
        va.reset(); vb.reset()
        rng = np.random.default_rng(2)
        for t in range(6):                       # one episode: the host path cannot follow the device's episode advance
            act = rng.uniform(-1, 1, (8, wa.env.S))
            oa, ra, da, ia = va.step(act)
            ob, rb, db, ib = vb.step(act)
            assert np.array_equal(da, db), t
            np.testing.assert_array_equal(ra, rb)
            if da.any():
                assert np.abs(ra).sum() > 0
                for i in np.nonzero(da)[0]:
                    np.testing.assert_array_equal(ia[i]["terminal_observation"], ib[i]["terminal_observation"])
        va.close(); vb.close()


# ---------------------------------------------------------------------------------------------- compact steps
@pytest.mark.parametrize("steps,idle_traffic,se_mode", [(4, False, "stream"), (4, False, "gather"), (13, False, "stream"),
                                                         (4, True, "stream"), (13, True, "gather")])
def test_compact_steps_against_the_oracle_through_scenario_changes(steps, idle_traffic, se_mode):
    """A step touches only the UEs that are in a slice when the traffic traces carry nothing for the others (compact mode;
    the library examines the pool).  Episodes shorter than the 10-TTI window, the scenario changing at every auto-reset:
    a UE that sat out an episode comes back with exactly the zeros it would have pushed into its window (MAPF and PF read
    it).  With bits for idle UEs in the pool the steps must stay full width: those UEs queue, age and drop packets like
    the reference's.  Everything against the oracle, which steps every UE every TTI."""
    need_gpu()
    from oracle import pyoracle
    B = 12
    env, tabs, se_pool, trf, start, (S, U, R, G, Us, n_ep, L) = short_episode_setup(B, steps, idle_traffic, se_mode)
    cfg = pyoracle.make_cfg(S, U, R, G, Us, max_steps=10 ** 6)
    oenvs, cur, tstep = [], start.copy(), np.zeros(B, dtype=int)
    for b in range(B):
        o = pyoracle.OracleEnv(cfg); o.set_scenario(tabs, int(cur[b] % tabs.n_scenarios)); o.reset(se_pool[cur[b] * L]); oenvs.append(o)
    env.reset()
    intra = np.ones(S, dtype=np.int32)
    saw_idle_packets = False
    for it in range(5 * steps):
        obs, rew, done = env.step()
        g = {k: x.cpu().numpy() for k, x in env.views().items()}
        ro = {k: x.cpu().numpy() for k, x in env.raw_observation().items()}
        oi, rw = obs["obs_inter"].cpu().numpy(), rew.cpu().numpy()
        for b, o in enumerate(oenvs):
            o.step(o.policy_mapf(), intra, se_pool[cur[b] * L + tstep[b]], trf[cur[b] * L + tstep[b]])
            tstep[b] += 1
            oo, raw = o.obs(), o.raw()
            np.testing.assert_allclose(rw[b], oo["reward"], rtol=0, atol=REW_TOL, err_msg=str((it, b)))
            if tstep[b] < steps:
                for name in ("pkt_incoming", "pkt_throughputs", "pkt_effective_thr", "dropped_pkts"):
                    assert np.array_equal(g[name][b].astype(np.float64), raw[name]), (it, b, name)
                assert np.array_equal(ro["buffer_occupancies"][b], raw["buffer_occupancies"]), (it, b)
                assert np.array_equal(ro["buffer_latencies"][b], raw["buffer_latencies"]), (it, b)
                np.testing.assert_allclose(oi[b], oo["obs_inter"], rtol=0, atol=OBS_TOL, err_msg=str((it, b)))
                idle = tabs.ue_slice[cur[b] % tabs.n_scenarios] < 0
                saw_idle_packets |= bool((raw["pkt_incoming"][idle] > 0).any())
            else:
                cur[b], tstep[b] = (cur[b] + 1) % n_ep, 0
                o.set_scenario(tabs, int(cur[b] % tabs.n_scenarios))
                o.reset(se_pool[cur[b] * L])
                np.testing.assert_allclose(oi[b], o.obs()["obs_inter"], rtol=0, atol=OBS_TOL)
    assert saw_idle_packets == idle_traffic
    env.close()


def test_compact_and_full_width_steps_agree_at_full_size(monkeypatch):
    """BASELINE configs[2] for 30 TTIs with compact steps (default) and with RANENV_COMPACT=0: identical state,
    observations and rewards; only the mean SE of UEs outside every slice (read by nobody) is not kept up."""
    need_gpu()
    a = bench_like(4096, False)
    monkeypatch.setenv("RANENV_COMPACT", "0")
    b = bench_like(4096, False)
    monkeypatch.delenv("RANENV_COMPACT")
    a.env.reset(); b.env.reset()
    a.env.set_partitions(3)
    a.env.rollout(30)
    for _ in range(30):
        b.env.step()
    assert_same_state(a.env, b.env, a.tables, "compact / full width", loose=LOOSE_SE_MEAN, outputs=("obs_inter", "obs_intra", "reward"))
    a.env.close(); b.env.close()


@pytest.mark.parametrize("se_mode", ["stream", "gather"])
def test_ranges_with_device_autoreset_equal_whole_batch_steps(se_mode):
    """step_async / step_wait with enable_autoreset: every range restarts its finished envs behind its own step, on its own
    stream (ranenv_autoreset_part).  Same numbers as env.step() with auto-reset (checked against the oracle elsewhere): state,
    observations, terminal observations, rewards and done flags at every TTI, three episodes of 5 TTIs per env, the
    scenario changing at every reset."""
    need_gpu()
    envs = []
    for _ in range(2):
        env, tabs, se_pool, trf, start, dims = short_episode_setup(16, 5, False, se_mode)
        env.reset()
        envs.append(env)
    a, b = envs
    ranges = b.set_ranges(2)
    torch.cuda.synchronize()
    for t in range(16):
        oa, ra, da = a.step()
        for k in range(2):
            with torch.cuda.stream(b.range_stream(k)):
                b.step_async(k)
        for k, (lo, hi) in enumerate(ranges):
            with torch.cuda.stream(b.range_stream(k)):
                ob, rb, db = b.step_wait(k)
                assert torch.equal(oa["obs_inter"][lo:hi], ob["obs_inter"]) and torch.equal(oa["obs_intra"][lo:hi], ob["obs_intra"]), (t, k)
                assert torch.equal(ra[lo:hi], rb) and torch.equal(da[lo:hi], db), (t, k)
                assert torch.equal(a.term_obs_inter[lo:hi], b.term_obs_inter[lo:hi]), (t, k)
                for name, x in a.views().items():
                    if x.shape[0] == a.B and name != "se_mean":
                        assert torch.equal(x[lo:hi], b.views()[name][lo:hi]), (t, k, name)
        if (t + 1) % 5 == 0:
            assert bool(da.all())
    assert a.views()["episode_number"].cpu().tolist() == b.views()["episode_number"].cpu().tolist()
    a.close(); b.close()


@pytest.mark.parametrize("se_mode", ["stream", "gather"])
def test_clearing_resets_then_compact_rollouts_then_full_width_steps_keep_the_window_sums(se_mode):
    """RANENV_F_CLEAR_HISTORY_ON_RESET + compact steps: an auto-reset that clears the window moves an env into a
    scenario where some UE is idle; more than hist_depth compact TTIs follow, then full-width steps (env.step() in the
    streaming mode, or a step with explicit traffic).  The idle UE's catch-up must not give up ring values of the era
    before the clear: win_sent / win_dropped (and everything else) equal those of a handle that never steps compactly."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd._lib import F_CLEAR_HISTORY_ON_RESET
    outs = []
    for compact in (1, 0):
        env, tabs, se_pool, trf, start, (S, U, R, G, Us, n_ep, L) = short_episode_setup(12, 28, False, se_mode,
                                                                                           flags=F_CLEAR_HISTORY_ON_RESET)
        env.set_option("compact", compact)
        assert env.get_option("compact") == compact
        env.reset()
        env.rollout(28)                # a whole episode: every ring slot of every slice member holds values; the auto-reset clears
        env.rollout(23)                # > hist_depth TTIs of the next scenario (idle UEs sit them out when compact)
        snap = []
        for _ in range(3):             # full-width steps: idle UEs catch up here
            env.step()
            torch.cuda.synchronize()
            snap.append({k: x.clone() for k, x in env.views().items() if k != "se_mean"})
        tb = torch.zeros((env.B, U), dtype=torch.float64, device=env.device)
        env.step(traffic_bits=tb)       # explicit traffic: full width in both SE modes
        torch.cuda.synchronize()
        snap.append({k: x.clone() for k, x in env.views().items() if k != "se_mean"})
        outs.append((snap, env.obs_inter.clone(), env.reward.clone()))
        env.close()
    (sa, oa, ra), (sb, ob, rb) = outs
    for i, (x, y) in enumerate(zip(sa, sb)):
        for k in x:
            assert torch.equal(x[k], y[k]), (i, k)
        assert int(x["win_sent"].min()) >= 0 and int(x["win_dropped"].min()) >= 0
    assert torch.equal(oa, ob) and torch.equal(ra, rb)


def test_options_are_set_and_read_back_and_unknown_keys_fail():
    need_gpu()
    from intent_radio_sched_multi_slice_amd._lib import RanEnvError
    a = bench_like(64, False)
    env = a.env
    for key, val in (("compact", 0), ("fuse", 7), ("row_width", 16), ("small_batch", 1), ("fuse_first1", 4), ("persist", 1), ("persist_chunk", 7)):
        env.set_option(key, val)
        assert env.get_option(key) == val, key
    assert env.get_option("fuse_first0") == 0
    # values outside a key's range are clamped / normalised on the way in
    clamped = (("fuse", 100, 64), ("fuse", -1, 0), ("persist", -7, -1), ("persist", 5, 1), ("persist_chunk", 0, 1),
               ("persist_chunk", 5000, 1000), ("persist_grid", -3, 0), ("mix", 9, 2), ("mix", -1, 0), ("tiny_step", 3, 1),
               ("pack", 2, 1), ("compact", 5, 1), ("autoreset_shortcut", 2, 1), ("fuse_first2", -4, 0))
    before = {key: env.get_option(key) for key, _, _ in clamped}
    for key, val, stored in clamped:
        env.set_option(key, val)
        assert env.get_option(key) == stored, (key, val)
    for key, val in before.items():
        env.set_option(key, val)               # (the rollout below steps under the settings of above)
    env.set_option("persist_inject_abort", 0)
    with pytest.raises(RanEnvError):
        env.get_option("persist_inject_abort")  # (settable, not readable)
    with pytest.raises(RanEnvError):
        env.set_option("no_such_knob", 1)
    with pytest.raises(RanEnvError):
        env.set_option("row_width", 8)          # < max(S, Us) = 10
    with pytest.raises(RanEnvError):
        env.get_option("no_such_knob")
    env.reset(); env.rollout(9); torch.cuda.synchronize()      # still steps under the odd settings
    assert int(env.views()["step_number"].min()) == 9
    env.close()


def test_gather_only_ingest_from_power_equals_pool_then_gather():
    """ranenv_bind_se_gather_from_power (channels/quadriga.py:56-76 for a gather-only user): the sidecars straight from QuaDRiGa
    received power are bit for bit those built from the RB-major pool ranenv_se_from_power writes, a handle without any RB-major
    pool resets / steps / rolls out / auto-resets to the same state, and what needs whole rows says so."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd._lib import RanEnvError
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload, quadriga_pool_from_power
    dev = torch.device("cuda", 0)
    n_traces, L, B = 6, 10, 96
    g = torch.Generator(device=dev); g.manual_seed(3)
    envs = []
    for mode in ("pool", "power"):
        wl = make_mult_slice_workload(B, dev, n_scenarios=16, n_traces=n_traces, trace_len=L, max_steps=1000)
        env = wl.env
        if mode == "pool":
            power = torch.rand((n_traces * L, env.R, env.U), generator=g, device=dev, dtype=torch.float64) * 4e-11 + 1e-14
            keep_power = power
            env.bind_se_pool(quadriga_pool_from_power(power, env.R))
            env.set_se_mode("gather")
        else:
            env.bind_se_gather_from_power(keep_power)
        eps = wl.env.episodes
        env.set_episodes(scenario=eps["scenario"], se_base=eps["se_base"], se_len=eps["se_len"], se_offset=eps["se_offset"],
                         trf_base=eps["trf_base"], trf_len=eps["trf_len"], trf_offset=eps["trf_offset"])
        envs.append(wl)
    a, b = envs
    sa, sb = a.env.se_sidecars(), b.env.se_sidecars()
    assert torch.equal(sa["row_mean"], sb["row_mean"]) and torch.equal(sa["ue_major"], sb["ue_major"])
    assert b.env.se_mode == "gather"
    for wl in envs:
        wl.env.reset(); wl.env.rollout(13); wl.env.step(); wl.env.rollout(4)
    torch.cuda.synchronize()
    va, vb = comparable_views(a), comparable_views(b)
    for k in va:
        assert torch.equal(va[k], vb[k]), k
    assert torch.equal(a.env.obs_inter, b.env.obs_inter) and torch.equal(a.env.obs_intra, b.env.obs_intra)
    assert torch.equal(a.env.reward, b.env.reward)
    with pytest.raises(RanEnvError):
        b.env.set_se_mode("stream")                      # no RB-major pool to stream
    with pytest.raises(RanEnvError):
        b.env.step_dense(torch.zeros((B, b.env.U, b.env.R), dtype=torch.uint8, device=dev))
    # explicit tiles still stream (whole rows are given), and binding a pool brings the streaming mode back
    tiles = quadriga_pool_from_power(keep_power[torch.arange(B, device=dev) % keep_power.shape[0]].contiguous(), b.env.R)
    b.env.step(se_tiles=tiles)
    b.env.bind_se_pool(quadriga_pool_from_power(keep_power, b.env.R))
    assert b.env.se_mode in ("stream", "gather")
    a.env.close(); b.env.close()
