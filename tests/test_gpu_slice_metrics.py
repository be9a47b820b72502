"""Per-slice episode metrics on the device (ranenv_enable_slice_metrics, include/ranenv.h "Per-slice episode metrics"):

1. against tests/golden/slice_metrics.npz -- the reference's calc_slice_violations(slice_per_metric=True) and calc_total_throughput
   per TTI on the closed loop of eval_metrics.npz, both window conventions;
2. against the eight per-env sums of the same run;
3. against the CPU oracle on the directed intents (tests/slice_metrics_ref.py; tests/test_slice_metrics_cpu.py holds the conditions
   that keep this from passing vacuously);
4. bit for bit across the launch paths, and nothing else moves when they are switched on;
5. reset, episode ends, slots, evaluate(), switching off;  6. the error paths.

Bars as everywhere: integers exact, float64 drifts within REW_TOL (1e-9) per TTI.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import slice_metrics_ref as smr
from tests.common import REW_TOL, load_golden
from tests.gpu_common import LOOSE_WINDOWS_AND_SE, assert_same_state, device_env_of_run, env_from_eval_fixture, need_gpu

pytestmark = pytest.mark.gpu

INT_COLS = [0, 1, 2, 3, 4, 6, 7, 8, 9]
E_INVALID, E_STATE = -1, -3


# ---- 1 / 2: the reference's evaluation code ------------------------------------------------------------------------------------------
def _msg_sizes(tabs, scen):
    return np.where(tabs.slice_has_req[scen] != 0, tabs.slice_message_size[scen], 0).astype(np.float64)


@pytest.mark.parametrize("window", ["live", "restarted"])
def test_per_tti_shares_equal_the_reference_evaluation_code(window):
    need_gpu()
    from intent_radio_sched_multi_slice_amd._lib import F_CLEAR_HISTORY_ON_RESET
    fx, tabs, env, (S, U, R, steps, n_ep) = env_from_eval_fixture(F_CLEAR_HISTORY_ON_RESET if window == "restarted" else 0)
    sx = load_golden("slice_metrics")
    assert np.array_equal(sx["cfg"], fx["cfg"]) and np.array_equal(sx["scen_ids"], fx["scen_ids"])
    tag = "live_deque" if window == "live" else "restarted_with_reset"
    want_m = sx[f"{tag}_intent_slice_metric"]                                          # [ep, t, S, 3]
    want_thr = [sx[f"{tag}_{n}"] for n in ("total_network_requested_throughput", "total_network_throughput", "total_network_eff_throughput")]
    env.enable_metrics(n_ep)
    env.enable_slice_metrics()
    env.reset()
    sm = env.slice_episode_metrics()
    B = env.B
    prev = np.zeros((B, S, 10))
    for ep in range(n_ep):
        scen = int(fx["scen_ids"][ep])
        active = tabs.slice_active[scen] != 0
        msg = _msg_sizes(tabs, scen)
        for t in range(steps):
            env.step()
            last = t == steps - 1
            now = (sm["episode_log"][:, ep] if last else sm["running"]).cpu().numpy()
            d = now - prev
            prev = np.zeros((B, S, 10)) if last else now
            m = want_m[ep, t]
            dm = np.where(m == -2, 1.0, m)
            exp = np.zeros((S, 6))
            exp[:, 0] = active
            exp[:, 1] = dm.min(axis=1) < 0
            exp[:, 2:5] = dm < 0
            exp[:, 5] = np.minimum(dm.min(axis=1), 0.0)
            assert not (exp[~active] != 0).any()               # (the reference skipped them: rows of -2)
            for b in range(B):
                assert np.array_equal(d[b, :, 0:5], exp[:, 0:5]), (window, ep, t, b, d[b, :, 0:5], exp[:, 0:5])
                np.testing.assert_allclose(d[b, :, 5], exp[:, 5], rtol=0, atol=REW_TOL, err_msg=str((window, ep, t, b)))
                for k, w in zip((6, 7, 8), want_thr):
                    got = float((d[b, :, k] * msg / 1e6).sum())
                    assert abs(got - w[ep, t]) <= 1e-9 * abs(w[ep, t]), (window, ep, t, b, k, got, w[ep, t])
    torch.cuda.synchronize()
    assert sm["episode_scenario"].cpu().numpy().tolist() == [[1, 4, 2]] * B
    assert env.episode_metrics()["episodes_done"].cpu().numpy().tolist() == [n_ep] * B
    env.close()


def test_evaluate_per_slice_is_consistent_with_the_eight_sums():
    """evaluate(per_slice=True) over two partitions: the per-slice columns summed over the slices against the per-env sums of the
    same run, and the result without per_slice is today's dict."""
    need_gpu()
    fx, tabs, env, (S, U, R, steps, n_ep) = env_from_eval_fixture()
    env.enable_metrics(n_ep)
    env.enable_slice_metrics()
    env.set_partitions(2)
    res = env.evaluate(n_ep, per_slice=True)
    sl = res["slice"]
    assert sl.shape == (env.B, n_ep, S, 10) and sl.dtype == np.float64
    assert res["scenario"].dtype == np.int32 and res["scenario"].tolist() == [[1, 4, 2]] * env.B
    assert np.array_equal(sl[:, :, :, 1].sum(axis=2), res["violations"])
    assert np.array_equal(sl[:, :, :, 8].sum(axis=2), res["pkts_sent"])
    assert np.array_equal(sl[:, :, :, 9].sum(axis=2), res["pkts_dropped"])
    np.testing.assert_allclose(sl[:, :, :, 5].sum(axis=2), res["distance"], rtol=0, atol=REW_TOL * steps)
    assert res["violations"].sum() > 0 and res["pkts_dropped"].sum() > 0
    assert (sl[:, :, :, 0].max(axis=2) == steps).all()
    # aggregated by slice type: the reference's own totals over the run (its dicts, rebuilt from the fixture's rows)
    from intent_radio_sched_multi_slice_amd.scenario import slice_type_from_tables, slice_type_report
    st = slice_type_from_tables(tabs)
    assert ((st >= 0) == (tabs.slice_has_req != 0)).all()           # the fixture's scenarios are made of the ten templates
    rep = slice_type_report(sl[0], res["scenario"][0], st, tabs)
    m = load_golden("slice_metrics")["live_deque_intent_slice_metric"]
    dm = np.where(m == -2, 1.0, m)
    assert sum(rep["violations_per_slice_type"].values()) == int((dm.min(axis=3) < 0).sum())
    per_metric = np.zeros(3)
    for d in rep["violations_slice_metric"].values():
        per_metric += [d.get("throughput", 0), d.get("reliability", 0), d.get("latency", 0)]
    assert per_metric.tolist() == (dm < 0).sum(axis=(0, 1, 2)).tolist()
    want = load_golden("slice_metrics")["live_deque_total_network_eff_throughput"].sum()
    assert abs(rep["total_network_eff_throughput"] - want) <= 1e-9 * want
    plain = env.evaluate(n_ep)
    assert sorted(plain) == sorted(env.METRIC_NAMES)
    env.close()


# ---- 3: the oracle on the directed intents -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", smr.DEVICE_CASES)
def test_directed_case_sums_equal_the_oracle(name):
    need_gpu()
    run = smr.run_of(name)
    c = run["case"]
    env = device_env_of_run(run, flags=0)
    env.enable_metrics(0)
    env.enable_slice_metrics()
    env.reset()
    for t in range(c["steps"]):
        sc, icb, _ = run["steps"][t]
        env.step(sc, icb) if c["policy"] == 0 else env.step()
    torch.cuda.synchronize()
    sm = env.slice_episode_metrics()
    assert "episode_log" not in sm
    got, exp = sm["running"].cpu().numpy(), smr.expected_sums(run)
    assert got.shape == exp.shape
    bad = np.argwhere(got[:, :, INT_COLS] != exp[:, :, INT_COLS])
    assert bad.size == 0, (name, "(env, slice, column index)", bad[:5].tolist(), got[tuple(bad[0][:2])], exp[tuple(bad[0][:2])])
    np.testing.assert_allclose(got[:, :, 5], exp[:, :, 5], rtol=0, atol=REW_TOL * c["steps"])
    env.close()


def test_range_intent_tables_stay_refused_with_slice_metrics_on():
    """RANGE_INTENT_CASE is the oracle's alone: the C ABI refuses a table that declares a metric twice (include/ranenv.h), with
    slice metrics on as without, and the handle goes on summing on the tables it had."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd.batched_env import RanEnvError
    run = smr.run_of("ref-overfulfill-0.5")
    env = device_env_of_run(run, flags=0)
    env.enable_metrics(0)
    env.enable_slice_metrics()
    bad = smr.run_of("range-intent")["tables"]
    with pytest.raises(RanEnvError, match="declares metric 0 twice"):
        env.load_scenarios(bad)
    env.reset()
    exp = np.zeros((env.B, env.S, 10))
    for t in range(4):
        env.step()
        for b, pe in enumerate(run["steps"][t][2]):
            exp[b] += smr.tti_share(run["tables"], int(run["scen"][b]), pe[2], pe[1])
    got = env.slice_episode_metrics()["running"].cpu().numpy()
    assert np.array_equal(got[:, :, INT_COLS], exp[:, :, INT_COLS])
    env.close()


# ---- 4: launch paths -----------------------------------------------------------------------------------------------------------------
T_PATH = 24
LENGTHS = (5, 7, 8, 12, 24, 6)


def _mapf_env(B=12, parts=1, se_mode="stream", slice_on=True, slots=6, size=None):
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    size = size or dict(n_slices=5, n_ues=25, n_rbs=135, rbs_per_rbg=5, max_ues_slice=10)
    wl = make_mult_slice_workload(B, torch.device("cuda", 0), policy=_lib.POLICY_MAPF, intra=_lib.INTRA_PF, n_scenarios=8, n_traces=8,
                                  trace_len=32, max_steps=1000, **size)
    env = wl.env
    env.set_se_mode(se_mode)
    eps = env.episodes
    env.set_episode_table(scenario=eps["scenario"], se_base=eps["se_base"], se_len=eps["se_len"], se_offset=eps["se_offset"],
                          trf_base=eps["trf_base"], trf_len=eps["trf_len"], trf_offset=eps["trf_offset"])
    env.set_max_steps(np.asarray(LENGTHS, dtype=np.int32)[np.arange(B) % len(LENGTHS)])
    env.enable_autoreset(0, B, episode_numbers=np.arange(B, dtype=np.int32))
    env.enable_metrics(slots)
    if slice_on:
        env.enable_slice_metrics()
    if parts > 1:
        env.set_partitions(parts)
    env.reset()
    return wl, env


def _snapshot(env, with_slice=True):
    torch.cuda.synchronize()
    out = {"m_" + k: v.clone() for k, v in env.episode_metrics().items()}
    if with_slice:
        out.update({"s_" + k: v.clone() for k, v in env.slice_episode_metrics().items()})
    return out


def _drive(env, path):
    if path == "step":
        for _ in range(T_PATH):
            env.step()
    elif path == "rollout":
        for k in (1, 7, T_PATH - 8):
            env.rollout(k)
    elif path == "ranges":
        ranges = env.set_ranges(2)
        env.reset()
        for _ in range(T_PATH):
            for k in range(len(ranges)):
                env.step_async(k)
            for k in range(len(ranges)):
                env.step_wait(k)
    else:
        raise ValueError(path)


def _assert_same(a, b, what):
    """(not assert_same_state: these are _snapshot dicts of metric sums, of envs that are closed by now)"""
    assert sorted(a) == sorted(b), what
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


def test_sums_are_bit_identical_across_launch_paths():
    need_gpu()
    _, ref = _mapf_env()
    _drive(ref, "step")
    want = _snapshot(ref)
    ref.close()
    done = want["m_episodes_done"].cpu().numpy()
    assert done.min() >= 1 and len(set(done.tolist())) >= 3            # episodes end at different TTIs in different envs
    assert (want["s_episode_scenario"][:, 0] >= 0).all() and want["s_running"].abs().sum() > 0
    for what, kw, path in (("rollout", {}, "rollout"), ("rollout over 2 partitions", dict(parts=2), "rollout"),
                           ("rollout over 3 partitions", dict(parts=3), "rollout"), ("step_async ranges", {}, "ranges"),
                           ("gather step loop", dict(se_mode="gather"), "step"), ("gather rollout", dict(se_mode="gather", parts=2), "rollout")):
        _, env = _mapf_env(**kw)
        _drive(env, path)
        _assert_same(_snapshot(env), want, what)
        env.close()


@pytest.mark.parametrize("path,parts", [("step", 1), ("rollout", 3)])
def test_nothing_else_moves_when_slice_metrics_are_on(path, parts):
    """Observations, reward, done, every view and the eight sums with slice metrics on are those of the same run without them
    (where the rollout then fuses TTIs into one launch and takes persistent launches, and with them on does neither)."""
    need_gpu()
    wl, on = _mapf_env(parts=parts, slice_on=True)
    _, off = _mapf_env(parts=parts, slice_on=False)
    _drive(on, path)
    _drive(off, path)
    assert_same_state(on, off, wl.tables, path, loose=LOOSE_WINDOWS_AND_SE)
    _assert_same(_snapshot(on, False), _snapshot(off, False), path)
    if path == "rollout":
        assert on.get_option("last_rollout_persistent") == 0
    on.close()
    off.close()


def test_collect_adds_what_the_rollout_under_the_same_nets_adds():
    need_gpu()
    from tests import collect_ref as cr
    B, snaps = 24, {}
    for what, parts in (("step", 1), ("rollout", 1), ("collect", 1), ("collect3", 3)):
        _, env, _ = cr.make_env("S5U25", "64x64", B, stochastic=True, autoreset=True, parts=parts, intra_input="mask_obs", trace_len=32)
        env.enable_metrics(6)
        env.enable_slice_metrics()
        env.reset()
        if what == "step":
            for _ in range(T_PATH):
                env.step()
        elif what == "rollout":
            env.rollout(T_PATH)
        else:
            env.collect(T_PATH)
        snaps[what] = _snapshot(env)
        env.close()
    assert snaps["step"]["s_running"].abs().sum() > 0 and (snaps["step"]["m_episodes_done"] > 0).any()
    for what in ("rollout", "collect", "collect3"):
        _assert_same(snaps[what], snaps["step"], what)


def test_collect_head_adds_what_the_rollout_under_the_same_head_net_adds():
    need_gpu()
    from tests import head_policy_ref as hr
    B, snaps = 24, {}
    for what, parts in (("step", 1), ("rollout", 3), ("collect_head", 1), ("collect_head3", 3)):
        _, env, _ = hr.make_env("S5U25", "64x64", "gauss_clip", B, stochastic=True, seed=0x1234, autoreset=True, parts=parts, metrics=6,
                                trace_len=32)
        env.enable_slice_metrics()
        env.reset()
        if what == "step":
            for _ in range(T_PATH):
                env.step()
        elif what == "rollout":
            env.rollout(T_PATH)
        else:
            env.collect_head(T_PATH, reward="twc")
        snaps[what] = _snapshot(env)
        env.close()
    assert snaps["step"]["s_running"].abs().sum() > 0 and (snaps["step"]["m_episodes_done"] > 0).any()
    for what in ("rollout", "collect_head", "collect_head3"):
        _assert_same(snaps[what], snaps["step"], what)


# ---- 5: lifecycle --------------------------------------------------------------------------------------------------------------------
def _plain_env(B=4, max_steps=9, flags=0, **kw):
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    wl = make_mult_slice_workload(B, torch.device("cuda", 0), policy=2, intra=1, n_scenarios=6, n_traces=12, trace_len=10,
                                  n_slices=5, n_ues=25, n_rbs=135, rbs_per_rbg=5, max_ues_slice=10, max_steps=max_steps, flags=flags, **kw)
    return wl, wl.env


def test_a_masked_reset_zeroes_only_the_masked_envs():
    need_gpu()
    _, env = _plain_env(max_steps=100)
    env.enable_metrics(0)
    env.enable_slice_metrics()
    env.reset()
    for _ in range(3):
        env.step()
    before = env.slice_episode_metrics()["running"].clone()
    assert (before[:, :, 0].amax(dim=1) == 3).all()
    env.reset(env_mask=np.array([1, 0, 1, 0], dtype=np.uint8))
    torch.cuda.synchronize()
    after = env.slice_episode_metrics()["running"]
    assert (after[[0, 2]] == 0).all() and torch.equal(after[[1, 3]], before[[1, 3]])
    env.step()
    torch.cuda.synchronize()
    assert after[:, :, 0].amax(dim=1).tolist() == [1, 4, 1, 4]
    env.close()


def test_per_env_episode_lengths_slots_and_overflow():
    """max_steps [9, 5, 7, 9], two slots, 18 TTIs in one rollout: env 1 ends three episodes -- the third is only counted."""
    need_gpu()
    wl, env = _plain_env()
    eps = env.episodes
    env.set_episode_table(scenario=eps["scenario"], se_base=eps["se_base"], se_len=eps["se_len"], se_offset=eps["se_offset"],
                          trf_base=eps["trf_base"], trf_len=eps["trf_len"], trf_offset=eps["trf_offset"])
    env.set_max_steps([9, 5, 7, 9])
    env.enable_autoreset(0, 4, episode_numbers=np.arange(4, dtype=np.int32))
    env.enable_metrics(2)
    env.enable_slice_metrics()
    env.reset()
    env.rollout(18)
    torch.cuda.synchronize()
    m, sm = env.episode_metrics(), env.slice_episode_metrics()
    assert m["episodes_done"].cpu().numpy().tolist() == [2, 3, 2, 2]
    log, run, scn = sm["episode_log"].cpu().numpy(), sm["running"].cpu().numpy(), sm["episode_scenario"].cpu().numpy()
    assert log.shape == (4, 2, 5, 10) and scn.shape == (4, 2)
    assert log[:, :, :, 0].max(axis=2).tolist() == [[9, 9], [5, 5], [7, 7], [9, 9]]
    assert run[:, :, 0].max(axis=1).tolist() == [0, 3, 4, 0]
    # the scenario rows: episode number n is descriptor n of the table (sequential from the env's own number, wrapping at 4)
    table = np.asarray(eps["scenario"])
    assert scn.tolist() == [[int(table[b]), int(table[(b + 1) % 4])] for b in range(4)]
    # active slices of the logged scenario row counted every TTI, the others never
    for b in range(4):
        for n in range(2):
            act = wl.tables.slice_active[scn[b, n]] != 0
            assert (log[b, n, :, 0] == np.where(act, [9, 5, 7, 9][b], 0)).all()
    assert np.array_equal(log[:, :, :, 8].sum(axis=2), m["episode_log"].cpu().numpy()[:, :, 6])
    env.close()


def test_evaluate_twice_and_switching_off():
    need_gpu()
    from intent_radio_sched_multi_slice_amd.batched_env import RanEnvError
    _, env = _plain_env()
    eps = env.episodes
    env.set_episode_table(scenario=eps["scenario"], se_base=eps["se_base"], se_len=eps["se_len"], se_offset=eps["se_offset"],
                          trf_base=eps["trf_base"], trf_len=eps["trf_len"], trf_offset=eps["trf_offset"])
    env.enable_autoreset(0, 4, episode_numbers=np.arange(4, dtype=np.int32))
    env.enable_metrics(2)
    env.enable_slice_metrics()
    first = env.evaluate(2, per_slice=True)
    second = env.evaluate(2, per_slice=True)
    for res in (first, second):                                   # not accumulated: 9 TTIs per episode, both times
        assert (res["slice"][:, :, :, 0].max(axis=2) == 9).all() and (res["ttis"] == 9).all()
        assert (res["scenario"] >= 0).all()
    env.disable_slice_metrics()
    with pytest.raises(RanEnvError, match="enable_slice_metrics"):
        env.evaluate(1, per_slice=True)
    env.enable_slice_metrics()
    # enable_metrics(-1) switches both off: nothing is added any more, and re-enabling needs enable_metrics again
    env.reset()
    env.step()
    torch.cuda.synchronize()
    kept = env.slice_episode_metrics()["running"].clone()
    assert kept[:, :, 0].amax() == 1
    env.disable_metrics()
    for _ in range(3):
        env.step()
    env.rollout(4)
    torch.cuda.synchronize()
    assert torch.equal(env.slice_episode_metrics()["running"], kept)
    with pytest.raises(RanEnvError, match=r"\(-3\)"):
        env.enable_slice_metrics()
    env.enable_metrics(2)
    torch.cuda.synchronize()
    assert torch.equal(env.slice_episode_metrics()["running"], kept)          # still off: enable_metrics alone leaves them alone
    env.enable_slice_metrics()
    torch.cuda.synchronize()
    assert (env.slice_episode_metrics()["running"] == 0).all()
    env.close()


# ---- 6: errors -----------------------------------------------------------------------------------------------------------------------
def test_error_paths_and_rollout_schedule():
    need_gpu()
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.batched_env import RanEnvError
    _, env = _plain_env(B=8, max_steps=1000)
    lib, h = env._lib, env._h
    stream = C.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)
    assert lib.ranenv_enable_slice_metrics(h, 1, stream) == E_STATE                 # no ranenv_enable_metrics first
    with pytest.raises(RanEnvError, match=r"\(-3\)"):
        env.slice_episode_metrics()
    env.enable_metrics(1)
    assert lib.ranenv_enable_slice_metrics(None, 1, stream) == E_INVALID
    env.enable_slice_metrics()
    env.reset()
    p = env._p_out
    assert lib.ranenv_step(h, None, None, None, None, p[0], None, p[2], p[3], stream) == E_INVALID       # NULL dev_obs_intra
    assert lib.ranenv_step(h, None, None, None, None, p[0], p[1], None, p[3], stream) == E_INVALID       # NULL dev_reward
    assert lib.ranenv_rollout(h, 4, p[0], None, p[2], p[3], stream) == E_INVALID
    assert lib.ranenv_step_range(h, 0, 4, None, None, None, None, p[0], None, p[2], p[3], stream) == E_INVALID
    torch.cuda.synchronize()
    assert (env.slice_episode_metrics()["running"] == 0).all()                     # the refused calls enqueued nothing
    # one TTI per launch, no persistent launch -- whatever the options ask for
    env.set_option("persist", 1)
    for parts, n in ((1, 8), (2, 8), (3, 5)):
        env.set_partitions(parts)
        env.rollout(n)
        assert env.get_option("last_rollout_persistent") == 0
        assert env.get_option("last_rollout_launches") == n * parts, (parts, n)
    torch.cuda.synchronize()
    assert env.slice_episode_metrics()["running"][:, :, 0].amax() == 21
    # switched off: the rollout is free to fuse again
    env.disable_slice_metrics()
    env.set_option("persist", 0)
    env.set_partitions(1)
    env.rollout(8)
    assert env.get_option("last_rollout_launches") < 8
    env.close()
    _, raw = _plain_env(flags=_lib.F_NO_RAW_OUTPUT)
    raw.enable_metrics(1)
    assert raw._lib.ranenv_enable_slice_metrics(raw._h, 1, stream) == E_INVALID      # columns 6 and 7 read the raw outputs
    raw.close()
