"""The step kernel and the head kernel against the CPU oracle on the directed intent inputs (tests/directed_intents.py):
every operator on every metric, requirement values where the three outcomes (over-fulfilled, in the band, violated) all
occur, one to three parameters in every metric order, slices with UEs and no requirement, inactive slices with UEs, all
three reward branches, and handles whose overfulfill / norm_* / bandwidth scalars are not the defaults.
tests/test_intent_branches_cpu.py holds the conditions that keep this file from passing vacuously (every category is
populated in the oracle on exactly these inputs) and shows that a kernel with a swapped operator, a compiled-in 0.2 or
40.0, or a wrong band expression would differ from the oracle here by more than the bars.

Bars as everywhere: integers bit-exact, float32 observations within 1e-5, float64 rewards within 1e-9, per TTI.

On top of the 1e-5 bar, every compared observation entry is held to what rounding predicts.  The observations are float32
roundings of float64 values; the device's float64 value d and the oracle's o differ by at most 1e-9 (the reward bar: the
rewards are those very float64 slice values), and rounding to nearest moves each by at most half a float32 ulp, so
    |float32(d) - float32(o)| <= 1e-9 + ulp32(o)
which for |o| >= 2^-6 (ulp32 >= 1.86e-9 > 1e-9) means: the two float32 numbers are equal or neighbours -- an integer ulp
distance of at most 1 (ULP_BOUND).  Below 2^-6 the absolute form is asserted.  test_float32_ulp_summary prints the largest
distance met by the tests that ran before it.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import directed_intents as di
from tests import intent_census as ic
from tests.common import OBS_TOL, PKT_COUNTS, REW_TOL, tti_metrics
from tests.gpu_common import ULP_BOUND, assert_build_ran, build_for, device_env_of_run, launches_since, need_gpu, select_build
from tests.gpu_common import SEEN as _SEEN, check_all as _check_all, check_env as _check_env, check_obs as _check_obs

pytestmark = pytest.mark.gpu


BUILDS = {      # the switches of tests/test_gpu_fuzz.py; the cases at which each build's own path applies
    "lean": tuple(c["name"] for c in di.CASES),
    "small": ("ref-default", "ref-all-scalars", "packable", "partial-wave", "one-slice"),
    "tiny1": ("ref-default", "ref-all-scalars", "packable", "partial-wave", "one-slice"),      # the whole-row build: what "small" ran before it named its own
    "gather": ("ref-all-scalars", "ref-overfulfill-0.5", "partial-wave", "grid-16x16", "no-remainder"),
    "packed": ("packable", "one-slice", "no-remainder"),               # two envs per wave: U <= 32 and S, Us <= 8
    "mixed": ("partial-wave",),                                        # mixed blocks: 64 < U <= 128
}


def _step(run, env, t):
    sc, icb, _ = run["steps"][t]
    return env.step(sc, icb) if run["case"]["policy"] == 0 else env.step()


_RUNS = {}


def _run_of(name, **override):
    """The oracle's replay of a directed case (kept for the module: several tests compare against the same one)."""
    key = (name, tuple(sorted(override.items())))
    if key not in _RUNS:
        _RUNS[key] = ic.replay(dict(di.CASE_BY_NAME[name], **override))
    return _RUNS[key]


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build,name", [(b, n) for b, names in BUILDS.items() for n in names])
def test_directed_case_vs_oracle(build, name, monkeypatch):
    """step() per TTI: the caller's scores and intra choices, or MARR / MAPF with each intra scheduler on the device.  Every launch
    ran the build the case is listed under (the library's launch counters); ("packed", "no-remainder") runs with an even batch of 8,
    since packed waves take an even number of envs."""
    need_gpu()
    select_build(monkeypatch, build)
    run = _run_of(name, B=8) if (build, name) == ("packed", "no-remainder") else _run_of(name)
    env = device_env_of_run(run)
    if build == "mixed":
        env.set_option("compact", 1)             # (mixed blocks are compact steps: whatever knob the suite runs under)
    env.reset()
    before = launches_since(env)
    for t in range(run["case"]["steps"]):
        obs, rew, done = _step(run, env, t)
        _check_all(run, t, env, obs, rew, build)
    assert int(done.sum()) == run["case"]["B"]
    want = build_for(env, build, per_element=run["case"]["per_element"])
    assert want == build, (build, name, want)     # (every listed case fits its build; the per-element case is listed under "lean" only)
    assert_build_ran(env, before, want, many=False, count=run["case"]["steps"])
    env.close()


@pytest.mark.parametrize("policy,intra", [(1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)])
def test_device_policies_with_each_intra_scheduler(policy, intra):
    """MARR and MAPF with round-robin, proportional-fair and max-throughput inside the slices, non-default scalars."""
    need_gpu()
    run = _run_of("ref-all-scalars", policy=policy, intra=intra, B=7, steps=20)
    env = device_env_of_run(run)
    env.reset()
    for t in range(run["case"]["steps"]):
        obs, rew, done = env.step()
        _check_all(run, t, env, obs, rew, (policy, intra))
    env.close()


@pytest.mark.parametrize("hist_depth", [1, 2, 10])
@pytest.mark.parametrize("path", ["step_range", "partitioned_rollout", "persistent_rollout"])
@pytest.mark.parametrize("name", ["ref-overfulfill-0.5", "partial-wave"])
def test_launch_paths(name, path, hist_depth):
    """The same TTIs issued as ranges on their own streams, as rollouts over three partitions and as persistent
    work-queue rollouts, with observation windows 1, 2 and 10 deep (the reliability drift sums the window, the throughput
    drift reads the previous TTI's occupancy)."""
    need_gpu()
    run = _run_of(name, D=hist_depth)
    c = run["case"]
    env = device_env_of_run(run)
    T = c["steps"]
    if path == "step_range":
        ranges = env.set_ranges(2)
        env.reset()
        for t in range(T):
            for k in range(len(ranges)):
                env.step_async(k)
            for k, (lo, hi) in enumerate(ranges):
                obs, rew, done = env.step_wait(k)
                torch.cuda.synchronize()
                g = {n: x.cpu().numpy() for n, x in env.views().items()}
                oi, oa, rw = env.obs_inter.cpu().numpy(), env.obs_intra.cpu().numpy(), env.reward.cpu().numpy()
                for b in range(lo, hi):
                    _check_env(run, t, b, g, oi, oa, rw, run["steps"][t][2][b], path)
    else:
        if path == "persistent_rollout":
            env.set_option("persist", 1); env.set_option("persist_chunk", 3)
        else:
            env.set_option("persist", 0)
        env.set_partitions(3)
        env.reset()
        t = 0
        for k in (1, 6, 2, T - 9):
            obs, rew, done = env.rollout(k)
            torch.cuda.synchronize()
            t += k
            if k > 1:
                assert env.get_option("last_rollout_persistent") == (1 if path == "persistent_rollout" else 0), (path, k)
            _check_all(run, t - 1, env, obs, rew, (path, k))
        assert t == T and env.get_option("persist_errors") == 0
    env.close()


def test_one_pass_through_a_device_autoreset():
    """Episodes of 9 TTIs over the directed scenarios, the next one installed and reset on the device: the 10-TTI window and
    the previous TTI's occupancy restart there (the agent's deque survives a reset and takes one all-zero entry), compared
    per TTI through two episode ends of every env."""
    need_gpu()
    from oracle import pyoracle
    base = _run_of("ref-overfulfill-0.5")
    c, d, tabs = base["case"], base["directed"], base["tables"]
    S, U, R, B, L, n_ep = c["S"], c["U"], c["R"], c["B"], 9, 8
    rng = np.random.default_rng(5)
    se_pool = di.se_tiles(611, n_ep * L, U, R)
    trf = np.concatenate([d.traffic_rows(e % tabs.n_scenarios, rng, L, 1.5) for e in range(n_ep)])
    run = dict(base, se_pool=se_pool, trf=trf, scen=np.arange(B) % tabs.n_scenarios)
    env = device_env_of_run(dict(run, case=dict(c, steps=L)), max_steps=L)
    ep = np.arange(n_ep)
    env.set_episode_table(scenario=ep % tabs.n_scenarios, se_base=ep * L, se_len=L, trf_base=ep * L, trf_len=L)
    start = np.arange(B) % n_ep
    env.enable_autoreset(0, n_ep, episode_numbers=start)
    cfg = pyoracle.make_cfg(S, U, R, c["G"], c["Us"], max_steps=10 ** 6, hist_depth=c["D"], **c["scalars"])
    oenvs, cur = [], start.copy()
    for b in range(B):
        o = pyoracle.OracleEnv(cfg); o.set_scenario(tabs, int(cur[b] % tabs.n_scenarios)); o.reset(se_pool[cur[b] * L]); oenvs.append(o)
    env.reset()
    intra = np.full(S, c["intra"], dtype=np.int32)
    for it in range(2 * L + 4):
        t = it % L
        obs, rew, done = env.step()
        g = {n: x.cpu().numpy() for n, x in env.views().items()}
        oi, oa, rw = obs["obs_inter"].cpu().numpy(), obs["obs_intra"].cpu().numpy(), rew.cpu().numpy()
        ti, ta, dn = env.term_obs_inter.cpu().numpy(), env.term_obs_intra.cpu().numpy(), done.cpu().numpy()
        for b, o in enumerate(oenvs):
            run["scen"][b] = cur[b] % tabs.n_scenarios
            _, count, _ = o.action_format(o.policy_mapf(), intra, want_dense=False)
            o.step(o.policy_mapf(), intra, se_pool[cur[b] * L + t], trf[cur[b] * L + t])
            assert bool(dn[b]) == (t == L - 1), (it, b)
            if t < L - 1:
                _check_env(run, it, b, g, oi, oa, rw, (count, o.raw(), o.obs()), "autoreset")
                continue
            _check_env(run, it, b, None, ti, ta, rw, (count, o.raw(), o.obs()), "terminal observation")
            cur[b] = (cur[b] + 1) % n_ep
            run["scen"][b] = cur[b] % tabs.n_scenarios
            assert int(g["episodes"][b, 0]) == run["scen"][b]
            o.set_scenario(tabs, int(run["scen"][b])); o.reset(se_pool[cur[b] * L])
            ro = o.obs()
            _check_obs("obs_inter", oi[b], ro["obs_inter"], ("first observation of the next episode", it, b), run)
            _check_obs("obs_intra", oa[b], ro["obs_intra"], ("first observation of the next episode", it, b), run)
    env.close()


@pytest.mark.parametrize("hist_depth", [10, 5])
@pytest.mark.parametrize("name", ["ref-all-scalars", "packable"])
def test_alternative_heads_on_the_directed_scenarios(name, hist_depth):
    """ranenv_head_kernel (SchedTWC / SchedColORAN: the drift over the doubled window) against OracleEnv.heads, round-robin
    inside the slices as their action_format does; the bars of tests/test_gpu_flags_and_errors.py's head test."""
    need_gpu()
    case = di.CASE_BY_NAME[name]
    tabs = di.materialise(case)[0].tables
    uc = (np.random.default_rng(3).integers(0, 4, tabs.slice_active.shape) * (tabs.slice_has_req != 0)).astype(np.int32)
    scen = np.arange(case["B"]) % case["n_scen"]
    run = ic.replay(dict(case, D=hist_depth, intra=0), extra=lambda o, b: o.heads(uc[scen[b]]))
    env = device_env_of_run(run)                       # (policy 0 with intra 0: the caller's scores, round-robin)
    env.enable_heads(uc)
    env.reset()
    saw_neg = saw_col = False
    for t in range(case["steps"]):
        assert not run["steps"][t][1].any()
        _step(run, env, t)
        ho, hr = env.head_obs.cpu().numpy(), env.head_reward.cpu().numpy()
        for b, pe in enumerate(run["steps"][t][2]):
            obs, r_twc, r_col = pe[6]
            tag = f"{name} D={hist_depth} TTI {t} env {b}"
            np.testing.assert_allclose(ho[b], obs, rtol=1e-6, atol=OBS_TOL, err_msg=tag)
            np.testing.assert_allclose(hr[b], [r_twc, r_col], rtol=0, atol=REW_TOL, err_msg=tag)
            saw_neg |= r_twc < 0; saw_col |= r_col != 0
    assert saw_neg and saw_col
    env.close()


def test_evaluate_sums_violations_and_distances_of_the_directed_drifts():
    """evaluate(): one episode per env in one rollout; violation counts exact, reward and distance sums within 1e-9 a TTI."""
    need_gpu()
    run = _run_of("ref-overfulfill-0.5")
    c, tabs = run["case"], run["tables"]
    B, T = c["B"], c["steps"]
    assert np.any((tabs.slice_active == 0) & (tabs.slice_has_req != 0) & (tabs.slice_nues > 0))     # an inactive slice with a drift row
    env = device_env_of_run(run)
    env.set_episode_table(scenario=run["scen"], se_base=np.arange(B) * T, se_len=T, trf_base=np.arange(B) * T, trf_len=T)
    env.enable_autoreset(0, B, episode_numbers=np.arange(B))
    env.enable_metrics(1)
    res = env.evaluate(1)
    exp = np.zeros((B, 8))
    for t in range(T):
        for b, pe in enumerate(run["steps"][t][2]):
            sc = int(run["scen"][b])
            exp[b] += tti_metrics(pe[2], pe[1], tabs.slice_active[sc][tabs.sorted_slices[sc]] != 0)
    got = np.stack([res[n][:, 0] for n in env.METRIC_NAMES], axis=1)
    assert np.array_equal(got[:, [0, 2, 3, 6, 7]], exp[:, [0, 2, 3, 6, 7]]), (got, exp)
    np.testing.assert_allclose(got[:, [1, 4, 5]], exp[:, [1, 4, 5]], rtol=0, atol=REW_TOL * T)
    assert exp[:, 2].sum() > 0 and exp[:, 3].sum() > 0 and (exp[:, 3] < exp[:, 2]).any()     # violations, of priority slices and of others
    env.close()


def test_two_parameters_on_one_metric_are_refused():
    """The reference adds one drift term per parameter; the step kernel keeps one (operator, value) per metric.  The C ABI
    therefore refuses a table with a range intent (include/ranenv.h), as set_from_reference refuses the request, and the
    handle goes on with the tables it had."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd.batched_env import RanEnvError
    run = _run_of("ref-overfulfill-0.5")
    env = device_env_of_run(run)
    bad = di.materialise(di.RANGE_INTENT_CASE)[0].tables
    assert (bad.n_scenarios, bad.n_slices, bad.n_ues) == (run["tables"].n_scenarios, env.S, env.U)
    with pytest.raises(RanEnvError, match="declares metric 0 twice"):
        env.load_scenarios(bad)
    env.reset()
    for t in range(4):
        obs, rew, done = env.step()
        _check_all(run, t, env, obs, rew, "after the refusal")
    env.close()


def test_float32_ulp_summary():
    """Largest distance between a device observation and the float32 rounding of the oracle's value, over every entry the
    tests above compared (runs last in this file; with -s it prints the figures)."""
    need_gpu()
    print(f"\ncompared (env, TTI) pairs: {_SEEN['pairs']}; observation entries: {_SEEN['entries']}; largest float32 ulp distance "
          f"(|oracle| >= 2^-6): {_SEEN['ulp']}; largest |device - float32(oracle)| below 2^-6: {_SEEN['abs_small']:.3e}")
    assert _SEEN["ulp"] <= ULP_BOUND
