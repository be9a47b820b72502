"""Helpers shared by the GPU test modules: everything that needs torch or a device.  The numpy-only parts (tolerances, rb_major,
oracle_envs, tti_metrics) are in tests/common.py.  tests/test_gpu_common_cpu.py drives the assertions here with stub envs."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.common import OBS_TOL, PKT_COUNTS, REW_TOL, load_golden, poisson_traffic_rows, rb_major, tables_from
from tests.synth import se_tile


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def to_host(d):
    """A dict of device tensors as numpy copies, behind a synchronize."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in d.items()}


# ----------------------------------------------------------------------------------------------------------------------
# two envs hold the same state
# ----------------------------------------------------------------------------------------------------------------------
# Per-UE fields that two launch paths may leave different for a UE outside every slice of the scenario its env plays (after a
# reset into another scenario, or from the start).  No observation reads them there, and a compact step (include/ranenv.h) does
# not keep them up, so envs that reach the same TTI by different launches may differ there and only there; at UEs in a slice
# they are compared exactly like every other field.  Each comparison names the set it was written with.  They are not merged:
# widening one weakens a test, narrowing one is a claim about the kernel.
# -- one schedule against another of the same policy path (fused / persistent / partitioned rollouts, step loops, the two SE
#    modes): compact steps do not keep the mean SE up.
LOOSE_SE_MEAN = ("se_mean",)
# -- rollout() against a step() loop under a policy network, over an explicit key list that holds neither se_mean nor
#    win_dropped: the sent-packets window after a reset into another scenario.
LOOSE_WIN_SENT = ("win_sent",)
# -- collect() against rollout() under the same nets, over every view: the sent-packets window and the mean SE.
LOOSE_WIN_SENT_AND_SE = ("win_sent", "se_mean")
# -- a head-policy rollout / collect_head / collect_replay, or a run with slice metrics on, against a step loop: these choose
#    compact steps differently, so both windows and the mean SE.
LOOSE_WINDOWS_AND_SE = ("win_sent", "win_dropped", "se_mean")

OUTPUTS = ("obs_inter", "obs_intra", "reward", "done")
HEAD_OUTPUTS = ("head_obs", "head_reward")


def in_slice_mask(tables, env):
    """bool [B, U]: UE u is in a slice of the scenario env b plays now -- read off the device, because auto-reset may have moved on."""
    scen = env.views()["episodes"][:, 0].to(torch.int64)
    return torch.as_tensor(tables.ue_slice >= 0, device=env.device)[scen]


def assert_same_state(a, b, tables, what, *, loose, keys=None, outputs=OUTPUTS, actions=(), metrics=None):
    """Envs ``a`` and ``b`` hold the same state, bit for bit: every view (or those in ``keys``), a key in ``loose`` at the UEs in a
    slice only (``tables`` may be None where ``loose`` is empty); then the output buffers named in ``outputs``, the entries of
    policy_actions() named in ``actions`` and, per getter in ``metrics`` ({"episode_metrics": ("running", ...)}), its entries."""
    if torch.device(a.device).type == "cuda":
        torch.cuda.synchronize()
    va, vb = a.views(), b.views()
    in_slice = in_slice_mask(tables, a) if loose else None
    for k in (va if keys is None else keys):
        x, y = (va[k][in_slice], vb[k][in_slice]) if k in loose else (va[k], vb[k])
        assert torch.equal(x, y), (what, k)
    for k in outputs:
        assert torch.equal(getattr(a, k), getattr(b, k)), (what, k)
    if actions:
        pa, pb = a.policy_actions(), b.policy_actions()
        for k in actions:
            assert torch.equal(pa[k], pb[k]), (what, "policy_actions", k)
    for getter, names in (metrics or {}).items():
        ma, mb = getattr(a, getter)(), getattr(b, getter)()
        for k in names:
            assert torch.equal(ma[k], mb[k]), (what, getter, k)


def comparable_views(wl):
    """env.views() of a Workload, cloned, with the mean SE of UEs outside every slice blanked (LOOSE_SE_MEAN)."""
    env = wl.env
    v = {k: x.clone() for k, x in env.views().items()}
    v["se_mean"] = torch.where(in_slice_mask(wl.tables, env), v["se_mean"], torch.zeros_like(v["se_mean"]))
    return v


# ----------------------------------------------------------------------------------------------------------------------
# the device against mirrored oracle envs
# ----------------------------------------------------------------------------------------------------------------------
def assert_matches_oracle(env, obs, rew, oenvs, tag, *, buffers=True, rb_count=None):
    """The device after a TTI against the oracle envs that mirror it (a list: env b is oenvs[b]; or {b: oracle env} for a
    sample): the four raw packet counts exactly, buffer_occupancies and buffer_latencies exactly (``buffers``), obs_inter and
    obs_intra within OBS_TOL, the rewards within REW_TOL.  ``obs`` / ``rew``: what the launch returned, or None for the env's own
    output buffers.  ``rb_count``: the allocation the oracle expects per mirrored env (indexed like ``oenvs``), compared exactly."""
    v = env.views()
    g = {k: v[k].cpu().numpy() for k in PKT_COUNTS + (("rb_count",) if rb_count is not None else ())}
    ro = {k: x.cpu().numpy() for k, x in env.raw_observation().items()} if buffers else None
    goi = (env.obs_inter if obs is None else obs["obs_inter"]).cpu().numpy()
    goa = (env.obs_intra if obs is None else obs["obs_intra"]).cpu().numpy()
    grw = (env.reward if rew is None else rew).cpu().numpy()
    for b, o in (oenvs.items() if isinstance(oenvs, dict) else enumerate(oenvs)):
        raw, oo = o.raw(), o.obs()
        if rb_count is not None:
            assert np.array_equal(g["rb_count"][b], rb_count[b]), (tag, b, "rb_count")
        for name in PKT_COUNTS:
            assert np.array_equal(g[name][b].astype(np.float64), raw[name]), (tag, b, name)
        if buffers:
            assert np.array_equal(ro["buffer_occupancies"][b], raw["buffer_occupancies"]), (tag, b, "buffer_occupancies")
            assert np.array_equal(ro["buffer_latencies"][b], raw["buffer_latencies"]), (tag, b, "buffer_latencies")
        for name, got in (("obs_inter", goi), ("obs_intra", goa)):
            want = np.asarray(oo[name])
            assert got[b].size == want.size, (tag, b, name)
            np.testing.assert_allclose(got[b].ravel(), want.ravel(), rtol=0, atol=OBS_TOL, err_msg=str((tag, b, name)))
        np.testing.assert_allclose(grw[b], oo["reward"], rtol=0, atol=REW_TOL, err_msg=str((tag, b)))


def select_build(monkeypatch, build):
    """The one place that maps a step-kernel build name to the knobs ranenv_create / bind_se_pool read.
    "lean" / "small": the streaming step kernel's two builds (96 VGPRs / 8 SE loads in flight for batches that fill the CUs, 128 /
    32 for small ones), forced because test batches are small -- and RANENV_TINY_STEP=0, or a one-TTI step of a test batch would run
    the whole-row build instead.  "tiny1": that whole-row build (RANENV_TINY_STEP=1 over the small build: one-TTI steps of a batch
    within 2 waves per SIMD).  "packed*": option pack on -- envs of at most 32 UEs and 8 slices two per wave where a launch covers an
    even number of them.  "mixed*": whole-batch steps as mixed blocks, forced for small batches (RANENV_MIX=2).  "per-element*": the
    small build; the caller creates the handle with F_SCALE_PER_ELEMENT.  "*gather": the SE gather mode, switched on at bind; the
    other names leave RANENV_SE_MODE, and all but "lean" / "small" / "tiny1" leave RANENV_TINY_STEP, as they find them."""
    known = ("lean", "small", "tiny1", "gather", "packed", "packed-gather", "mixed", "mixed-gather", "per-element", "per-element-gather")
    assert build in known, build
    monkeypatch.setenv("RANENV_SMALL_BATCH", "0" if build == "lean" or build.startswith(("packed", "mixed")) else "1")
    monkeypatch.setenv("RANENV_PACK", "1" if build.startswith("packed") else "0")
    monkeypatch.setenv("RANENV_MIX", "2" if build.startswith("mixed") else "0")
    if build in ("lean", "small"):
        monkeypatch.setenv("RANENV_TINY_STEP", "0")
    elif build == "tiny1":
        monkeypatch.setenv("RANENV_TINY_STEP", "1")
    if build.endswith("gather"):
        monkeypatch.setenv("RANENV_SE_MODE", "gather")


# ----------------------------------------------------------------------------------------------------------------------
# the device against an oracle replay of a directed case (tests/intent_census.py: replay), per TTI: integers exact, OBS_TOL,
# REW_TOL and -- on top -- every observation entry within what rounding predicts.  The observations are float32 roundings of
# float64 values; the device's float64 value d and the oracle's o differ by at most 1e-9 (the reward bar), and rounding to
# nearest moves each by at most half a float32 ulp, so for |o| >= 2^-6 the two float32 numbers are equal or neighbours
# (ULP_BOUND); below 2^-6 the absolute form |float32(d) - float32(o)| <= 1e-9 + ulp32(o) is asserted.
# ----------------------------------------------------------------------------------------------------------------------
ULP_BOUND = 1
SEEN = {"ulp": 0, "entries": 0, "pairs": 0, "abs_small": 0.0}      # the largest distances met so far (test_float32_ulp_summary)


def _ordered(x32):
    """float32 -> int64 that counts representable numbers: neighbours differ by 1, -0.0 and +0.0 coincide."""
    i = x32.view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _where(name, idx, run):
    """(slice position or slice, column) of a flat observation index: columns 0-2 are the metrics' slice drifts."""
    c = run["case"]
    w = 10 if name == "obs_inter" else 2 * c["Us"] + 9
    return {"row": int(idx) // w, "column": int(idx) % w}


def check_obs(name, got, exp64, tag, run):
    got = np.asarray(got, dtype=np.float32).ravel()
    exp64 = np.asarray(exp64, dtype=np.float64).ravel()
    err = np.abs(got.astype(np.float64) - exp64)
    if not (err <= OBS_TOL).all():          # (NaN fails too)
        k = int(np.argmax(np.where(np.isnan(err), np.inf, err)))
        raise AssertionError(f"{name} differs by {err[k]:.3e} at {tag} {_where(name, k, run)}: device {got[k]!r}, oracle {exp64[k]!r}")
    exp32 = exp64.astype(np.float32)
    ulp = np.abs(_ordered(got) - _ordered(exp32))
    big = np.abs(exp64) >= 2.0 ** -6
    SEEN["entries"] += got.size
    if big.any():
        SEEN["ulp"] = max(SEEN["ulp"], int(ulp[big].max()))
    if (~big).any():
        SEEN["abs_small"] = max(SEEN["abs_small"], float(np.abs(got.astype(np.float64) - exp32.astype(np.float64))[~big].max()))
    bound = np.where(big, 0.0, 1e-9) + np.spacing(np.maximum(np.abs(exp32), np.float32(2.0 ** -126))).astype(np.float64)
    bad = np.where(big, ulp > ULP_BOUND, np.abs(got.astype(np.float64) - exp32.astype(np.float64)) > bound)
    if bad.any():
        k = int(np.argmax(bad))
        raise AssertionError(f"{name} is {ulp[k]} float32 ulps from the rounded oracle value at {tag} {_where(name, k, run)}: "
                             f"device {got[k]!r}, oracle {exp64[k]!r}")


def check_env(run, t, b, g, obs_inter, obs_intra, rew, expected, what=""):
    """One (env, TTI) pair: allocation and packet counts bit-exact, observations and rewards within the bars."""
    count, raw, oo = expected[0], expected[1], expected[2]
    tag = (run["case"]["name"], what, "TTI", t, "env", b, "scenario", int(run["scen"][b]))
    if g is not None:
        assert np.array_equal(g["rb_count"][b], count), (tag, "rb_count")
        for name in PKT_COUNTS:
            assert np.array_equal(g[name][b].astype(np.float64), raw[name]), (tag, name)
    check_obs("obs_inter", obs_inter[b], oo["obs_inter"], tag, run)
    check_obs("obs_intra", obs_intra[b], oo["obs_intra"], tag, run)
    err = np.abs(rew[b] - oo["reward"])
    if not (err <= REW_TOL).all():
        k = int(np.argmax(np.where(np.isnan(err), np.inf, err)))
        raise AssertionError(f"reward[{k}] ({'inter-slice' if k == 0 else f'slice {k - 1}'}) differs by {err[k]:.3e} at {tag}: "
                             f"device {rew[b][k]!r}, oracle {oo['reward'][k]!r}")
    SEEN["pairs"] += 1


def check_all(run, t, env, obs, rew, what=""):
    g = {n: x.cpu().numpy() for n, x in env.views().items()}
    oi, oa, rw = obs["obs_inter"].cpu().numpy(), obs["obs_intra"].cpu().numpy(), rew.cpu().numpy()
    for b, expected in enumerate(run["steps"][t][2]):
        check_env(run, t, b, g, oi, oa, rw, expected, what)


# ----------------------------------------------------------------------------------------------------------------------
# which build of the step kernel ran (BatchedRanEnv.step_launches: the library's own count of its step launches)
# ----------------------------------------------------------------------------------------------------------------------
STEP_BUILDS = ("lean", "small", "gather", "tiny1", "mixed", "packed", "persist", "persist_tiny")


def launches_since(env, before=None):
    """env.step_launches() now (a snapshot), or -- with an earlier snapshot -- what was launched since."""
    now = dict(env.step_launches())
    if before is None:
        return now
    return {k: v - before.get(k, 0) for k, v in now.items()}


def assert_build_ran(env, before, build, *, many=None, count=None, also=()):
    """Since the snapshot ``before`` the env's step launches ran ``build`` (a name of STEP_BUILDS, or a tuple of names for a run
    that legitimately uses several: each of them must have run) and no other build.  ``count``: the launches of the named builds
    together, exactly (None: at least one each).  ``many``: True -- every one of them a launch of several TTIs, False -- none.
    ``also``: builds that may have run beside them (a schedule the test does not pin down launch by launch); they count towards
    ``count``.  A failure prints the whole delta."""
    delta = launches_since(env, before)
    names = (build,) if isinstance(build, str) else tuple(build)
    also = tuple(b for b in also if b not in names)
    assert names and all(b in STEP_BUILDS for b in names + also), (names, also)
    what = f"expected {' + '.join(names)}" + (f" (possibly {' / '.join(also)})" if also else "") + ("" if many is None else f" (many={many})") + \
           ("" if count is None else f" x {count}") + \
           f"; launched since the snapshot: { {k: v for k, v in delta.items() if v} or 'nothing' } (all: {delta})"
    for b in STEP_BUILDS:
        if b not in names + also:
            assert delta[b] == 0 and delta[b + "_many"] == 0, f"build {b} ran; {what}"
    for b in names:
        assert delta[b] > 0, f"build {b} did not run; {what}"
        if many is not None:
            assert delta[b + "_many"] == (delta[b] if many else 0), f"build {b}: launches of several TTIs; {what}"
    if count is not None:
        assert sum(delta[b] for b in names + also) == count, f"launch count; {what}"
    return delta


def step_shape(env):
    """(threads per env, row width) of the handle's step kernel: whole waves of one lane per UE and per slice-table word; max(S, Us)
    rounded up to 8, 10 or 16 (ranenv_create)."""
    nt = max(-(-env.U // 64), -(-(env.S * 8) // 64)) * 64
    m = max(env.S, env.Us)
    return nt, (8 if m <= 8 else (10 if m <= 10 else 16))


def build_for(env, name, *, many=False, n=None, partitions=1, masked=False, explicit_traffic=False, explicit_se=False, per_element=False):
    """The build a step launch of a test under the select_build name ``name`` has to run (a key of step_launches()): the named
    build wherever the shape and the call meet the conditions the library states for it (include/ranenv.h, options "pack" / "mix" /
    "tiny_step" / "small_batch"), else the build such a launch falls back to, by the knobs read back from the handle.  ``n`` envs of
    the launch (None: the whole batch), of a batch cut into ``partitions``; ``masked``: under an env mask; ``explicit_traffic`` /
    ``explicit_se``: the call hands traffic / SE tiles over (full width; the streaming kernel).  For test batches, which all stay
    within 2 waves per SIMD on any chip of 16 CUs or more."""
    nt, width = step_shape(env)
    n = env.B if n is None else n
    gather = name.endswith("gather") and not explicit_se
    if per_element or name.startswith("per-element"):
        return "gather" if gather else "lean"
    if name.startswith("mixed") and nt == 128 and n == env.B and partitions == 1 and not masked and not explicit_traffic and \
            env.get_option("compact") == 1:
        return "mixed"
    if name.startswith("packed") and width == 8 and env.U <= 32 and nt == 64 and n % 2 == 0 and not masked:
        return "packed"
    if gather:
        return "gather"
    if not many and env.get_option("tiny_step") == 1:
        got = "tiny1"
    else:
        got = "small" if env.get_option("small_batch") == 1 else "lean"
    if name in ("lean", "small") or (name == "tiny1" and not many):
        assert got == name, (name, got, "the knobs of select_build did not reach the handle")
    return got


# ----------------------------------------------------------------------------------------------------------------------
# workloads and fixtures
# ----------------------------------------------------------------------------------------------------------------------
def small_workload(B, steps, **kw):
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    return make_mult_slice_workload(B, torch.device("cuda", 0), policy=2, intra=1, n_scenarios=6, n_traces=12, trace_len=10,
                                    n_slices=5, n_ues=25, n_rbs=135, rbs_per_rbg=5, max_ues_slice=10, max_steps=steps, **kw)


def bench_like(B, gather, seed=10, n_traces=16, trace_len=24, steps=1000):
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    wl = make_mult_slice_workload(B, torch.device("cuda", 0), n_scenarios=32, n_traces=n_traces, trace_len=trace_len,
                                  seed=seed, max_steps=steps)
    wl.env.set_se_mode("gather" if gather else "stream")      # (explicit: the RANENV_SE_MODE knob may have switched it at bind)
    return wl


def shaped_workload(S, Us, B, max_steps=1000, seed=10, U=None, R=25, G=1, trace_len=32):
    """An env whose scenarios 0..3 have every slice active (every sorted position unmasked) and 4..7 from 1 to S slices; env b
    plays scenario b % 8, so env 0 always has them all."""
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.scenario import generate_scaled_scenarios
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    U = min(S * Us, 256) if U is None else U
    wl = make_mult_slice_workload(B, torch.device("cuda", 0), policy=_lib.POLICY_MAPF, intra=_lib.INTRA_PF, n_scenarios=8,
                                  n_traces=8, trace_len=trace_len, seed=seed, n_slices=S, n_ues=U, n_rbs=R, rbs_per_rbg=G,
                                  max_ues_slice=Us, max_steps=max_steps, min_slices=1, min_ues=1)
    full = generate_scaled_scenarios(4, seed=seed + 1, n_slices=S, n_ues=U, max_ues_slice=Us, min_slices=S, min_ues=1)
    for f in dataclasses.fields(full):
        getattr(wl.tables, f.name)[:4] = getattr(full, f.name)
    env = wl.env
    env.load_scenarios(wl.tables)
    eps = env.episodes
    scen = np.arange(B) % 8
    env.set_episodes(scenario=scen, se_base=eps["se_base"], se_len=eps["se_len"], se_offset=eps["se_offset"],
                     trf_base=scen * trace_len, trf_len=trace_len, trf_offset=eps["trf_offset"])
    wl.scenario = scen
    return wl


def short_episode_setup(B, steps, idle_traffic, se_mode="stream", flags=0):
    """B envs over a table of 6 episodes that alternate between scenarios (a UE idle in one episode is in a slice in the
    next), `steps` TTIs per episode, auto-reset on the device, MAPF + PF."""
    from intent_radio_sched_multi_slice_amd.batched_env import BatchedRanEnv
    from intent_radio_sched_multi_slice_amd.scenario import generate_scaled_scenarios
    S, U, R, G, Us = 5, 25, 135, 5, 5
    tabs = generate_scaled_scenarios(6, seed=3, n_slices=S, n_ues=U, max_ues_slice=Us, min_slices=3, min_ues=2)
    rng = np.random.default_rng(23)
    n_ep, L = 6, steps
    se_pool = np.stack([se_tile(81 + ep, t, U, R) for ep in range(n_ep) for t in range(L)])
    trf = np.concatenate([poisson_traffic_rows(tabs, ep % tabs.n_scenarios, rng, L) for ep in range(n_ep)])
    if idle_traffic:                       # bits for every UE, in a slice or not
        trf = trf + rng.poisson(3, trf.shape) * 1e6
    env = BatchedRanEnv(batch=B, n_slices=S, n_ues=U, n_rbs=R, rbs_per_rbg=G, max_ues_slice=Us, n_scenarios=tabs.n_scenarios,
                        max_steps=steps, flags=flags)
    env.load_scenarios(tabs)
    env.bind_se_pool(torch.as_tensor(rb_major(se_pool), device=env.device))
    env.bind_traffic_pool(torch.as_tensor(trf.astype(np.int32), device=env.device))
    ep = np.arange(n_ep)
    env.set_episode_table(scenario=ep % tabs.n_scenarios, se_base=ep * L, se_len=L, trf_base=ep * L, trf_len=L)
    env.set_policy(2, 1)
    if se_mode == "gather":
        env.set_se_mode("gather")
    start = np.arange(B) % n_ep
    env.enable_autoreset(0, n_ep, episode_numbers=start)
    return env, tabs, se_pool, trf, start, (S, U, R, G, Us, n_ep, L)


def env_from_eval_fixture(flags=0, B=2):
    """tests/golden/eval_metrics.npz's closed loop on the device: B envs that all start at episode 0 of its table, MAPF + PF."""
    from intent_radio_sched_multi_slice_amd.batched_env import BatchedRanEnv
    fx = load_golden("eval_metrics")
    S, U, R, G, Us, seed, steps, n_ep = (int(x) for x in fx["cfg"])
    tabs = tables_from(fx)
    env = BatchedRanEnv(batch=B, n_slices=S, n_ues=U, n_rbs=R, rbs_per_rbg=G, max_ues_slice=Us, n_scenarios=tabs.n_scenarios,
                        max_steps=steps, flags=flags)
    env.load_scenarios(tabs)
    se = np.stack([rb_major(se_tile(seed + ep, t, U, R)) for ep in range(n_ep) for t in range(steps)])
    env.bind_se_pool(torch.as_tensor(se, device=env.device))
    env.bind_traffic_pool(torch.as_tensor(fx["traffic"].reshape(n_ep * steps, U).astype(np.int32), device=env.device))
    ep = np.arange(n_ep)
    env.set_episode_table(scenario=fx["scen_ids"], se_base=ep * steps, se_len=steps, trf_base=ep * steps, trf_len=steps)
    env.set_policy(2, 1)                                   # MAPF + PF on the device
    env.enable_autoreset(0, n_ep, episode_numbers=np.zeros(B, dtype=np.int32))
    return fx, tabs, env, (S, U, R, steps, n_ep)


def device_env_of_run(run, max_steps=None, flags=None, batch=None):
    """The device env of an oracle replay of a directed case (tests/intent_census.py: replay); ``flags`` None: from the case's
    ``per_element``.  ``batch``: more envs than the case's B -- env j then plays what env j % B plays (the same scenario, tiles and
    traffic rows), so that the first B envs are the replay's and every other env a copy of one of them."""
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.batched_env import BatchedRanEnv
    c, tabs = run["case"], run["tables"]
    T, B = c["steps"], c["B"]
    if flags is None:
        flags = _lib.F_SCALE_PER_ELEMENT if c["per_element"] else 0
    n = B if batch is None else batch
    env = BatchedRanEnv(batch=n, n_slices=c["S"], n_ues=c["U"], n_rbs=c["R"], rbs_per_rbg=c["G"], max_ues_slice=c["Us"],
                        n_scenarios=tabs.n_scenarios, max_steps=T if max_steps is None else max_steps, hist_depth=c["D"],
                        flags=flags, **c["scalars"])
    env.load_scenarios(tabs)
    env.bind_se_pool(torch.as_tensor(rb_major(run["se_pool"]), device=env.device))
    env.bind_traffic_pool(torch.as_tensor(run["trf"].astype(np.int32), device=env.device))
    src = np.arange(n) % B
    env.set_episodes(scenario=np.asarray(run["scen"])[src], se_base=src * T, se_len=T, trf_base=src * T, trf_len=T)
    env.set_policy(c["policy"], c["intra"])
    return env


# ----------------------------------------------------------------------------------------------------------------------
# policy nets of the width / depth grid (tests/test_policy_ref_cpu.py and tests/test_gpu_policy_network_shapes.py)
# ----------------------------------------------------------------------------------------------------------------------
# (S, Us, B, inter hidden widths, inter activation, intra hidden widths, intra activation, intra layout, stochastic)
GRID = [
    (10, 10, 33, [7], "relu", [1], "tanh", "obs", False),
    (5, 10, 100, [512, 1, 512], "tanh", [33, 512, 96, 7], "relu", "mask_obs", True),
    (1, 1, 1, [32], "tanh", [96], "tanh", "obs", True),
    (16, 16, 31, [160, 480], "relu", [511], "relu", "mask_obs", False),
    (13, 5, 100, [100, 255, 64], "tanh", [480, 160], "tanh", "obs", True),
    (10, 10, 100, [511], "relu", [7, 33], "relu", "obs", True),
    (5, 10, 31, [256, 256], "tanh", [64, 64, 64, 64], "tanh", "mask_obs", False),
    (16, 16, 33, [33], "tanh", [100, 1], "relu", "obs", True),
    (13, 5, 1, [96, 96, 96], "relu", [255], "tanh", "mask_obs", True),
    (1, 1, 100, [480], "tanh", [32, 160], "relu", "mask_obs", False),
    (10, 10, 31, [512, 512], "tanh", [1, 512, 1], "relu", "obs", False),
    (5, 10, 33, [64, 7, 255, 33], "tanh", [1], "relu", "obs", True),
]


def make_net(dims, act, seed, gain=1.0):
    """A torch.nn.Sequential MLP with uniform(+-gain / sqrt(fan_in)) weights and biases."""
    g = torch.Generator().manual_seed(seed)
    mods = []
    for i in range(len(dims) - 1):
        lin = torch.nn.Linear(dims[i], dims[i + 1])
        with torch.no_grad():
            bound = gain / np.sqrt(dims[i])
            lin.weight.copy_((torch.rand(lin.weight.shape, generator=g) * 2 - 1) * bound)
            lin.bias.copy_((torch.rand(lin.bias.shape, generator=g) * 2 - 1) * bound)
        mods.append(lin)
        if i < len(dims) - 2:
            mods.append(torch.nn.Tanh() if act == "tanh" else torch.nn.ReLU())
    return torch.nn.Sequential(*mods)


def make_inter_net(S, widths, act, seed):
    """An inter-slice net whose log_std outputs sit around -1, as a trained policy's do (std well below 1, so that the
    noise moves the scores without clamping most of them)."""
    net = make_net([10 * S] + list(widths) + [2 * S], act, seed)
    with torch.no_grad():
        net[-1].bias[S:] -= 1.0
    return net
