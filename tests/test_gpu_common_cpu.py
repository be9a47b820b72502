"""The shared assertions of tests/gpu_common.py without a device: on stub envs (CPU tensors behind the attributes the helpers
read) they pass on equal state and fail on every kind of difference the private copies they replaced would have caught."""
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import gpu_common as gc
from tests.common import OBS_TOL, PKT_COUNTS, REW_TOL, oracle_envs, poisson_traffic_rows
from tests.synth import se_tile


class _StubEnv:
    device = torch.device("cpu")

    def __init__(self, views, outputs, raw=None, actions=None, metrics=None):
        self._views, self._raw, self._actions, self._metrics = views, raw, actions, metrics
        for k, x in outputs.items():
            setattr(self, k, x)

    def views(self):
        return self._views

    def raw_observation(self):
        return self._raw

    def policy_actions(self):
        return self._actions

    def episode_metrics(self):
        return self._metrics


# ---- assert_same_state ---------------------------------------------------------------------------------------------------------------
B, U = 3, 4
TABLES = types.SimpleNamespace(ue_slice=np.array([[0, 0, 1, 1], [0, 1, 1, -1]]))      # UE 3 is outside every slice in scenario 1 only
SCENARIO = [0, 1, 1]
OUT_OF_SLICE = [(1, 3), (2, 3)]
LOOSE_SETS = {"se_mean": gc.LOOSE_SE_MEAN, "win_sent": gc.LOOSE_WIN_SENT, "win_sent_and_se": gc.LOOSE_WIN_SENT_AND_SE,
              "windows_and_se": gc.LOOSE_WINDOWS_AND_SE}
PER_UE = ("queue_pkts", "win_sent", "win_dropped", "se_mean")


def _state():
    g = torch.Generator().manual_seed(1)
    views = {k: torch.randint(1, 9, (B, U), generator=g).to(torch.float64 if k == "se_mean" else torch.int32) for k in PER_UE}
    views["step_number"] = torch.tensor([5, 5, 2], dtype=torch.int32)
    views["episodes"] = torch.tensor([[s, 7] for s in SCENARIO], dtype=torch.int32)
    outputs = dict(obs_inter=torch.rand((B, 20), generator=g), obs_intra=torch.rand((B, 2, 17), generator=g),
                   reward=torch.rand((B, 3), generator=g, dtype=torch.float64), done=torch.zeros(B, dtype=torch.uint8),
                   head_obs=torch.rand((B, 20), generator=g))
    return _StubEnv(views, outputs, actions=dict(scores=torch.rand((B, 2), generator=g, dtype=torch.float64),
                                                 intra=torch.ones((B, 2), dtype=torch.uint8)),
                    metrics=dict(running=torch.rand((B, 8), generator=g, dtype=torch.float64)))


def _bump(x, at):
    x[at] = x[at] + 1


def _differs(loose, change, **kw):
    a, b = _state(), _state()
    change(b)
    with pytest.raises(AssertionError):
        gc.assert_same_state(a, b, TABLES, "stub", loose=loose, **kw)


def test_in_slice_mask_follows_the_scenario_on_the_device():
    assert gc.in_slice_mask(TABLES, _state()).tolist() == [[True] * 4, [True, True, True, False], [True, True, True, False]]


@pytest.mark.parametrize("name", list(LOOSE_SETS))
def test_assert_same_state_is_exact_except_for_loose_keys_outside_every_slice(name):
    loose = LOOSE_SETS[name]
    everything = dict(outputs=gc.OUTPUTS + ("head_obs",), actions=("scores", "intra"), metrics={"episode_metrics": ("running",)})
    gc.assert_same_state(_state(), _state(), TABLES, "equal", loose=loose, **everything)
    for k in PER_UE:
        for at in [(b, u) for b in range(B) for u in range(U)]:
            change = lambda e, k=k, at=at: _bump(e.views()[k], at)
            if k in loose and at in OUT_OF_SLICE:      # stale there by design: the one difference that is let through
                a, b = _state(), _state()
                change(b)
                gc.assert_same_state(a, b, TABLES, (k, at), loose=loose)
            else:
                _differs(loose, change)
    for b in range(B):
        _differs(loose, lambda e, b=b: _bump(e.views()["step_number"], b))
    _differs(loose, lambda e: _bump(e.views()["episodes"], (0, 1)))
    # a key list: the listed keys are compared, loose or strict as above, and the others are not
    keys = ("queue_pkts", "win_sent")
    _differs(loose, lambda e: _bump(e.views()["queue_pkts"], (1, 3)), keys=keys)
    _differs(loose, lambda e: _bump(e.views()["win_sent"], (2, 0)), keys=keys)
    a, b = _state(), _state()
    _bump(b.views()["win_dropped"], (0, 0))
    gc.assert_same_state(a, b, TABLES, "unlisted", loose=loose, keys=keys)
    # whatever else the caller asks for
    for k in gc.OUTPUTS:
        _differs(loose, lambda e, k=k: _bump(getattr(e, k), 1))
    _differs(loose, lambda e: _bump(e.head_obs, (2, 0)), outputs=gc.OUTPUTS + ("head_obs",))
    for k in ("scores", "intra"):
        _differs(loose, lambda e, k=k: _bump(e.policy_actions()[k], (0, 1)), actions=("scores", "intra"))
    _differs(loose, lambda e: _bump(e.episode_metrics()["running"], (1, 7)), metrics={"episode_metrics": ("running",)})


def test_comparable_views_blanks_the_mean_se_outside_every_slice_only():
    wl = types.SimpleNamespace(env=_state(), tables=TABLES)
    v, raw = gc.comparable_views(wl), wl.env.views()
    for k in raw:
        want = raw[k].clone()
        if k == "se_mean":
            for at in OUT_OF_SLICE:
                want[at] = 0
        assert torch.equal(v[k], want), k


# ---- assert_matches_oracle -----------------------------------------------------------------------------------------------------------
def _oracle_pair():
    """The smallest shape of tests/test_gpu_parity.py: two oracle envs stepped twice under the caller's scores."""
    from intent_radio_sched_multi_slice_amd.scenario import generate_scaled_scenarios
    S, U_, R, G, Us = 3, 7, 5, 1, 4
    tabs = generate_scaled_scenarios(3, seed=5, n_slices=S, n_ues=U_, max_ues_slice=Us, min_slices=1, min_ues=1)
    rng = np.random.default_rng(7)
    scen = rng.integers(0, tabs.n_scenarios, 2)
    oenvs = oracle_envs(tabs, scen, (S, U_, R, G, Us), 4)
    trf = [poisson_traffic_rows(tabs, int(sc), rng, 2) for sc in scen]
    counts = None
    for b, o in enumerate(oenvs):
        o.reset(se_tile(90, 0, U_, R))
    for t in range(2):
        sc, ic = rng.uniform(-1, 1, (2, S)), rng.integers(0, 3, (2, S)).astype(np.uint8)
        counts = [o.action_format(sc[b], ic[b], want_dense=False)[1] for b, o in enumerate(oenvs)]
        for b, o in enumerate(oenvs):
            o.step(sc[b], ic[b], se_tile(90, t, U_, R), trf[b][t])
    return oenvs, counts


def _stub_of(oenvs, counts):
    raws, obs = [o.raw() for o in oenvs], [o.obs() for o in oenvs]
    stack = lambda rows, dtype: torch.as_tensor(np.stack([np.asarray(r) for r in rows])).to(dtype)
    views = {k: stack([r[k] for r in raws], torch.int32) for k in PKT_COUNTS}
    views["rb_count"] = stack(counts, torch.int32)
    raw = {k: stack([r[k] for r in raws], torch.float64) for k in ("buffer_occupancies", "buffer_latencies")}
    outputs = dict(obs_inter=stack([o["obs_inter"] for o in obs], torch.float32), obs_intra=stack([o["obs_intra"] for o in obs], torch.float32),
                   reward=stack([o["reward"] for o in obs], torch.float64))
    return _StubEnv(views, outputs, raw=raw)


def test_assert_matches_oracle_passes_on_the_oracles_own_outputs_and_fails_on_each_perturbation():
    oenvs, counts = _oracle_pair()
    assert sum(int(o.raw()["pkt_incoming"].sum()) for o in oenvs) > 0

    def check(change=None, as_dict=False, **kw):
        env = _stub_of(oenvs, counts)
        if change is not None:
            change(env)
        obs = dict(obs_inter=env.obs_inter, obs_intra=env.obs_intra)
        gc.assert_matches_oracle(env, obs, env.reward, dict(enumerate(oenvs)) if as_dict else oenvs, "stub", **kw)
        gc.assert_matches_oracle(env, None, None, oenvs, "stub, the env's own buffers", **kw)

    check()
    check(as_dict=True, rb_count=dict(enumerate(counts)))
    check(rb_count=counts, buffers=False)

    def ulp(x, at):
        x[at] = float(np.nextafter(float(x[at]), np.inf))

    def shift(x, by):
        flat = x.view(-1)
        k = int(flat.abs().argmin())
        flat[k] = flat[k] + by

    perturbations = [lambda e, k=k: _bump(e.views()[k], (1, 2)) for k in PKT_COUNTS]
    perturbations += [lambda e: ulp(e.raw_observation()["buffer_occupancies"], (0, 3)),
                      lambda e: ulp(e.raw_observation()["buffer_latencies"], (1, 0)),
                      lambda e: shift(e.obs_inter, 2 * OBS_TOL), lambda e: shift(e.obs_intra, -2 * OBS_TOL),
                      lambda e: shift(e.reward, 2 * REW_TOL)]
    for change in perturbations:
        with pytest.raises(AssertionError):
            check(change)
    with pytest.raises(AssertionError):
        check(lambda e: _bump(e.views()["rb_count"], (0, 0)), rb_count=counts)
    check(lambda e: ulp(e.raw_observation()["buffer_occupancies"], (0, 3)), buffers=False)      # switched off by the caller: not compared


# ---- select_build --------------------------------------------------------------------------------------------------------------------
KNOBS = ("RANENV_SMALL_BATCH", "RANENV_PACK", "RANENV_MIX", "RANENV_SE_MODE", "RANENV_TINY_STEP")
# what the build fixture of test_gpu_parity.py, _select_build of test_gpu_intent_branches.py and test_gpu_fuzz.py set for the name
BUILD_KNOBS = {
    "lean": ("0", "0", "0", None, "0"),
    "small": ("1", "0", "0", None, "0"),
    "tiny1": ("1", "0", "0", None, "1"),
    "gather": ("1", "0", "0", "gather", None),
    "packed": ("0", "1", "0", None, None),
    "packed-gather": ("0", "1", "0", "gather", None),
    "mixed": ("0", "0", "2", None, None),
    "mixed-gather": ("0", "0", "2", "gather", None),
    "per-element": ("1", "0", "0", None, None),
    "per-element-gather": ("1", "0", "0", "gather", None),
}


@pytest.mark.parametrize("build", list(BUILD_KNOBS))
def test_select_build_sets_the_knobs_each_module_set(build, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    gc.select_build(monkeypatch, build)
    assert tuple(os.environ.get(k) for k in KNOBS) == BUILD_KNOBS[build]


def test_select_build_refuses_an_unknown_name(monkeypatch):
    with pytest.raises(AssertionError):
        gc.select_build(monkeypatch, "packed_gather")


def test_select_build_leaves_the_tiny_step_knob_alone_for_the_other_names(monkeypatch):
    for build in BUILD_KNOBS:
        if build not in ("lean", "small", "tiny1"):
            monkeypatch.setenv("RANENV_TINY_STEP", "7")
            gc.select_build(monkeypatch, build)
            assert os.environ["RANENV_TINY_STEP"] == "7", build


# ---- launches_since / assert_build_ran -----------------------------------------------------------------------------------------------
class _CountingEnv:
    """step_launches() of a handle: all sixteen keys, cumulative."""

    def __init__(self):
        self.n = {k: 0 for b in gc.STEP_BUILDS for k in (b, b + "_many")}

    def launch(self, build, times=1, many=False):
        self.n[build] += times
        if many:
            self.n[build + "_many"] += times

    def step_launches(self):
        return dict(self.n)


def test_launches_since_is_a_snapshot_or_a_delta():
    env = _CountingEnv()
    env.launch("tiny1", 3)
    before = gc.launches_since(env)
    assert len(before) == 16 and before["tiny1"] == 3 and before["lean"] == 0
    env.launch("lean", 2, many=True)
    assert before["lean"] == 0                                   # (a copy: the snapshot does not move)
    d = gc.launches_since(env, before)
    assert d["lean"] == 2 and d["lean_many"] == 2 and d["tiny1"] == 0 and sum(d.values()) == 4


def test_assert_build_ran_passes_on_the_named_build_and_fails_on_every_other_outcome():
    env = _CountingEnv()
    env.launch("tiny1", 5)                                       # (before the snapshot: never counted)
    before = gc.launches_since(env)
    with pytest.raises(AssertionError, match="did not run"):     # nothing launched
        gc.assert_build_ran(env, before, "lean")
    env.launch("lean", 4)
    # pass: by name, with the count, with many=False
    gc.assert_build_ran(env, before, "lean")
    d = gc.assert_build_ran(env, before, "lean", many=False, count=4)
    assert d["lean"] == 4
    # wrong build: the message prints the whole delta
    with pytest.raises(AssertionError, match=r"build lean ran.*'lean': 4"):
        gc.assert_build_ran(env, before, "small")
    # wrong many, either way
    with pytest.raises(AssertionError, match="several TTIs"):
        gc.assert_build_ran(env, before, "lean", many=True)
    env.launch("lean", 1, many=True)
    with pytest.raises(AssertionError, match="several TTIs"):    # 1 of 5: neither all nor none
        gc.assert_build_ran(env, before, "lean", many=True)
    with pytest.raises(AssertionError, match="several TTIs"):
        gc.assert_build_ran(env, before, "lean", many=False)
    gc.assert_build_ran(env, before, "lean", count=5)
    # wrong count
    with pytest.raises(AssertionError, match="launch count"):
        gc.assert_build_ran(env, before, "lean", count=4)
    # two builds: one name fails, the tuple passes and wants both
    env.launch("persist", 2, many=True)
    with pytest.raises(AssertionError, match="build persist ran"):
        gc.assert_build_ran(env, before, "lean")
    gc.assert_build_ran(env, before, ("lean", "persist"), count=7)
    with pytest.raises(AssertionError, match="build gather did not run"):
        gc.assert_build_ran(env, before, ("lean", "persist", "gather"))
    with pytest.raises(AssertionError, match="launch count"):
        gc.assert_build_ran(env, before, ("lean", "persist"), count=5)
    # builds that may run beside the named one: let through, counted, and still not enough on their own
    gc.assert_build_ran(env, before, "lean", also=("persist", "tiny1"), count=7)
    with pytest.raises(AssertionError, match="build small did not run"):
        gc.assert_build_ran(env, before, "small", also=("lean", "persist"))
    # a fresh snapshot starts from here
    after = gc.launches_since(env)
    env.launch("persist", 1, many=True)
    gc.assert_build_ran(env, after, "persist", many=True, count=1)
    with pytest.raises(AssertionError):
        gc.assert_build_ran(env, after, "not-a-build")


# ---- build_for -----------------------------------------------------------------------------------------------------------------------
class _ShapeEnv:
    def __init__(self, S, U, Us, B, **options):
        self.S, self.U, self.Us, self.B = S, U, Us, B
        self.options = dict(dict(compact=1, tiny_step=1, small_batch=0), **options)

    def get_option(self, key):
        return self.options[key]


def test_build_for_names_the_build_where_the_shape_fits_and_the_fallback_where_not():
    ref, wide, grid = _ShapeEnv(5, 25, 5, 8), _ShapeEnv(10, 100, 10, 7), _ShapeEnv(16, 256, 16, 6)
    assert gc.step_shape(ref) == (64, 8) and gc.step_shape(wide) == (128, 10) and gc.step_shape(grid) == (256, 16)
    assert gc.step_shape(_ShapeEnv(9, 25, 5, 8)) == (128, 10)              # (nine slices: two waves of slice-table words)
    # packed waves: row width 8, at most 32 UEs, one wave, an even launch, no env mask
    assert gc.build_for(ref, "packed") == gc.build_for(ref, "packed-gather") == gc.build_for(ref, "packed", many=True, n=4, partitions=2) == "packed"
    assert gc.build_for(ref, "packed", explicit_traffic=True, explicit_se=True) == "packed"
    assert gc.build_for(ref, "packed", n=3, partitions=2) == gc.build_for(ref, "packed", masked=True) == gc.build_for(wide, "packed") == "tiny1"
    assert gc.build_for(_ShapeEnv(5, 25, 5, 7), "packed") == gc.build_for(_ShapeEnv(5, 33, 5, 8), "packed") == "tiny1"
    assert gc.build_for(ref, "packed-gather", masked=True) == "gather" and gc.build_for(wide, "packed", many=True) == "lean"
    # mixed blocks: two waves, the whole batch in one launch, a compact step
    assert gc.build_for(wide, "mixed") == gc.build_for(wide, "mixed-gather", many=True) == "mixed"
    for kw in (dict(n=3, partitions=2), dict(partitions=3), dict(masked=True), dict(explicit_traffic=True)):
        assert gc.build_for(wide, "mixed", **kw) == "tiny1" and gc.build_for(wide, "mixed-gather", **kw) == "gather", kw
    assert gc.build_for(_ShapeEnv(10, 100, 10, 7, compact=0), "mixed") == gc.build_for(ref, "mixed") == gc.build_for(grid, "mixed") == "tiny1"
    assert gc.build_for(wide, "mixed-gather", explicit_traffic=True, explicit_se=True) == "tiny1"
    # the streaming names: what the knobs on the handle select, and the name has to agree with them
    assert gc.build_for(_ShapeEnv(5, 25, 5, 8, tiny_step=0), "lean") == gc.build_for(_ShapeEnv(5, 25, 5, 8, tiny_step=0), "lean", many=True) == "lean"
    assert gc.build_for(_ShapeEnv(5, 25, 5, 8, tiny_step=0, small_batch=1), "small") == "small"
    assert gc.build_for(_ShapeEnv(5, 25, 5, 8, small_batch=1), "tiny1") == "tiny1" and gc.build_for(_ShapeEnv(5, 25, 5, 8, small_batch=1), "tiny1", many=True) == "small"
    for env, name in ((ref, "lean"), (_ShapeEnv(5, 25, 5, 8, tiny_step=0, small_batch=1), "lean"), (_ShapeEnv(5, 25, 5, 8, tiny_step=0), "small"),
                      (_ShapeEnv(5, 25, 5, 8, tiny_step=0), "tiny1")):
        with pytest.raises(AssertionError, match="did not reach the handle"):
            gc.build_for(env, name)
    # the per-element rounding has lean and gather builds only
    assert gc.build_for(ref, "per-element") == gc.build_for(wide, "mixed", per_element=True) == gc.build_for(ref, "packed", per_element=True) == "lean"
    assert gc.build_for(ref, "per-element-gather", many=True) == "gather" and gc.build_for(ref, "per-element-gather", explicit_se=True) == "lean"
    assert gc.build_for(ref, "gather") == "gather" and gc.build_for(ref, "gather", explicit_se=True) == "tiny1"
