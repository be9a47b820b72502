"""Every build of the step kernel against the CPU oracle, with the library's own launch counters saying that the named build --
and no other -- ran.

The step kernel exists in eight builds (StepBuild, csrc/ranenv_internal.h), each per row width (8, 10, 16), most of them for one
TTI per launch and for several (MANY), several for both SE modes, two for the per-element rounding.  Which one a launch runs is
decided by a dozen conditions on shape, batch size, options and call state (step_choice, rollout_plan in csrc/ranenv_host.cpp), so a
test that merely carries a build's name may never have run it.  Here every reachable (build, MANY, SE mode, rounding) runs at two
shapes per row width -- one of one wave per env, one of two -- forced through set_option after create (not through the
environment: the result does not depend on how the suite was started), steps a device policy (MAPF + PF) over an oracle replay of
a directed case, and is held to the bars of tests/test_gpu_intent_branches.py: integers exact, observations within 1e-5 and one
float32 ulp of the rounded oracle value, rewards within 1e-9.  assert_build_ran then takes the launch counters' word for the build,
the MANY axis and the exact number of launches.

"1" cases are a step() loop: T launches of one TTI.  "many" cases are rollouts of 1, 6, 2 and the remaining TTIs on an unpartitioned
batch with option fuse = 64: one launch per call, the first of one TTI (the same build, MANY = false), the others of several.
The persistent builds run every call as work-queue launches (always the MANY form).  The streaming persistent build is chosen for
batches beyond 2 waves per SIMD only (below, the whole-row persistent build takes over), so that case runs a batch just beyond
that size, read from the device's CU count: env j plays what env j % B plays, the first B envs are compared with the oracle and
every other env with the env it copies, bit for bit.
"""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import directed_intents as di
from tests import intent_census as ic
from tests.gpu_common import STEP_BUILDS, assert_build_ran, check_all, device_env_of_run, launches_since, need_gpu, step_shape

# (name, S, U, R, G, Us): per row width one shape of one wave per env (nt == 64) and one of two (nt == 128).  Width 8 / one wave is
# tests/directed_intents.py's "packable" size (two envs per wave); width 10 / one wave needs S <= 8 (S >= 9 alone makes two waves of
# slice-table words) and Us in 9..10: the reference's own 5 x 25 with 10 UEs per slice.
SHAPES = (
    ("w8-nt64", 8, 32, 64, 2, 8),
    ("w8-nt128", 6, 90, 72, 3, 8),
    ("w10-nt64", 5, 25, 135, 5, 10),
    ("w10-nt128", 10, 100, 60, 3, 10),
    ("w16-nt64", 4, 37, 100, 5, 12),
    ("w16-nt128", 12, 100, 120, 3, 12),
)
SHAPE_BY_NAME = {s[0]: s for s in SHAPES}
EXPECTED_SHAPE = {"w8-nt64": (64, 8), "w8-nt128": (128, 8), "w10-nt64": (64, 10), "w10-nt128": (128, 10), "w16-nt64": (64, 16),
                  "w16-nt128": (128, 16)}

# (build, many, SE mode, per-element rounding) and the shapes it exists at
_ALL = tuple(s[0] for s in SHAPES)
_NT128 = tuple(s[0] for s in SHAPES if s[0].endswith("nt128"))
ROWS = (
    ("lean", False, "stream", False, _ALL), ("lean", True, "stream", False, _ALL),
    ("small", False, "stream", False, _ALL), ("small", True, "stream", False, _ALL),
    ("tiny1", False, "stream", False, _ALL),
    ("gather", False, "gather", False, _ALL), ("gather", True, "gather", False, _ALL),
    ("packed", False, "stream", False, ("w8-nt64",)), ("packed", True, "stream", False, ("w8-nt64",)),
    ("packed", False, "gather", False, ("w8-nt64",)), ("packed", True, "gather", False, ("w8-nt64",)),
    ("mixed", False, "stream", False, _NT128), ("mixed", True, "stream", False, _NT128),
    ("mixed", False, "gather", False, _NT128), ("mixed", True, "gather", False, _NT128),
    ("persist", True, "stream", False, _ALL), ("persist", True, "gather", False, _ALL),
    ("persist_tiny", True, "stream", False, _ALL),
    ("lean", False, "stream", True, _ALL), ("lean", True, "stream", True, _ALL),
    ("gather", False, "gather", True, _ALL), ("gather", True, "gather", True, _ALL),
)
MATRIX = [(b, m, se, pe, sh) for b, m, se, pe, shapes in ROWS for sh in shapes]

# what pick() of csrc/ranenv_step.hip can return for a step-mode launch: (build, several TTIs per launch)
PICKABLE = {("lean", False), ("lean", True), ("small", False), ("small", True), ("gather", False), ("gather", True), ("tiny1", False),
            ("mixed", False), ("mixed", True), ("packed", False), ("packed", True), ("persist", True), ("persist_tiny", True)}

# the options that choose the build, all set for every case (whatever the environment preset)
KNOBS = {
    "lean": dict(small_batch=0, tiny_step=0, pack=0, mix=0, persist=0),
    "small": dict(small_batch=1, tiny_step=0, pack=0, mix=0, persist=0),
    "tiny1": dict(small_batch=1, tiny_step=1, pack=0, mix=0, persist=0),
    "gather": dict(small_batch=0, tiny_step=1, pack=0, mix=0, persist=0),
    "packed": dict(small_batch=0, tiny_step=1, pack=1, mix=0, persist=0),
    "mixed": dict(small_batch=0, tiny_step=1, pack=0, mix=2, persist=0),
    "persist": dict(small_batch=0, tiny_step=1, pack=0, mix=0, persist=1, persist_chunk=3),
    "persist_tiny": dict(small_batch=0, tiny_step=1, pack=0, mix=0, persist=1, persist_chunk=3),
}

_RUNS = {}


def _run_of(shape, per_element):
    """The oracle's replay of the shape's case (kept for the module: every build at that shape compares against the same one).  Built
    the directed_intents way, not added to its CASES."""
    key = (shape, per_element)
    if key not in _RUNS:
        name, S, U, R, G, Us = SHAPE_BY_NAME[shape]
        k = _ALL.index(shape)
        _RUNS[key] = ic.replay(di._case("builds-" + name, S, U, R, G, Us, B=8 + 2 * (k % 3), steps=21 + k, n_scen=4, first=3 + 7 * k,
                                        load=1.2, low_se=3 if k % 2 else 0, policy=2, intra=1, D=(10, 2, 10, 7, 1, 10)[k],
                                        per_element=per_element))
    return _RUNS[key]


def _id(p):
    build, many, se_mode, pe, shape = p
    return f"{build}-{'many' if many else '1'}-{se_mode}{'-pe' if pe else ''}-{shape}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", MATRIX, ids=_id)
def test_build_vs_oracle(case):
    need_gpu()
    build, many, se_mode, pe, shape = case
    run = _run_of(shape, pe)
    c = run["case"]
    B, T = c["B"], c["steps"]
    assert 8 <= B <= 12 and 20 <= T <= 26
    batch = None
    if build == "persist" and se_mode == "stream":
        # just beyond 2 waves per SIMD (8 per CU): the smallest even batch whose rollouts the streaming persistent build takes
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        batch = (8 * cus // (EXPECTED_SHAPE[shape][0] // 64) + 2) // 2 * 2
    env = device_env_of_run(run, batch=batch)
    assert step_shape(env) == EXPECTED_SHAPE[shape]
    env.set_se_mode(se_mode)
    for k, v in dict(KNOBS[build], compact=1, fuse=64, persist_grid=0).items():
        env.set_option(k, v)
    env.reset()
    before = launches_since(env)

    def copies_agree(what):
        if batch is None:
            return
        src = torch.arange(batch, device=env.device) % B
        for k, x in dict(env.views(), obs_inter=env.obs_inter, obs_intra=env.obs_intra, reward=env.reward).items():
            if k != "episodes":
                assert torch.equal(x, x[src]), (what, k, "an env differs from the env whose inputs it shares")

    if not many:
        for t in range(T):
            obs, rew, done = env.step()
            check_all(run, t, env, obs, rew, _id(case))
        assert int(done.sum()) == B
        assert_build_ran(env, before, build, many=False, count=T)
    else:
        persistent = build.startswith("persist")
        t = 0
        for k in (1, 6, 2, T - 9):
            at = launches_since(env)
            obs, rew, done = env.rollout(k)
            torch.cuda.synchronize()
            t += k
            n = env.get_option("last_rollout_launches")
            assert env.get_option("last_rollout_persistent") == (1 if persistent else 0), (_id(case), k)
            assert persistent or n == 1, (_id(case), k, n)
            # (a persistent launch is the MANY form whatever its length; else a call of one TTI is one launch of the one-TTI form)
            assert_build_ran(env, at, build, many=persistent or k > 1, count=n)
            check_all(run, t - 1, env, {"obs_inter": obs["obs_inter"][:B], "obs_intra": obs["obs_intra"][:B]}, rew[:B], (_id(case), k))
            copies_agree((_id(case), k))
        assert t == T and env.get_option("persist_errors") == 0
        assert_build_ran(env, before, build)
    env.close()


@pytest.mark.gpu
def test_launch_counters_are_cumulative_read_only_and_not_preset_from_the_environment(monkeypatch):
    """step_launches(): sixteen keys, zero on a fresh handle whatever RANENV_STEP_LAUNCHES_* says (the keys are no rows of the options
    table), cumulative over calls, untouched by resets, refused by set_option as unknown like any other unknown key."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd.batched_env import RanEnvError
    monkeypatch.setenv("RANENV_STEP_LAUNCHES_LEAN", "5")
    monkeypatch.setenv("RANENV_STEP_LAUNCHES_LEAN_MANY", "5")
    run = _run_of("w10-nt64", False)
    env = device_env_of_run(run)
    for k, v in dict(KNOBS["lean"], compact=1, fuse=64).items():
        env.set_option(k, v)
    env.set_se_mode("stream")
    zero = {k: 0 for b in STEP_BUILDS for k in (b, b + "_many")}
    assert env.step_launches() == zero
    env.reset()
    assert env.step_launches() == zero
    env.step(); env.step()
    assert env.step_launches() == dict(zero, lean=2)
    env.rollout(5)
    assert env.step_launches() == dict(zero, lean=3, lean_many=1)
    env.reset()
    env.set_option("small_batch", 1)
    env.step()
    assert env.step_launches() == dict(zero, lean=3, lean_many=1, small=1)
    for key in ("step_launches_lean", "step_launches_lean_many", "step_launches_persist_tiny"):
        with pytest.raises(RanEnvError, match="unknown option"):
            env.set_option(key, 0)
    for key in ("step_launches_", "step_launches_many", "step_launches_lean_many_many", "step_launches_dense"):
        with pytest.raises(RanEnvError, match="unknown option"):
            env.get_option(key)
    assert env.step_launches() == dict(zero, lean=3, lean_many=1, small=1)
    env.close()


def test_the_matrix_covers_every_build_the_launch_table_can_pick():
    """From this module's own parameter table: every (build, MANY) that pick() can return for a step launch has a row, at every row
    width and -- where the build exists in both -- in both SE modes; and the builds pick() switches over are the eight the counters
    and this matrix know.  A build added to the launch table without a row here fails this test."""
    covered = {(b, m) for b, m, se, pe, sh in MATRIX}
    assert covered == PICKABLE, (covered ^ PICKABLE)
    assert {b for b, m in PICKABLE} == set(STEP_BUILDS)
    for b, m in PICKABLE:
        shapes = {sh for bb, mm, se, pe, sh in MATRIX if (bb, mm) == (b, m)}
        widths = {EXPECTED_SHAPE[sh][1] for sh in shapes}
        assert widths == ({8} if b == "packed" else {8, 10, 16}), (b, m, widths)
        waves = {EXPECTED_SHAPE[sh][0] for sh in shapes}
        assert waves == ({64} if b == "packed" else ({128} if b == "mixed" else {64, 128})), (b, m, waves)
    for b in ("packed", "mixed", "persist"):                       # the builds with a gather form of their own
        assert {se for bb, m, se, pe, sh in MATRIX if bb == b} == {"stream", "gather"}, b
    for b in ("lean", "gather"):                                   # the builds with a per-element form
        assert {(m, pe) for bb, m, se, pe, sh in MATRIX if bb == b} == {(False, False), (True, False), (False, True), (True, True)}, b
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "intent_radio_sched_multi_slice_amd", "csrc",
                            "ranenv_step.hip")).read()
    pick = src[src.index("step_kernel_t pick("):src.index("}  // namespace")]
    assert {n.lower() for n in re.findall(r"case SB_(\w+):", pick)} == set(STEP_BUILDS)
