"""What a rollout decides before it enqueues anything, pinned by the library's own counters: the schedule (one persistent work-queue
launch per class, or launches per chunk), how many launches, which build of the step kernel they run, and whether they read the
member-lines copy.

Counters only: that the builds compute the same numbers is held by tests/test_gpu_step_builds.py, tests/test_gpu_member_lines.py and
tests/test_gpu_configs.py.  Per row of TABLE a device env is made (device_env_of_run of the oracle replay test_gpu_step_builds keeps for
the shape, the batch sized from the device's CU count N), EVERY option that takes part in the decision is set after create (so a run of
the suite under RANENV_PERSIST / RANENV_SMALL_BATCH / RANENV_MEMBER_LINES presets decides the same), and per rollout(k) of the row
four things are compared: last_rollout_persistent, last_rollout_launches, last_rollout_member_lines and the step_launches() delta
(assert_build_ran: the named build and no other, that many launches, that many of them of several TTIs).

The expected values are what the library did BEFORE rollout_plan / step_choice (csrc/ranenv_host.cpp) replaced the conditions that
were spread over rollout_run, step_plan and persist_launch; the table was written first and run against that library.  The rules it
pins, with N the device's CU count and "waves" the waves of an env's block:
  - auto persistent: batch * waves <= 8 N (whole-row regime; streaming build persist_tiny, gather build persist); SE gather mode up
    to 44 N envs; streaming, not small_batch, up to 20 N envs and 4 <= k <= 64;
  - never persistent: option compact off, a policy net, head outputs, slice metrics, a trace, the per-element flag -- the first four
    also mean one TTI per launch -- nor (auto only) more than two distinct episode ends inside the call;
  - launches per chunk: fuse = clamp(k / 4, 1, 10) TTIs per launch; with partitions the first launches are fuse, (3 fuse + 4) / 5
    and -- the last partition -- 1 TTI long;
  - member lines: streaming, compact, not per-element, and the launches are the streaming persistent build (not the whole-row one)
    or the lean build of several TTIs (so not at fuse = 1: k < 8 at the default fuse).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.gpu_common import assert_build_ran, device_env_of_run, launches_since, make_inter_net, need_gpu, step_shape
from tests.test_gpu_step_builds import EXPECTED_SHAPE, _run_of

# the options of the decision at their defaults (small_batch: what ranenv_create derives, batch <= 8 N, see _env)
DEFAULTS = dict(compact=1, fuse=0, tiny_step=1, persist=-1, persist_chunk=10, persist_grid=0, pack=1, mix=1, member_lines=-1)

# batch of a row from (N, waves of a block, the replay's own B)
BATCH = {
    "case": lambda N, w, B: B,
    "whole-row": lambda N, w, B: 8 * N // w,                           # at 8 N waves
    "beyond": lambda N, w, B: (8 * N // w + 2) // 2 * 2,               # the smallest even batch beyond 8 N waves
    "above-20N": lambda N, w, B: 20 * N + 2,
    "below-44N": lambda N, w, B: 44 * N - 2,
    "above-44N": lambda N, w, B: 44 * N + 2,
}


def R(k, persistent, launches, member_lines, build, many, **options):
    """One rollout(k) of a row: the three read-only options, the build, how many of the launches are of several TTIs; ``options``
    are set just before it (and stay set)."""
    return dict(k=k, persistent=persistent, launches=launches, member_lines=member_lines, build=build, many=many, options=options)


def _blocker(setup, launches, many):
    """k = 8 at the beyond-8N streaming batch, where auto would run persistently: not with the blocker, nor with persist forced."""
    return (f"blocker-{setup}", "w16-nt64", "beyond", "stream", {}, setup, 1,
            (R(8, 0, launches, 0, "lean", many), R(8, 0, launches, 0, "lean", many, persist=1)))


# (id, shape, batch, SE mode, options beside DEFAULTS, setup, partitions, rollouts)
TABLE = (
    # whole-row regime: persistent whatever k, one class, never member lines
    ("whole-row-stream-nt64", "w16-nt64", "whole-row", "stream", {}, None, 1,
     (R(1, 1, 1, 0, "persist_tiny", 1), R(70, 1, 1, 0, "persist_tiny", 1))),
    ("whole-row-stream-nt128", "w8-nt128", "whole-row", "stream", {}, None, 1,
     (R(1, 1, 1, 0, "persist_tiny", 1), R(70, 1, 1, 0, "persist_tiny", 1))),
    ("whole-row-gather-nt64", "w16-nt64", "whole-row", "gather", {}, None, 1,
     (R(1, 1, 1, 0, "persist", 1), R(70, 1, 1, 0, "persist", 1))),
    ("whole-row-gather-nt128", "w8-nt128", "whole-row", "gather", {}, None, 1,
     (R(1, 1, 1, 0, "persist", 1), R(70, 1, 1, 0, "persist", 1))),
    # beyond 8 N waves, streaming: persistent for 4..64 TTIs; k = 1 and k = 3 run launches of one TTI (fuse = 1: no member lines)
    ("beyond-stream", "w16-nt64", "beyond", "stream", {}, None, 1,
     (R(1, 0, 1, 0, "lean", 0), R(3, 0, 3, 0, "lean", 0), R(4, 1, 1, 1, "persist", 1), R(64, 1, 1, 1, "persist", 1),
      R(65, 0, 7, 1, "lean", 7))),
    ("beyond-stream-small_batch", "w16-nt64", "beyond", "stream", dict(small_batch=1), None, 1,
     (R(3, 0, 3, 0, "small", 0), R(4, 0, 4, 0, "small", 0), R(64, 0, 7, 0, "small", 7), R(65, 0, 7, 0, "small", 7))),
    ("beyond-stream-member_lines-off", "w16-nt64", "beyond", "stream", dict(member_lines=0), None, 1,
     (R(3, 0, 3, 0, "lean", 0), R(4, 1, 1, 0, "persist", 1), R(64, 1, 1, 0, "persist", 1), R(65, 0, 7, 0, "lean", 7))),
    ("beyond-stream-compact-off", "w16-nt64", "beyond", "stream", dict(compact=0), None, 1,
     (R(4, 0, 4, 0, "lean", 0), R(64, 0, 7, 0, "lean", 7))),
    # the thresholds in envs per CU
    ("above-20N-stream", "w16-nt64", "above-20N", "stream", {}, None, 1, (R(20, 0, 4, 1, "lean", 4),)),
    ("below-44N-gather", "w16-nt64", "below-44N", "gather", {}, None, 1, (R(20, 1, 1, 0, "persist", 1),)),
    ("above-44N-gather", "w16-nt64", "above-44N", "gather", {}, None, 1, (R(20, 0, 4, 0, "gather", 4),)),
    # each blocker on its own: one TTI per launch (k launches), but for the per-element flag (fuse = 2)
    _blocker("net", 8, 0), _blocker("heads", 8, 0), _blocker("slice-metrics", 8, 0), _blocker("trace", 8, 0),
    _blocker("per-element", 4, 4),
    # auto-reset, per-env episode lengths: persistent launches run up to the next episode end of the batch (3 + 2 + 1 + 2 TTIs);
    # three distinct ends inside the call: launches per chunk, cut at every end (2 + 1 + 2 + 1 + 2 TTIs)
    ("two-ends", "w16-nt64", "beyond", "stream", {}, ("lengths", (3, 5)), 1, (R(8, 1, 4, 1, "persist", 4),)),
    ("three-ends", "w16-nt64", "beyond", "stream", {}, ("lengths", (3, 5, 6)), 1,
     (R(8, 0, 5, 1, "lean", 3), R(8, 1, 4, 1, "persist", 4, persist=1))),
    # partitions: k = 20 -> fuse 5, first launches 5 / 3 / 1: 4 + 5 + 5 launches, one of them of one TTI; k = 3 -> fuse 1
    ("partitions-1", "w16-nt64", "beyond", "stream", dict(persist=0), None, 1, (R(20, 0, 4, 1, "lean", 4), R(3, 0, 3, 0, "lean", 0))),
    ("partitions-3", "w16-nt64", "beyond", "stream", dict(persist=0), None, 3, (R(20, 0, 14, 1, "lean", 13), R(3, 0, 9, 0, "lean", 0))),
    # the builds that are neither lean nor persistent take no member lines (k = 6: fuse 1; fuse = 3: two launches of 3 TTIs)
    ("mixed", "w8-nt128", "case", "stream", dict(persist=0, mix=2), None, 1,
     (R(6, 0, 6, 0, "mixed", 0), R(6, 0, 2, 0, "mixed", 2, fuse=3))),
    ("packed", "w8-nt64", "case", "stream", dict(persist=0), None, 1,
     (R(6, 0, 6, 0, "packed", 0), R(6, 0, 2, 0, "packed", 2, fuse=3))),
)


def _env(shape, batch, se_mode, options, setup, parts):
    from intent_radio_sched_multi_slice_amd import _lib
    run = _run_of(shape, False)
    N = torch.cuda.get_device_properties(0).multi_processor_count
    nt = EXPECTED_SHAPE[shape][0]
    B = BATCH[batch](N, nt // 64, run["case"]["B"])
    env = device_env_of_run(run, max_steps=1000, batch=B, flags=_lib.F_SCALE_PER_ELEMENT if setup == "per-element" else 0)
    assert step_shape(env) == EXPECTED_SHAPE[shape] and env.B == B
    env.set_se_mode(se_mode)
    for key, v in {**DEFAULTS, "small_batch": 1 if B <= 8 * N else 0, **options}.items():
        env.set_option(key, v)
    if setup == "net":
        env.set_policy_network(make_inter_net(env.S, [8], "tanh", 1))
    elif setup == "heads":
        env.enable_heads()
    elif setup == "slice-metrics":
        env.enable_metrics(0)
        env.enable_slice_metrics()
    elif setup == "trace":
        env.bind_trace([0, 3], capacity=16, se=False)
    elif isinstance(setup, tuple):                     # ("lengths", per-env episode lengths in rotation), auto-reset on
        eps = env.episodes
        env.set_episode_table(scenario=eps["scenario"], se_base=eps["se_base"], se_len=eps["se_len"], se_offset=eps["se_offset"],
                              trf_base=eps["trf_base"], trf_len=eps["trf_len"], trf_offset=eps["trf_offset"])
        env.set_max_steps(np.asarray(setup[1], dtype=np.int32)[np.arange(B) % len(setup[1])])
        env.enable_autoreset(0, B, episode_numbers=np.arange(B, dtype=np.int32))
    if parts > 1:
        env.set_partitions(parts)
    return env


@pytest.mark.gpu
@pytest.mark.parametrize("row", TABLE, ids=lambda row: row[0])
def test_rollout_plan(row):
    need_gpu()
    name, shape, batch, se_mode, options, setup, parts, rollouts = row
    env = _env(shape, batch, se_mode, options, setup, parts)
    for r in rollouts:
        for key, v in r["options"].items():
            env.set_option(key, v)
        env.reset()                                    # (every step counter at 0: the episode ends fall where the row says)
        at = launches_since(env)
        env.rollout(r["k"])
        torch.cuda.synchronize()
        got = dict(persistent=env.get_option("last_rollout_persistent"), launches=env.get_option("last_rollout_launches"),
                   member_lines=env.get_option("last_rollout_member_lines"))
        delta = launches_since(env, at)
        print(name, "k", r["k"], r["options"], got, {key: v for key, v in delta.items() if v})
        assert got == {key: r[key] for key in got}, (name, r["k"], r["options"], got)
        assert_build_ran(env, at, r["build"], count=r["launches"])
        assert delta[r["build"] + "_many"] == r["many"], (name, r["k"], r["options"], delta)
    assert env.get_option("persist_errors") == 0
    env.close()
