"""Seeded fuzz of the step kernel against the CPU oracle: shapes, window depths, age caps, load levels and the way the
TTIs are issued (caller's scores, device policy step by step, device policy as a rollout over partitions) are drawn
from a fixed seed, so a failure reproduces from its case number.  Bars as everywhere: integers bit-exact, float32
observations within 1e-5, float64 rewards within 1e-9.

Every case ends with the library's launch counters (tests/gpu_common.py: assert_build_ran): the build the column is named for
ran, and no other.  The columns "lean", "small", "tiny1", "gather", "packed", "mixed", "per-element*" run draw_fuzz_case's shapes;
of those, none of the first 24 is packable and three can run mixed blocks, so under "packed" and "mixed" most of them assert the
build such a launch falls back to (build_for) -- they stay as the whole-row and persistent builds' fuzz at those knobs.  The
columns of test_fuzz_case_drawn_for_its_build take their shapes from draw_fuzz_case_for, inside what packed waves / mixed blocks
need, and every one of their cases runs the named build.

Rollouts: "lean", "small" and the drawn "packed*" / "mixed*" cases switch the persistent rollout off, so that the launches of
several TTIs of the named build run; the other columns leave it to the library, which takes batches of this size through one
persistent launch per call ("tiny1": the whole-row persistent build, "gather": the gather one).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.common import oracle_envs, poisson_traffic_rows, rb_major
from tests.gpu_common import assert_build_ran, assert_matches_oracle, build_for, launches_since, need_gpu, select_build
from tests.intent_census import draw_fuzz_case, draw_fuzz_case_for, even_cut, fuzz_scenarios
from tests.synth import se_tile

pytestmark = pytest.mark.gpu

N_CASES = int(__import__("os").environ.get("RANENV_FUZZ_CASES", "24"))   # more for a one-off soak: RANENV_FUZZ_CASES=400
N_DRAWN = max(1, N_CASES // 2)                                           # per column of the cases drawn for their build

CHUNKED = ("lean", "small")          # the names whose rollouts are to run the launches of several TTIs of the named build


def run_fuzz_case(build, c, k, B, parts, *, chunked, own_build):
    """One case on the device against the oracle; then which builds ran.  ``chunked``: the persistent rollout is switched off.
    ``own_build``: the case was drawn for the build, which must then be the one that ran."""
    # "per-element": RANENV_F_SCALE_PER_ELEMENT -- the other rounding of pkt_throughputs, in the oracle and in builds of their own
    flagged = build.startswith("per-element")
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.batched_env import BatchedRanEnv
    S, U, R, G, Us, D = c["S"], c["U"], c["R"], c["G"], c["Us"], c["D"]
    rng = np.random.default_rng(500 + k)
    tabs = fuzz_scenarios(c, 40 + k)
    steps = c["steps"]
    scen = rng.integers(0, tabs.n_scenarios, B)
    se_pool = np.stack([se_tile(300 + k, t, U, R, low_se_every=c["low_se"]) for t in range(B * steps)])
    trf = np.concatenate([poisson_traffic_rows(tabs, int(scen[b]), rng, steps) for b in range(B)]) * c["load"]
    trf = np.floor(trf)
    env = BatchedRanEnv(batch=B, n_slices=S, n_ues=U, n_rbs=R, rbs_per_rbg=G, max_ues_slice=Us,
                        n_scenarios=tabs.n_scenarios, max_steps=steps, hist_depth=D, flags=_lib.F_SCALE_PER_ELEMENT if flagged else 0)
    if build.startswith("mixed"):
        env.set_option("compact", 1)             # (mixed blocks are compact steps: whatever knob the suite runs under)
    env.load_scenarios(tabs)
    env.bind_se_pool(torch.as_tensor(rb_major(se_pool), device=env.device))
    env.bind_traffic_pool(torch.as_tensor(trf.astype(np.int32), device=env.device))
    env.set_episodes(scenario=scen, se_base=np.arange(B) * steps, se_len=steps, trf_base=np.arange(B) * steps, trf_len=steps)
    oenvs = oracle_envs(tabs, scen, (S, U, R, G, Us), steps, hist_depth=D, per_element=flagged)
    for b, o in enumerate(oenvs):
        o.reset(se_pool[b * steps])
    if c["how"] == "external":
        env.set_policy(0, 255)
    else:
        env.set_policy(c["policy"], c["intra"])
    intra_fixed = c["intra"]
    env.reset()
    before = launches_since(env)

    def oracle_step(t, sc, ic):
        """the oracle envs through TTI t; the allocations they expect of it"""
        counts = []
        for b, o in enumerate(oenvs):
            counts.append(o.action_format(sc[b], ic[b], want_dense=False)[1])
            o.step(sc[b], ic[b], se_pool[b * steps + t], trf[b * steps + t])
        return counts

    def device_scores():
        if c["policy"] == 1:
            return np.stack([o.policy_marr() for o in oenvs])
        return np.stack([o.policy_mapf() for o in oenvs])

    if c["how"] == "device_rollout":
        ranges = env.set_ranges(parts) if parts > 1 else [(0, B)]
        if chunked:
            env.set_option("persist", 0)
        counts = None
        for t in range(steps):
            counts = oracle_step(t, device_scores(), np.full((B, S), intra_fixed, dtype=np.uint8))
        obs, rew, done = env.rollout(steps)
        torch.cuda.synchronize()
        assert_matches_oracle(env, obs, rew, oenvs, (k, c, steps - 1), rb_count=counts)
        n = env.get_option("last_rollout_launches")
        if env.get_option("last_rollout_persistent") == 1:
            # one work-queue launch per class: the gather build in gather mode, else -- a batch within 2 waves per SIMD -- the whole-row one
            assert not chunked and not flagged and not own_build, (build, k, "a persistent rollout")
            delta = assert_build_ran(env, before, "persist" if env.se_mode == "gather" else "persist_tiny", many=True, count=n)
        else:
            # every partition in launches of its own, of one TTI or several: the build of each (range, launch form)
            names = {(m, build_for(env, build, many=m, n=hi - lo, partitions=parts, per_element=flagged)) for lo, hi in ranges for m in (True, False)}
            main = sorted({b for m, b in names if m})
            delta = assert_build_ran(env, before, tuple(main), also=tuple(sorted({b for m, b in names})), count=n)
            if own_build:
                assert main == [build.split("-")[0]], (build, k, main, ranges)
                assert ranges == list(zip(even_cut(B, parts), even_cut(B, parts)[1:])) or build.startswith("mixed"), (build, k, ranges)
    else:
        for t in range(steps):
            if c["how"] == "external":
                sc = rng.uniform(-1, 1, (B, S))
                sc[rng.random((B, S)) < 0.15] = -1.0
                ic = rng.integers(0, 3, (B, S)).astype(np.uint8)
                counts = oracle_step(t, sc, ic)
                obs, rew, done = env.step(sc, ic)
            else:
                sc = device_scores(); ic = np.full((B, S), intra_fixed, dtype=np.uint8)
                counts = oracle_step(t, sc, ic)
                obs, rew, done = env.step()
            assert_matches_oracle(env, obs, rew, oenvs, (k, c, t), buffers=False, rb_count=counts)
        want = build_for(env, build, per_element=flagged)
        if own_build:
            assert want == build.split("-")[0], (build, k, want)
        delta = assert_build_ran(env, before, want, many=False, count=steps)
    env.close()
    return delta


@pytest.mark.parametrize("k", range(N_CASES))
@pytest.mark.parametrize("build", ["lean", "small", "tiny1", "gather", "packed", "mixed", "per-element", "per-element-gather"])
def test_fuzz_case_vs_oracle(k, build, monkeypatch):
    """draw_fuzz_case's shapes under every build name.  "lean" / "small" / "tiny1" / "gather" / "per-element*" run the build they
    name at every shape (build_for asserts it for the first three); "packed" and "mixed" run theirs where the drawn shape allows it
    (packed: two envs per wave where U <= 32 and S, Us <= 8; mixed blocks where 64 < U <= 128, the step is compact and the launch
    covers the whole batch) and else assert the build the launch falls back to: the whole-row build for step loops, the whole-row
    persistent build for rollouts."""
    need_gpu()
    select_build(monkeypatch, build)
    run_fuzz_case(build, draw_fuzz_case(k), k, 8 if build == "packed" else 7, 3, chunked=build in CHUNKED, own_build=False)


@pytest.mark.parametrize("k", range(N_DRAWN))
@pytest.mark.parametrize("build", ["packed", "packed-gather", "mixed", "mixed-gather"])
def test_fuzz_case_drawn_for_its_build(k, build, monkeypatch):
    """draw_fuzz_case_for's shapes: every case runs packed waves / mixed blocks and nothing else, in step loops and -- the
    persistent rollout switched off -- in rollouts (packed: over partitions of even ranges; mixed: unpartitioned)."""
    need_gpu()
    select_build(monkeypatch, build)
    c = draw_fuzz_case_for(build, k)
    run_fuzz_case(build, c, 1000 + k, c["B"], c["parts"], chunked=True, own_build=True)
