"""The serving order of member lines (include/ranenv.h, "MEMBER LINES": ranenv_member_serving_order): the members step kernels
serve the holders of an RB first and run a sum-only body for the passes behind the last holder.  Which cluster and pass serves a
member changes no bit: the same rollouts with member lines off (whole tiles, lane = UE, no serving order at all) and on give
torch.equal views, observations and rewards -- for the lean build over 1 and 3 partitions and the streaming persistent build, under
the device policies MAPF + PF, MARR + RR and MAPF + maximum throughput (other holder sets: who holds an RB is the intra-slice
scheduler's choice), at the headline shape (two-wave envs, 5 lines per UE), a 16-wide shape of 17 lines per UE and a one-line shape whose
ahead-requested prefix is half a wave, and through auto-resets that change the member set.  One test reads rb_count back and shows
that the walks had waves with sum-only passes and waves with none."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.gpu_common import assert_build_ran, comparable_views, launches_since, need_gpu, short_episode_setup

pytestmark = pytest.mark.gpu

# (headline: S 10 / U 100 / R 135; NP 16 with 17 lines per UE; one line per UE: P0 = 4 passes requested ahead)
SHAPES = [dict(), dict(n_slices=3, n_ues=40, n_rbs=419, max_ues_slice=16, min_slices=2, min_ues=3),
          dict(n_slices=6, n_ues=48, n_rbs=24, max_ues_slice=8, min_slices=4, min_ues=5)]
LINES = (5, 17, 1)
LEAN = dict(small_batch=0, tiny_step=0, pack=0, mix=0, compact=1, fuse=64, persist=0)
PERSIST = dict(small_batch=0, tiny_step=1, pack=0, mix=0, compact=1, fuse=64, persist=1, persist_chunk=3, persist_grid=192)
CALLS = (1, 6, 2, 23, 9)
POLICIES = {"mapf-pf": (2, 1), "marr-rr": (1, 0), "mapf-mt": (2, 2)}      # (_lib.POLICY_*, _lib.INTRA_*)


def _set(env, knobs, member_lines):
    for k, v in dict(knobs, member_lines=member_lines).items():
        env.set_option(k, v)


def _persist_batch(env_threads):
    """Just above 2 waves per SIMD (8 per CU): the smallest even batch whose rollouts the streaming persistent build takes."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return (8 * cus // (env_threads // 64) + 2) // 2 * 2


def _snap(wl):
    torch.cuda.synchronize()
    env = wl.env
    return comparable_views(wl), env.obs_inter.clone(), env.obs_intra.clone(), env.reward.clone()


def _same(a, b, what):
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), (what, k)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]), what


def _walk(wl, knobs, member_lines, parts, persistent, stats=None):
    env = wl.env
    env.set_se_mode("stream")
    _set(env, knobs, member_lines)
    env.set_partitions(parts)
    env.reset()
    snaps = [_snap(wl)]
    for k in CALLS:
        at = launches_since(env)
        env.rollout(k)
        snaps.append(_snap(wl))
        assert env.get_option("last_rollout_persistent") == (1 if persistent else 0), k
        assert_build_ran(env, at, "persist" if persistent else "lean", many=True if persistent else None)
        # the members build ran wherever it exists: every persistent launch, every rollout of more than one TTI of the lean build
        assert env.get_option("last_rollout_member_lines") == (member_lines if (persistent or k > 1) else 0), k
        if stats is not None:
            stats.append(_wave_passes(wl, stats.lines))
    return snaps


def _wave_passes(wl, nl):
    """Per wave that holds a member, at the TTI the views show: (passes walked, passes that keep the masked sum), from rb_count
    through ranenv_member_serving_order.  Lane l of an env owns its l-th member in ascending UE order."""
    from intent_radio_sched_multi_slice_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    count = wl.env.views()["rb_count"].cpu().numpy()
    member = wl.tables.ue_slice[wl.scenario] >= 0
    slots, mp = (C.c_int32 * 64)(), C.c_int32()
    out = []
    for b in range(count.shape[0]):
        holds = count[b][member[b]] > 0              # (ascending UE id = lane order)
        for w0 in range(0, holds.size, 64):
            h = holds[w0:w0 + 64]
            mm = (1 << h.size) - 1
            hm = sum(1 << int(l) for l in np.flatnonzero(h))
            assert lib.ranenv_member_serving_order(mm, hm, nl, 4, slots, C.byref(mp)) == 0
            out.append((-(-h.size // 8), mp.value))
    return out


class _Stats(list):
    lines = 0


@pytest.mark.parametrize("build", ["lean-1", "lean-3", "persist"])
@pytest.mark.parametrize("policy", sorted(POLICIES))
@pytest.mark.parametrize("shape", range(3))
def test_serving_order_changes_no_bit(shape, policy, build):
    need_gpu()
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    dev = torch.device("cuda", 0)
    kw = SHAPES[shape]
    persistent = build == "persist"
    nt = 128 if kw.get("n_ues", 100) > 64 else 64
    B = _persist_batch(nt) if persistent else 300
    pol, intra = POLICIES[policy]
    outs = []
    for ml in (0, 1):
        wl = make_mult_slice_workload(B, dev, policy=pol, intra=intra, n_scenarios=12, n_traces=6, trace_len=20, max_steps=1000, **kw)
        outs.append(_walk(wl, PERSIST if persistent else LEAN, ml, 1 if persistent else int(build[-1]), persistent))
        if persistent:
            assert wl.env.get_option("persist_errors") == 0
        wl.env.close()
    for i, (a, b) in enumerate(zip(*outs)):
        _same(a, b, (shape, policy, build, i))


@pytest.mark.parametrize("shape", range(3))
def test_the_walks_have_waves_with_sum_only_passes_and_waves_with_none(shape):
    """Otherwise the equality above would say nothing about the sum-only body: under MAPF + PF some waves walk passes behind their last
    holder (masked passes < passes) and some keep the masked sum to the end; under MARR + RR some waves keep it to the end as well."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    dev = torch.device("cuda", 0)
    seen = {}
    for policy in ("mapf-pf", "marr-rr"):
        pol, intra = POLICIES[policy]
        wl = make_mult_slice_workload(300, dev, policy=pol, intra=intra, n_scenarios=12, n_traces=6, trace_len=20, max_steps=1000, **SHAPES[shape])
        stats = _Stats()
        stats.lines = LINES[shape]
        from intent_radio_sched_multi_slice_amd import _lib
        assert _lib.load().ranenv_member_line_plan(wl.env.R, 0, None, None, None) == LINES[shape]
        _walk(wl, LEAN, 1, 1, False, stats)
        wl.env.close()
        waves = [x for per_call in stats for x in per_call]
        seen[policy] = (sum(1 for p, m in waves if m < p), sum(1 for p, m in waves if m == p), len(waves))
        assert all(1 <= m <= p for p, m in waves), policy
    print("waves (with sum-only passes, without, all):", seen)
    some, none_, _ = seen["mapf-pf"]
    assert some > 0 and none_ > 0, seen
    assert seen["marr-rr"][1] > 0, seen


@pytest.mark.parametrize("build", ["lean", "persist"])
def test_serving_order_through_auto_resets_that_change_the_member_set(build):
    """Episodes of 13 TTIs over a table of alternating scenarios; rollouts that end inside an episode and exactly on its end."""
    need_gpu()
    persistent = build == "persist"
    B = _persist_batch(64) if persistent else 48
    outs = []
    for ml in (0, 1):
        env, tabs, *_ = short_episode_setup(B, 13, idle_traffic=False)
        env.set_se_mode("stream")
        _set(env, PERSIST if persistent else LEAN, ml)
        env.reset()
        snaps = []
        for k in (5, 8, 13, 7, 19):          # ends: inside, on the end (13), on the end (26), inside, on the end (52)
            at = launches_since(env)
            env.rollout(k)
            torch.cuda.synchronize()
            snaps.append(({n: x.clone() for n, x in env.views().items()}, env.obs_inter.clone(), env.obs_intra.clone(), env.reward.clone()))
            assert_build_ran(env, at, "persist" if persistent else "lean", many=True)
            assert env.get_option("last_rollout_member_lines") == ml, k
        outs.append(snaps)
        env.close()
    for i, (a, b) in enumerate(zip(*outs)):
        _same(a, b, (build, i))
