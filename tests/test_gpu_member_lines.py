"""Member lines (include/ranenv.h, "MEMBER LINES"; option "member_lines"): compact streaming rollouts read a per-UE line copy of the
SE pool -- the rows of slice members only, eight lanes per member -- instead of whole tiles.  The copy is an index transform of
the pool, and every number a rollout produces with it is, bit for bit, what the rollout produces without it: for the lean build of
several TTIs and the streaming persistent build, at three shapes (row widths 10 / 8 / 16, one and two waves per env), for member
counts at the edges of a cluster of 8 and of a wave, through auto-resets that change the member set, after a rebind of the pool,
and inside a stream capture (where the copy is never built)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.gpu_common import assert_build_ran, comparable_views, launches_since, need_gpu, short_episode_setup
from tests.member_lines_ref import lay_out_pool, plan_of

pytestmark = pytest.mark.gpu

SHAPES = [dict(), dict(n_slices=5, n_ues=25, n_rbs=135, rbs_per_rbg=5, max_ues_slice=5, min_slices=3, min_ues=2),
          dict(n_slices=3, n_ues=40, n_rbs=419, max_ues_slice=16, min_slices=2, min_ues=3)]
LEAN = dict(small_batch=0, tiny_step=0, pack=0, mix=0, compact=1, fuse=64, persist=0)
PERSIST = dict(small_batch=0, tiny_step=1, pack=0, mix=0, compact=1, fuse=64, persist=1, persist_chunk=3, persist_grid=192)
CALLS = (1, 6, 2, 23, 9)


def _set(env, knobs, member_lines):
    for k, v in dict(knobs, member_lines=member_lines).items():
        env.set_option(k, v)


def _persist_batch(env_threads):
    """Just above 2 waves per SIMD (8 per CU): the smallest even batch whose rollouts the streaming persistent build takes
    (as tests/test_gpu_step_builds.py computes it)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return (8 * cus // (env_threads // 64) + 2) // 2 * 2


@pytest.mark.parametrize("quad", [0, 1])
@pytest.mark.parametrize("U,R", [(100, 135), (25, 135), (7, 5), (33, 8), (64, 130), (40, 419)])
def test_retile_member_lines_is_an_index_transform(U, R, quad):
    need_gpu()
    from intent_radio_sched_multi_slice_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    n = 5
    g = torch.Generator(device=dev); g.manual_seed(U * 1000 + R)
    rb = torch.rand((n, R, U), generator=g, device=dev, dtype=torch.float32)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    src, stride = rb, R * U
    if quad:
        Rq = (R + 3) // 4
        src = torch.empty((n, Rq, U, 4), device=dev, dtype=torch.float32)
        assert lib.ranenv_se_retile_quad(C.c_void_p(rb.data_ptr()), C.c_void_p(src.data_ptr()), n, U, R, stream) == 0
        stride = Rq * U * 4
    lines = len(plan_of(R))
    out = torch.full((n, U, lines, 32), -1.0, device=dev, dtype=torch.float32)
    assert lib.ranenv_se_retile_member_lines(C.c_void_p(src.data_ptr()), quad, stride, C.c_void_p(out.data_ptr()), n, U, R, stream) == 0
    torch.cuda.synchronize()
    want = lay_out_pool(rb.cpu().numpy())
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))        # (bits: the padding is +0.0)
    assert torch.equal(out, torch.as_tensor(want, device=dev))


def _snap(wl_or_env, tables=None):
    torch.cuda.synchronize()
    env = getattr(wl_or_env, "env", wl_or_env)
    v = comparable_views(wl_or_env) if tables is None else {k: x.clone() for k, x in env.views().items()}
    return v, env.obs_inter.clone(), env.obs_intra.clone(), env.reward.clone()


def _same(a, b, what):
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), (what, k)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]), what


def _walk(wl, knobs, member_lines, parts, persistent):
    """reset, then rollouts of CALLS TTIs: the snapshots, and per call (last_rollout_member_lines, launches)."""
    env = wl.env
    env.set_se_mode("stream")
    _set(env, knobs, member_lines)
    env.set_partitions(parts)
    env.reset()
    snaps, used = [_snap(wl)], []
    for k in CALLS:
        at = launches_since(env)
        env.rollout(k)
        snaps.append(_snap(wl))
        assert env.get_option("last_rollout_persistent") == (1 if persistent else 0), k
        assert_build_ran(env, at, "persist" if persistent else "lean", many=True if persistent else None)
        used.append(env.get_option("last_rollout_member_lines"))
    return snaps, used


@pytest.mark.parametrize("build", ["lean-1", "lean-3", "persist"])
@pytest.mark.parametrize("shape", range(3))
def test_member_lines_equal_whole_tiles_bit_for_bit(shape, build):
    need_gpu()
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    dev = torch.device("cuda", 0)
    kw = SHAPES[shape]
    persistent = build == "persist"
    nt = 128 if kw.get("n_ues", 100) > 64 else 64
    B = _persist_batch(nt) if persistent else 300
    outs = []
    for ml in (0, 1):
        wl = make_mult_slice_workload(B, dev, n_scenarios=12, n_traces=6, trace_len=20, max_steps=1000, **kw)
        snaps, used = _walk(wl, PERSIST if persistent else LEAN, ml, 1 if persistent else int(build[-1]), persistent)
        # the variant ran wherever it exists: every persistent launch, every rollout of more than one TTI of the lean build
        assert used == [ml if (persistent or k > 1) else 0 for k in CALLS], (build, ml, used)
        if persistent:
            assert wl.env.get_option("persist_errors") == 0 and wl.env.get_option("persist_stat_push") > 0      # envs changed hands
        outs.append(snaps)
        wl.env.close()
    for i, (a, b) in enumerate(zip(*outs)):
        _same(a, b, (shape, build, i))


def _directed(members, R, B, dev, last_tile_env=True):
    """U = 100, 10 slices of up to 10 UEs: scenario i has members[i] UEs in slices (the others idle)."""
    from intent_radio_sched_multi_slice_amd.batched_env import BatchedRanEnv
    from intent_radio_sched_multi_slice_amd.scenario import SLICE_TEMPLATES, ScenarioTables, slice_template_dict
    from intent_radio_sched_multi_slice_amd.workloads import mimic_quadriga_pool, poisson_traffic_pool
    S, U, Us, n_traces, L = 10, 100, 10, 4, 12
    rng = np.random.default_rng(5 + R)
    t = ScenarioTables.empty(len(members), S, U, Us)
    for i, m in enumerate(members):
        counts = [Us] * (m // Us) + ([m % Us] if m % Us else [])
        ues = rng.choice(U, m, replace=False)
        bsa, sua = np.zeros((1, S)), np.zeros((S, U))
        req = {f"slice_{s}": {} for s in range(S)}
        used = 0
        for s, cnt in enumerate(counts):
            bsa[0, s] = 1
            req[f"slice_{s}"] = slice_template_dict((s + i) % len(SLICE_TEMPLATES))
            sua[s, ues[used:used + cnt]] = 1
            used += cnt
        t.set_from_reference(i, bsa, sua, req, True)
    env = BatchedRanEnv(batch=B, n_slices=S, n_ues=U, n_rbs=R, rbs_per_rbg=1, max_ues_slice=Us, n_scenarios=len(members), max_steps=1000,
                        device=dev)
    env.load_scenarios(t)
    env.bind_se_pool(mimic_quadriga_pool(n_traces, L, U, R, 77 + R, env.device))
    env.bind_traffic_pool(torch.from_numpy(poisson_traffic_pool(t, L, 9)).to(env.device))
    scen = np.arange(B) % len(members)
    trace = np.arange(B) % n_traces
    off = rng.integers(0, L, B)
    if last_tile_env:                      # env B - 1 starts at the pool's last tile
        trace[B - 1] = n_traces - 1; off[B - 1] = L - 1
    env.set_episodes(scenario=scen, se_base=trace * L, se_len=L, se_offset=off, trf_base=scen * L, trf_len=L, trf_offset=rng.integers(0, L, B))
    env.set_policy(2, 1)
    return env, t


@pytest.mark.parametrize("R", [8, 5])
@pytest.mark.parametrize("build", ["lean", "persist"])
def test_member_counts_at_the_edges_of_a_cluster_and_of_a_wave(R, build):
    """1, 7, 8, 9, 63, 64, 65 and all 100 UEs in slices; R = 8 is one line without a tail, R = 5 the tail line alone.  The last env
    starts at the pool's last tile."""
    need_gpu()
    dev = torch.device("cuda", 0)
    members = (1, 7, 8, 9, 63, 64, 65, 100)
    persistent = build == "persist"
    B = _persist_batch(128) if persistent else 24
    outs = []
    for ml in (0, 1):
        env, t = _directed(members, R, B, dev)
        env.set_se_mode("stream")
        _set(env, PERSIST if persistent else LEAN, ml)
        env.reset()
        snaps = [_snap(env, t)]
        for k in (5, 9):
            env.rollout(k)
            snaps.append(_snap(env, t))
            assert env.get_option("last_rollout_member_lines") == ml
        outs.append(snaps)
        env.close()
    for i, (a, b) in enumerate(zip(*outs)):
        _same(a, b, (R, build, i))


@pytest.mark.parametrize("build", ["lean", "persist"])
def test_auto_reset_changes_the_member_set_between_launches(build):
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
            env.rollout(k)
            torch.cuda.synchronize()
            snaps.append(({n: x.clone() for n, x in env.views().items()}, env.obs_inter.clone(), env.obs_intra.clone(), env.reward.clone()))
            assert env.get_option("last_rollout_member_lines") == ml, k
        outs.append(snaps)
        env.close()
    for i, (a, b) in enumerate(zip(*outs)):
        _same(a, b, (build, i))


def test_rebinding_the_pool_rebuilds_the_copy():
    """Rollouts, then a second pool with other values is bound to the same handle: the results follow the new pool -- those of a
    fresh handle bound to it, and those of a handle that went the same way with the variant off.  (The handles clear the 10-TTI
    window at a reset: without that flag a reset handle keeps its window and a fresh handle has none, whatever the SE path.)  In
    between the SE gather mode and back: the copy survives it."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload, mimic_quadriga_pool
    dev = torch.device("cuda", 0)
    kw = dict(n_scenarios=12, n_traces=6, trace_len=20, max_steps=1000, seed=10, flags=_lib.F_CLEAR_HISTORY_ON_RESET)
    B = 64
    pool2 = mimic_quadriga_pool(6, 20, 100, 135, 4242, dev)

    def walk(env):
        env.set_se_mode("stream")
        env.reset(); env.rollout(7); a = env.get_option("last_rollout_member_lines")
        env.set_se_mode("gather"); env.rollout(5); g = env.get_option("last_rollout_member_lines")
        env.set_se_mode("stream"); env.rollout(9); b = env.get_option("last_rollout_member_lines")
        torch.cuda.synchronize()
        v = env.views()
        return (a, g, b), [x.clone() for x in (env.reward, env.obs_inter, env.obs_intra, v["queue_pkts"], v["pkt_throughputs"], v["pkt_effective_thr"])]

    # the same episodes on the second pool (make_mult_slice_workload's own draws)
    rng = np.random.default_rng(kw["seed"] + 31)
    scenario = rng.integers(0, 12, B); se_offset = rng.integers(0, 20, B); trf_offset = rng.integers(0, 20, B)
    rebound = []
    for ml in (1, 0):
        wl = make_mult_slice_workload(B, dev, **kw)
        _set(wl.env, LEAN, ml)
        used0, first = walk(wl.env)
        wl.env.bind_se_pool(pool2)
        wl.env.set_episodes(scenario=scenario, se_base=(np.arange(B) % 6) * 20, se_len=20, se_offset=se_offset, trf_base=scenario * 20, trf_len=20,
                            trf_offset=trf_offset)
        used1, again = walk(wl.env)
        assert used0 == (ml, 0, ml) and used1 == (ml, 0, ml), (ml, used0, used1)
        assert not torch.equal(first[0], again[0])          # (the second pool's values differ)
        rebound.append(again)
        wl.env.close()
    fresh = make_mult_slice_workload(B, dev, se_pool=pool2, **kw)
    _set(fresh.env, LEAN, 0)
    used2, want = walk(fresh.env)
    assert used2 == (0, 0, 0)
    for i, (x, y, z) in enumerate(zip(rebound[0], rebound[1], want)):
        assert torch.equal(x, y), ("variant on / off over the rebind", i)
        assert torch.equal(x, z), ("rebound handle / fresh handle", i)
    fresh.env.close()


def test_a_captured_rollout_does_not_build_the_copy():
    need_gpu()
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    dev = torch.device("cuda", 0)
    outs = []
    for captured in (False, True):
        wl = make_mult_slice_workload(64, dev, n_scenarios=12, n_traces=6, trace_len=20, max_steps=1000)
        env = wl.env
        env.set_se_mode("stream")
        _set(env, LEAN, 0 if not captured else 1)
        env.reset(); env.step(); torch.cuda.synchronize()
        if not captured:
            env.rollout(6); env.rollout(6)
        else:
            s = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(s):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
                    env.rollout(6)
            assert env.get_option("last_rollout_member_lines") == 0
            g.replay(); g.replay()
        outs.append(_snap(wl))
        env.close()
    _same(outs[0], outs[1], "captured")


def test_the_member_kernels_fit_five_waves_per_simd():
    """From the shipped code object (tools/kernel_resources.py, as tests/test_kernel_resources.py reads it)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from intent_radio_sched_multi_slice_amd.csrc import build as hip_build
    import kernel_resources
    hip_build.build()
    by = {k["name"]: k for k in kernel_resources.kernel_resources()}
    for n in ("ranenv_core_kernel_members<10>", "ranenv_persist_kernel_members<10>"):
        assert n in by, n
        assert by[n]["vgpr_count"] <= 96 and by[n].get("private_segment_fixed_size", 0) == 0 and by[n].get("vgpr_spill_count", 0) == 0, by[n]
