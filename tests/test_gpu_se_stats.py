"""Scenario load on the device (ranenv_build_se_stats / ranenv_rbs_needed) against numpy float64 and the restatement of
results/gen_results.py in tests/se_stats_ref.py; tests/test_se_stats_cpu.py holds that restatement against the reference's own
output and asserts that the inputs used here reach every branch.  Everything is compared exactly: the kernels restate numpy's
summation order, and the build has correctly rounded /, sqrt and no contraction."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import se_stats_ref as ssr
from tests.common import rb_major
from tests.gpu_common import assert_same_state, need_gpu, small_workload

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TILES = 37


def _env(S, U, Us, R, n_scenarios=1, max_steps=16, batch=1):
    from intent_radio_sched_multi_slice_amd.batched_env import BatchedRanEnv
    return BatchedRanEnv(batch=batch, n_slices=S, n_ues=U, n_rbs=R, rbs_per_rbg=1, max_ues_slice=Us, n_scenarios=n_scenarios,
                         max_steps=max_steps)


def _tiles(U, R, seed, n=N_TILES):
    """(n, U, R) float32: synthetic tiles with a few spiky and starved rows among them."""
    role = np.full(U, -1)
    role[1::7] = ssr.SPIKY
    role[3::5] = ssr.STARVED
    return np.stack([ssr.directed_tile(role, seed, t, U, R) for t in range(n)])


def _quad(tiles_ur, pad_value):
    """(n, U, R) -> RB-quad-major (n, ceil(R/4), U, 4), the slots behind RB R-1 holding ``pad_value``."""
    n, U, R = tiles_ur.shape
    Rq = (R + 3) // 4
    q = np.full((n, Rq * 4, U), pad_value, dtype=np.float32)
    q[:, :R] = np.swapaxes(tiles_ur, 1, 2)
    return np.ascontiguousarray(q.reshape(n, Rq, 4, U).transpose(0, 1, 3, 2))


# ---- statistics -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U", [25, 100, 256])
@pytest.mark.parametrize("R", [7, 8, 9, 129, 135, 488])
def test_tile_stats_equal_numpy_in_both_layouts(R, U):
    """below a leaf's 8, one group, a tail, past numpy's 128 split, the workload's own, the largest; one, two and four waves"""
    need_gpu()
    tiles = _tiles(U, R, seed=R * 1000 + U)
    want = ssr.tile_stats(tiles)
    env = _env(5, U, min(16, max(3, U // 5)), R)
    pool = torch.as_tensor(rb_major(tiles), device=env.device)
    got = {}
    for layout in ("rb", "quad"):
        env.bind_se_pool(pool, layout=layout)
        assert env.se_layout == layout
        got[layout] = env.se_tile_stats().cpu().numpy().copy()
        assert got[layout].shape == (N_TILES, 4, U)
    for k, name in enumerate(("mean", "std", "min", "max")):
        assert np.array_equal(got["rb"][:, k], want[:, k]), (name, "rb")
        assert np.array_equal(got["quad"][:, k], want[:, k]), (name, "quad")
    env.set_se_mode("gather")
    assert np.array_equal(env.se_sidecars()["row_mean"].cpu().numpy(), got["quad"][:, 0])     # bit for bit the gather sidecar's mean
    assert np.array_equal(env.se_tile_stats().cpu().numpy(), got["quad"])                     # (the mode does not touch them)
    env.close()


@pytest.mark.parametrize("R,U", [(135, 25), (9, 100), (130, 70)])
def test_tile_stats_with_padded_stride_and_poisoned_padding(R, U):
    """Any tile_stride; what lies between the tiles, and the quad layout's slots behind RB R-1, takes no part (it is poisoned here:
    one element read would wreck a minimum, a maximum or a sum)."""
    need_gpu()
    n = 11
    tiles = _tiles(U, R, seed=R + U, n=n)
    want = ssr.tile_stats(tiles)
    env = _env(5, U, 5, R)
    lib, h = env._lib, env._h
    Rq = (R + 3) // 4
    for quad, stride, body in ((0, U * R + 7, rb_major(tiles).reshape(n, -1)), (1, Rq * U * 4 + 12, None)):
        for poison in (3e38, -3e38):
            if quad:
                body = _quad(tiles, poison).reshape(n, -1)
            flat = np.full((n, stride), poison, dtype=np.float32)
            flat[:, :body.shape[1]] = body
            dev = torch.as_tensor(flat, device=env.device)
            bind = lib.ranenv_bind_se_pool_quad if quad else lib.ranenv_bind_se_pool
            env._check(bind(h, C.c_void_p(dev.data_ptr()), n, stride), "bind")
            got = env.se_tile_stats().cpu().numpy()
            assert np.array_equal(got, want), (quad, poison)
    env.close()


# ---- RBs needed -----------------------------------------------------------------------------------------------------------------------
def _load_env(case, T):
    env = _env(case["S"], case["U"], case["Us"], case["R"], n_scenarios=case["tabs"].n_scenarios, max_steps=T)
    env.load_scenarios(case["tabs"])
    env.bind_se_pool(torch.as_tensor(rb_major(case["pool"]), device=env.device))
    return env


def _gamma(n):
    u = 2.0 ** -53
    return n * u / (1 - n * u)


def _check_case(case, T):
    env = _load_env(case, T)
    full = {k: v.cpu().numpy() for k, v in env.scenario_load(case["eps"], T, per_step=True).items()}
    lean = {k: v.cpu().numpy() for k, v in env.scenario_load(case["eps"], T).items()}
    assert set(lean) == {"episode_mean"} and np.array_equal(lean["episode_mean"], full["episode_mean"])
    for i in range(len(case["eps"])):
        per_slice, net, ep_mean = ssr.episode_load(case, i, T)
        assert np.array_equal(full["per_step_slice"][i], per_slice), i
        assert np.array_equal(full["per_step_network"][i], net), i
        assert np.array_equal(full["episode_mean"][i], ep_mean), i                     # numpy's order is reproduced
        ref = np.mean(full["per_step_network"][i], axis=0)                            # ... and any order is within gamma_{T-1} (terms >= 0)
        assert np.all(np.abs(full["episode_mean"][i] - ref) <= _gamma(T - 1) * np.abs(ref)), i
    return env, full


@pytest.mark.parametrize("name", list(ssr.DEVICE_CASES))
def test_rbs_needed_equals_the_restatement(name):
    """S 5 / U 25, S 10 / U 100, S 16 / U 256 (Us 16: the U sum splits pairwise); episodes on different scenario rows, traces
    shorter than the episode (the modulo wraps) and entered at an offset"""
    need_gpu()
    case, T = ssr.device_case(name)
    env, full = _check_case(case, T)
    assert full["per_step_slice"].shape == (len(case["eps"]), T, case["S"], 6)
    # the defaults: the bound episode table and max_steps
    env.set_episode_table(scenario=case["eps"]["scenario"], se_base=case["eps"]["se_base"], se_len=case["eps"]["se_len"],
                          se_offset=case["eps"]["se_offset"])
    assert np.array_equal(env.scenario_load()["episode_mean"].cpu().numpy(), full["episode_mean"])
    env.close()


def test_golden_episodes_on_the_device():
    """the three episodes of tests/golden/rbs_needed.npz (the reference's own output): every array exactly, and the chosen three"""
    from intent_radio_sched_multi_slice_amd.scenario import rank_by_load
    need_gpu()
    g = np.load(os.path.join(REPO, "tests", "golden", "rbs_needed.npz"), allow_pickle=True)
    case, T = ssr.golden_case(), ssr.GOLDEN["T"]
    env, full = _check_case(case, T)
    for n in range(3):
        for c, w in enumerate(("avg", "min", "max")):
            assert np.array_equal(full["per_step_network"][n, :, c], g[f"network_{w}_needed_rbs"][n]), (n, w)
            assert np.array_equal(full["per_step_slice"][n, :, :, c].T, g[f"slice_{w}_needed_rbs"][n]), (n, w)
        for c, key in ((3, "throughput_per_rb"), (4, "throughput_per_rb_min"), (5, "throughput_per_rb_max")):
            assert np.array_equal(full["per_step_slice"][n, :, :, c].T, g[key][n]), (n, key)
    assert np.array_equal(full["episode_mean"][:, 0], g["total_avg_needed_rbs"])
    assert list(rank_by_load(full["episode_mean"][:, 0])) == g["chosen"].tolist()
    env.close()


def test_episode_mean_over_a_long_episode():
    """T = 1000 on a trace of 7 tiles: the mean over the steps runs through numpy's pairwise recursion (three levels deep)"""
    need_gpu()
    S, U, Us, R, T = 5, 25, 5, 135, 1000
    case = ssr.make_case(S, U, Us, R, [1, 0], [7, 3], [2, 0], seed=9)
    env, _ = _check_case(case, T)
    env.close()


# ---- side effects ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["stream", "gather"])
def test_building_the_statistics_changes_nothing_else(mode):
    need_gpu()
    B, n = 24, 9
    a, b = small_workload(B, 40), small_workload(B, 40)
    for wl in (a, b):
        wl.env.set_se_mode(mode)
        wl.env.reset()
    stats = b.env.se_tile_stats().clone()
    load = b.env.scenario_load(n_steps=5)["episode_mean"].clone()
    a.env.rollout(n)
    b.env.rollout(n)
    assert_same_state(a.env, b.env, a.tables, f"rollout({n}) with and without the statistics, {mode}", loose=())
    assert torch.equal(b.env.se_tile_stats(), stats)                                  # ... and steps leave the statistics alone
    assert torch.equal(b.env.scenario_load(n_steps=5)["episode_mean"], load)
    tiles = b.env.pooled_tiles(torch.arange(stats.shape[0], device=b.env.device)).cpu().numpy()
    assert np.array_equal(stats.cpu().numpy(), ssr.tile_stats(np.swapaxes(tiles, 1, 2)))
    a.env.close()
    b.env.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors():
    from intent_radio_sched_multi_slice_amd._lib import RanEnvError
    need_gpu()
    case, T = ssr.device_case("S5_U25")
    S, U, Us, R = case["S"], case["U"], case["Us"], case["R"]
    env = _env(S, U, Us, R, n_scenarios=3, max_steps=T)
    lib, h = env._lib, env._h
    E_INVALID, E_STATE = -1, -3
    eps = case["eps"].copy()
    out = torch.zeros((len(eps), 3), dtype=torch.float64, device=env.device)

    def call(e, n_steps=T, n=None):
        e = np.ascontiguousarray(e)
        return lib.ranenv_rbs_needed(h, C.c_void_p(e.ctypes.data), len(e) if n is None else n, n_steps, None, None, C.c_void_p(out.data_ptr()), None)

    assert lib.ranenv_build_se_stats(h, None) == E_STATE                              # no pool bound
    with pytest.raises(RanEnvError, match="SE pool"):
        env.se_tile_stats()
    assert lib.ranenv_get_se_stats(h, None, None) == E_STATE
    env.load_scenarios(case["tabs"])
    pool = torch.as_tensor(rb_major(case["pool"]), device=env.device)
    env.bind_se_pool(pool)
    assert call(eps) == E_STATE and b"ranenv_build_se_stats" in lib.ranenv_last_error(h)   # statistics not built
    n_tiles = env.se_tile_stats().shape[0]
    assert call(eps) == 0
    for field, value in (("scenario", 3), ("scenario", -1), ("se_len", 0), ("se_offset", -1), ("se_base", -1)):
        bad = eps.copy()
        bad[field][1] = value
        assert call(bad) == E_INVALID, (field, value)
        assert b"episode 1" in lib.ranenv_last_error(h)
    bad = eps.copy()
    bad["se_offset"][2] = bad["se_len"][2]
    assert call(bad) == E_INVALID
    bad = eps.copy()
    bad["se_base"][3] = n_tiles - bad["se_len"][3] + 1                                # the trace leaves the pool by one tile
    assert call(bad) == E_INVALID and b"exceeds the pool" in lib.ranenv_last_error(h)
    assert call(eps, n_steps=0) == E_INVALID and call(eps, n=0) == E_INVALID
    assert lib.ranenv_rbs_needed(h, C.c_void_p(eps.ctypes.data), len(eps), T, None, None, None, None) == E_INVALID
    with pytest.raises(RanEnvError, match="n_steps"):
        env.scenario_load(eps, 0)
    assert torch.equal(out, env.scenario_load(eps, T)["episode_mean"])               # the failed calls wrote nothing
    # binding a pool drops the statistics -- the same pool again, too
    env.bind_se_pool(pool)
    assert lib.ranenv_get_se_stats(h, None, None) == E_STATE and call(eps) == E_STATE
    assert env.se_tile_stats().shape[0] == n_tiles and call(eps) == 0                # ... and they are built again on first use
    # a handle fed from power alone has no float32 pool
    power = torch.rand((4, R, U), dtype=torch.float64, device=env.device) * 1e-9
    env.bind_se_gather_from_power(power)
    assert lib.ranenv_get_se_stats(h, None, None) == E_STATE
    assert lib.ranenv_build_se_stats(h, None) == E_STATE and b"straight from power" in lib.ranenv_last_error(h)
    with pytest.raises(RanEnvError):
        env.scenario_load(eps, T)
    env.close()
