"""Populations without a device: the launch geometry of the library (ranenv_population_tiles, computed by the function the kernel
uses) against its Python restatement in tests/population_ref.py, the tables and lists that are refused, planted slips of the
env -> member map that the float64 twin must show, the twin's share of decidable rows for the nets the GPU tests use,
``evaluate_population``'s reduction, and the new exports."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import population_ref as pop
from tests import policy_ref as pr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1357_9BDF_2468_ACE0
MODES = [False, True]
E_INVALID = -1
NEW_EXPORTS = ("ranenv_set_population", "ranenv_get_population", "ranenv_set_population_policy", "ranenv_set_population_value",
               "ranenv_set_population_member", "ranenv_population_tiles")


@pytest.fixture(scope="module")
def lib():
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.csrc import build
    build.build()
    return _lib.load()


def _tiles(lib, first, e0, n, rpe, outs=True):
    """(status, [(member, row0, rows)]) of ranenv_population_tiles"""
    first = np.asarray(first, dtype=np.int32)
    G = len(first) - 1
    cap = (n * rpe + 31) // 32 + max(G, 0) + 1 if n > 0 and rpe > 0 else 1
    mem, row0, rows = (np.full(cap, -7, dtype=np.int32) for _ in range(3))
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    nt = C.c_int32(-1)
    rc = lib.ranenv_population_tiles(G, p(first), e0, n, rpe, *(p(a) if outs else None for a in (mem, row0, rows)), C.byref(nt))
    if rc != 0:
        return rc, None
    assert 0 <= nt.value < cap and np.all(mem[nt.value:] == -7)
    return rc, list(zip(mem[:nt.value].tolist(), row0[:nt.value].tolist(), rows[:nt.value].tolist()))


def _draw(rng):
    G = int(rng.choice([1, 2, 3, 7, 63, 64]))
    first = np.concatenate([[0], np.cumsum(rng.choice([1, 2, 5, 31, 32, 33, 70], size=G))])
    B = int(first[-1])
    e0 = int(rng.integers(0, B))
    n = int(rng.integers(1, B - e0 + 1))
    if rng.random() < 0.3:                 # a launch from a member's first env to a member's last
        a, b = sorted(rng.integers(0, G + 1, 2))
        if a < b:
            e0, n = int(first[a]), int(first[b] - first[a])
    return first.tolist(), e0, n, int(rng.choice([1, 3, 5, 10, 16]))


def test_the_librarys_tiles_are_the_restatements_and_partition_the_launch(lib):
    rng = np.random.default_rng(2024)
    cut = 0
    for _ in range(200):
        first, e0, n, rpe = _draw(rng)
        rc, got = _tiles(lib, first, e0, n, rpe)
        assert rc == 0 and got == pop.tiles(first, e0, n, rpe), (first, e0, n, rpe)
        cover = np.zeros(n * rpe, dtype=int)
        for m, row0, rows in got:
            assert 1 <= rows <= pop.NET_ROWS                                   # no tile is empty
            cover[row0:row0 + rows] += 1
            envs = e0 + np.arange(row0, row0 + rows) // rpe
            assert np.all(pop.owner(first, envs) == m), (first, e0, n, rpe, m)  # every row of the tile is its member's
        assert np.all(cover == 1)                                               # every row of the launch lies in exactly one tile
        members = [m for m, _, _ in got]
        assert members == sorted(members)                                       # member-major
        assert lib.ranenv_population_tiles(len(first) - 1, np.asarray(first, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32)), e0, n, rpe,
                                           None, None, None, C.byref(C.c_int32())) == 0
        cut += first.count(e0) == 0 or first.count(e0 + n) == 0
    assert cut > 50                                                             # launches that start or end inside a member


def test_the_cases_of_the_gpu_tests_have_the_tiles_they_are_built_around(lib):
    assert _tiles(lib, pop.FIRST_A, 0, 70, 1)[1] == [(0, 0, 5), (1, 5, 32), (2, 37, 32), (2, 69, 1)]
    assert _tiles(lib, pop.FIRST_A, 24, 24, 1)[1] == [(1, 0, 13), (2, 13, 11)]             # partition 1 of 3: envs 24..47
    assert _tiles(lib, pop.FIRST_A, 36, 34, 3)[1] == [(1, 0, 3), (2, 3, 32), (2, 35, 32), (2, 67, 32), (2, 99, 3)]     # range 1 of 2, intra rows
    rc, b = _tiles(lib, pop.FIRST_B, 0, 96, 3)
    assert len(b) == 64 and b[-1] == (63, 94 * 3, 6) and [r for _, _, r in b[:2]] == [3, 6]
    assert _tiles(lib, [0, 70], 0, 70, 1)[1] == [(0, 0, 32), (0, 32, 32), (0, 64, 6)]


def test_refused_tables_and_ranges(lib):
    from intent_radio_sched_multi_slice_amd.batched_env import population_first
    for first in ([0, 5, 5, 9], [0, 5, 4, 9], [1, 5, 9], [0]):
        assert _tiles(lib, first, 0, 1, 1)[0] == E_INVALID, first
    assert _tiles(lib, list(range(66)), 0, 1, 1)[0] == E_INVALID                # 65 members
    assert _tiles(lib, list(range(65)), 0, 64, 1)[0] == 0                       # 64 are fine
    nt = C.c_int32()
    assert lib.ranenv_population_tiles(0, (C.c_int32 * 1)(0), 0, 1, 1, None, None, None, C.byref(nt)) == E_INVALID      # no members, a pointer
    assert lib.ranenv_population_tiles(2, None, 0, 1, 1, None, None, None, C.byref(nt)) == E_INVALID
    for e0, n, rpe in ((-1, 2, 1), (0, 0, 1), (0, 10, 1), (5, 5, 1), (0, 9, 0)):
        assert _tiles(lib, [0, 4, 9], e0, n, rpe)[0] == E_INVALID, (e0, n, rpe)
    # the Python side's table: the same rules plus the batch, before any library call
    assert population_first(70, sizes=[5, 32, 33]).tolist() == pop.FIRST_A and population_first(70, pop.FIRST_A).dtype == np.int32
    for bad in ([0, 5, 5, 70], [0, 40, 37, 70], [1, 5, 70], [0, 5, 69], [0, 5, 71], [0], list(range(66))):
        with pytest.raises(ValueError):
            population_first(bad[-1] if bad in ([0], list(range(66))) else 70, bad)
    with pytest.raises(ValueError):
        population_first(70, sizes=[5, 0, 65])
    with pytest.raises(ValueError):
        population_first(70)


class _Stub:
    """BatchedRanEnv's list handling without a handle: S 3 / Us 4 on the CPU"""
    def __new__(cls, first):
        from intent_radio_sched_multi_slice_amd.batched_env import BatchedRanEnv
        env = object.__new__(BatchedRanEnv)
        env.S, env.Us, env.W, env.B, env.device = 3, 4, 17, first[-1], torch.device("cpu")
        env._population, env._intra_layout, env._keep, env._h, env._lib = np.asarray(first, dtype=np.int32), 0, {}, None, None
        return env


def test_lists_of_wrong_length_or_mixed_shape_raise_before_any_library_call():
    """(the stub has no library: a call that reached one would raise AttributeError, not ValueError)"""
    from tests.gpu_common import make_inter_net, make_net
    env = _Stub(pop.FIRST_A)
    inters, intras, v_inters, v_intras = pop.make_nets("a-S3-32", 5)
    with pytest.raises(ValueError, match="one per member is 3"):
        env.set_policy_network(inters[:2], intras[:2])
    with pytest.raises(ValueError, match="one per member is 3"):
        env.set_policy_network(inters, intras + intras[:1])
    with pytest.raises(ValueError, match="one per member is 3"):
        env.set_value_network(v_inters + v_inters, None)
    with pytest.raises(ValueError, match="a list of nets, one per member"):
        env.set_policy_network(inters, intras[0])
    with pytest.raises(ValueError, match="differs from net 0"):
        env.set_policy_network(inters[:2] + [make_inter_net(3, [24], "tanh", 1)], intras)
    with pytest.raises(ValueError, match="differs from net 0"):
        env.set_policy_network(inters, intras[:2] + [make_net([17, 32, 3], "relu", 1)])
    with pytest.raises(ValueError, match="differs from net 0"):
        env.set_value_network(v_inters, v_intras[:2] + [make_net([17, 32, 32, 1], "tanh", 1)])
    with pytest.raises(ValueError, match="precision"):
        env.set_policy_network(inters, intras, precision="fp8")
    with pytest.raises(ValueError, match="the other layout"):
        env.set_value_network(v_inters, [make_net([21, 32, 1], "tanh", m) for m in range(3)])
    for m in (-1, 3):
        with pytest.raises(ValueError, match="outside the population"):
            env.set_population_member(m, inter=inters[0])
    with pytest.raises(ValueError, match="input width"):
        env.set_population_member(1, intra=make_net([21, 32, 3], "tanh", 1))
    env._population = None
    with pytest.raises(ValueError, match="no population set"):
        env.set_policy_network(inters, intras)
    with pytest.raises(ValueError, match="no population set"):
        env.population_slices()
    assert [(s.start, s.stop) for s in _Stub(pop.FIRST_A).population_slices()] == [(0, 5), (5, 37), (37, 70)]


@pytest.fixture(scope="module")
def twins():
    """Per (twin net case, stochastic): snapshot, nets, the float64 reference -- computed once, shared, left unchanged."""
    out = {}
    for k, (name, seed) in enumerate(pop.TWIN_NETS):
        snap = pop.synthetic_snapshot(name, 60 + k)
        inters, intras, _, _ = pop.make_nets(name, seed)
        for st in MODES:
            out[name, st] = (snap, inters, intras, pop.policy_ref(snap, inters, intras, pop.CASES[name][2], st, SEED, pop.CASES[name][5]))
    return out


@pytest.mark.parametrize("slip", list(pop.SLIPS))
@pytest.mark.parametrize("stochastic", MODES)
@pytest.mark.parametrize("name", [n for n, _ in pop.TWIN_NETS])
def test_a_slipped_env_to_member_map_changes_the_twins_actions(twins, name, stochastic, slip):
    """Every moved env's net outputs leave the bounds, the others' actions stay, and the slipped twin's own actions, handed to check_actions as a
    device's, are refused."""
    snap, inters, intras, ref = twins[name, stochastic]
    first, layout = pop.CASES[name][2], pop.CASES[name][5]
    wrong = pop.policy_ref(snap, inters, intras, first, stochastic, SEED, layout, slip=slip)
    e = np.arange(first[-1])
    moved = pop.SLIPS[slip](first, e) != pop.owner(first, e)
    assert {"next": 70, "first": 65, "boundary": 2}[slip] == moved.sum()
    # (float64 GEMMs of other row counts: equal to rounding, not bit for bit)
    assert np.allclose(wrong.out[~moved], ref.out[~moved], rtol=0, atol=1e-12) and np.allclose(wrong.logits[~moved], ref.logits[~moved], rtol=0, atol=1e-12)
    for b in np.flatnonzero(moved):          # every moved env shows, in its scores and in a decidable intra choice or logit
        assert np.any(np.abs(wrong.out[b] - ref.out[b]) > ref.out_t[b] + wrong.out_t[b]), (slip, b)
        assert np.any(np.abs(wrong.logits[b] - ref.logits[b]) > ref.logit_bound[b] + wrong.logit_bound[b]), (slip, b)
    with pytest.raises(AssertionError, match="outside the bound|intra choices differ"):
        pr.check_actions(ref, wrong.scores, wrong.intra, min_safe=0.9)


def test_the_twin_decides_nine_rows_in_ten_for_every_net_the_gpu_tests_check():
    for n, (name, seed) in enumerate(pop.TWIN_NETS):
        inters, intras, _, _ = pop.make_nets(name, seed)
        S, Us, first, widths, act, layout = pop.CASES[name]
        for st in MODES:
            for draw in range(2):
                ref = pop.policy_ref(pop.synthetic_snapshot(name, 2000 + 10 * n + draw), inters, intras, first, st, SEED, layout)
                assert ref.intra_safe.mean() >= 0.9, (name, st, ref.intra_safe.mean())
                assert pr.check_actions(ref, ref.scores, ref.intra, min_safe=0.9) >= 0.9 * first[-1] * S


def test_copies_of_one_net_are_the_one_net_twin():
    name = "a-S5-48x40"
    S, Us, first, widths, act, layout = pop.CASES[name]
    inters, intras, _, _ = pop.make_nets(name, 9)
    snap = pop.synthetic_snapshot(name, 3)
    a = pop.policy_ref(snap, [inters[1]] * 3, [intras[1]] * 3, first, True, SEED, layout)
    b = pr.PolicyRef(snap["obs_inter"], snap["mask_inter"], pop.layers_of(inters[1]), snap["obs_intra"], snap["mask_intra"], pop.layers_of(intras[1]),
                     stochastic=True, seed=SEED, layout=layout, env_ids=np.arange(70), episode=snap["episode_number"], step=snap["step_number"])
    # (float64 GEMMs of other row counts: equal to rounding, not bit for bit)
    assert np.allclose(a.scores, b.scores, rtol=0, atol=1e-12) and np.allclose(a.logits, b.logits, rtol=0, atol=1e-12)
    assert np.array_equal(a.intra[b.intra_safe], b.intra[b.intra_safe]) and np.array_equal(a.active, b.active)


def test_population_means_is_np_mean_of_the_members_block():
    from intent_radio_sched_multi_slice_amd.batched_env import population_means
    rng = np.random.default_rng(11)
    res = {"reward": rng.standard_normal((70, 4)), "violations": rng.integers(0, 9, (70, 4)).astype(np.float64),
           "slice": rng.standard_normal((70, 4, 3, 10)), "scenario": rng.integers(0, 8, (70, 4)).astype(np.int32)}
    out = population_means(res, pop.FIRST_A)
    assert set(out) == {"reward", "violations", "slice"}
    for m, (lo, hi) in enumerate(zip(pop.FIRST_A[:-1], pop.FIRST_A[1:])):
        assert out["reward"][m] == np.mean(res["reward"][lo:hi]) and out["violations"][m] == np.mean(res["violations"][lo:hi])
        assert np.array_equal(out["slice"][m], np.mean(res["slice"][lo:hi], axis=(0, 1)))
    assert out["reward"].shape == (3,) and out["slice"].shape == (3, 3, 10)


def test_header_binding_and_library_agree_on_the_new_exports(lib):
    from intent_radio_sched_multi_slice_amd import _lib
    header = open(os.path.join(REPO, "include", "ranenv.h")).read()
    declared = set(re.findall(r"^int (ranenv_[a-z_]+)\s*\(", header, flags=re.M))
    for name in NEW_EXPORTS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
        proto = re.search(r"^int " + name + r"\(([^)]*)\)", header, flags=re.M).group(1)
        assert len(_lib.FUNCTIONS[name][1]) == len(proto.split(",")), name
    assert lib.ranenv_abi_version() == _lib.ABI_VERSION == 10 and "#define RANENV_ABI_VERSION 10" in header
