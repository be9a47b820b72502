"""The row lists on the device, without a GPU: the keyed permutation of include/ranenv.h "Row lists on the device" at its pinned
values, as a permutation at every size class, and as a shuffle; the numpy twin ``adapters.ppo_row_order_reference`` against the
plain-Python restatement of tests/ppo_row_order_ref.py and against ``adapters.ppo_row_order``'s tables and row sets; the planted
slips of the twin against the comparison and the cases of tests/test_gpu_ppo_row_order.py; the exports and the new kernels'
resources.  Every comparison is exact."""
from __future__ import annotations

import ctypes
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from intent_radio_sched_multi_slice_amd import adapters
from intent_radio_sched_multi_slice_amd.adapters import ppo_row_order_reference, ppo_row_permutation
from tests import ppo_row_order_ref as rr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
NEW_EXPORTS = ("ranenv_ppo_row_count", "ranenv_ppo_row_order")
BIG_N = 2_000_003


# ---- the permutation ------------------------------------------------------------------------------------------------------------------
def test_pinned_values():
    """The values of the issue's prototype, from the twin and from the plain restatement"""
    for P in (lambda *a: ppo_row_permutation(*a).tolist(), rr.permutation):
        assert P(10, 7, 0, 0, 0) == [5, 3, 2, 7, 0, 6, 8, 9, 1, 4]
        assert P(2, 1, 0, 0, 0) == [1, 0]
        assert P(3, 1, 0, 0, 1) == [0, 2, 1]
        p = P(33, 2 ** 33 + 5, 2, 3, 1)
        assert p[:8] == [9, 7, 11, 20, 23, 16, 27, 21] and p[-1] == 30
    p = ppo_row_permutation(262144, 12345, 3, 0, 0)
    assert p[:6].tolist() == [116701, 214248, 103782, 199985, 97171, 219702]
    assert int((np.arange(262144, dtype=np.int64) * p % 1000003).sum() % 1000003) == 20841
    assert ppo_row_permutation(1, 9, 4, 2, 1).tolist() == [0] and ppo_row_permutation(0, 9, 4, 2, 1).size == 0
    assert adapters.ROWS_TAG == int.from_bytes(b"SHUF", "big") == rr.TAG


_BIG = {}


def _big(epoch):
    if epoch not in _BIG:
        _BIG[epoch] = ppo_row_permutation(BIG_N, 77, epoch, 1, 1)
    return _BIG[epoch]


@pytest.mark.parametrize("n", list(range(1, 80)) + [96, 264, 1000, 2048, 4097, 65536, 262144, BIG_N])
def test_a_permutation_at_every_size(n):
    """n = 1 .. 79 (every half-width h up to 4, n at, below and above the powers of two and of four) and the larger sizes, three
    epochs each: every value of [0, n) exactly once.  Up to 4097 the plain restatement gives the same list and counts the walk: no
    position took more than 64 passes (a pass leaves the excess with probability below 3/4; the issue's prototype met 36 at most)."""
    for epoch in range(3):
        p = _big(epoch) if n == BIG_N else ppo_row_permutation(n, 77, epoch, 1, 1)
        assert p.dtype == np.int64 and p.shape == (n,)
        assert np.array_equal(np.sort(p), np.arange(n)), (n, epoch)
        if n <= 4097:
            passes = []
            assert rr.permutation(n, 77, epoch, 1, 1, passes) == p.tolist(), (n, epoch)
            assert max(passes, default=1) <= 64, (n, epoch, max(passes))


def test_two_epochs_of_a_large_unit_share_next_to_nothing():
    agree = int((_big(0) == _big(1)).sum())
    print(f"n = {BIG_N}: epochs 0 and 1 agree in {agree} positions")
    assert agree < 10


@pytest.mark.parametrize("n", [33, 264])
def test_the_shuffle_looks_uniform(n):
    """4000 draws with seed 1000 + s, epoch s % 5, unit s % 3, kind s % 2: the mean fixed points per permutation in [0.9, 1.1], the
    mean successions P(i + 1) == P(i) + 1 in [0.85, 1.1], the position-by-value chi-square over (n - 1)^2 below 1.2 (a uniform
    shuffle: 1, about 1, 1; the issue's prototype: 1.009 / 0.968 / 1.106 at n 33, 1.012 / 1.014 / 1.006 at n 264)."""
    draws = 4000
    counts = np.zeros((n, n), dtype=np.int64)
    fixed = succ = 0
    pos = np.arange(n)
    for s in range(draws):
        p = ppo_row_permutation(n, 1000 + s, s % 5, s % 3, s % 2)
        fixed += int((p == pos).sum())
        succ += int((p[1:] == p[:-1] + 1).sum())
        counts[pos, p] += 1
    expect = draws / n
    chi = float(((counts - expect) ** 2 / expect).sum()) / (n - 1) ** 2
    print(f"n = {n}: fixed points {fixed / draws:.3f}, successions {succ / draws:.3f}, chi-square / (n - 1)^2 {chi:.3f}")
    assert 0.9 <= fixed / draws <= 1.1
    assert 0.85 <= succ / draws <= 1.1
    assert chi < 1.2


# ---- the twin -------------------------------------------------------------------------------------------------------------------------
def _seeded_case(i):
    """Mask i of 200: T 1..5, B 1..9, S 1..5, a random cut of B into members, both groupings (slices: one member), Bernoulli masks of
    varying density with now and then a dead slice or a dead member"""
    rng = np.random.default_rng(5000 + i)
    T, B, S = int(rng.integers(1, 6)), int(rng.integers(1, 10)), int(rng.integers(1, 6))
    per_slice = i % 3 == 2
    G = 1 if per_slice else int(rng.integers(1, B + 1))
    first = [0] + sorted(rng.choice(np.arange(1, B), size=G - 1, replace=False).tolist()) + [B] if G > 1 else [0, B]
    mask = (rng.random((T, B, S)) < rng.choice([0.1, 0.5, 0.9])).astype(np.int8) * int(rng.integers(1, 4))
    if i % 7 == 3:
        mask[:, :, int(rng.integers(0, S))] = 0
    if i % 11 == 5:
        mask[:, first[0]:first[1], :] = 0
    return mask, first, per_slice, int(rng.integers(1, 4)), int(rng.integers(0, 2 ** 63))


def test_the_twin_against_the_plain_restatement_and_the_torch_path():
    """200 seeded masks: the twin's lists and tables equal the plain restatement's; every epoch's slice of unit u is a permutation of
    u's base list; the tables equal ``adapters.ppo_row_order``'s for the same record, and each list sorted per unit equals that
    function's list sorted per unit."""
    seen_empty = seen_slices = seen_members = 0
    for i in range(200):
        mask, first, per_slice, epochs, seed = _seeded_case(i)
        twin = ppo_row_order_reference(mask, first, epochs, seed, per_slice=per_slice)
        lists, firsts, bases = rr.row_order(mask.tolist(), first, epochs, seed, rr.SLICES if per_slice else rr.MEMBERS)
        theirs = adapters.ppo_row_order({"mask_inter": torch.from_numpy(mask)}, first, epochs, seed=i, per_slice=per_slice)
        for kind in ("inter", "intra"):
            o, f = twin["order_" + kind], twin["first_" + kind]
            assert o.dtype == np.int32 and f.dtype == np.int32 and o.shape == (epochs, firsts[kind][-1])
            assert f.tolist() == firsts[kind], (i, kind)
            assert o.tolist() == lists[kind], (i, kind)
            assert np.array_equal(f, theirs["first_" + kind]), (i, kind)
            t = theirs["order_" + kind].numpy()
            for u, base in enumerate(bases[kind]):
                seen_empty += not base
                for k in range(epochs):
                    assert sorted(o[k, f[u]:f[u + 1]].tolist()) == base == sorted(t[k, f[u]:f[u + 1]].tolist()), (i, kind, u, k)
        seen_slices += per_slice
        seen_members += len(first) > 2
    assert seen_empty > 10 and seen_slices > 50 and seen_members > 50
    inter_only = ppo_row_order_reference((3, 4, 2), [0, 1, 4], 2, 9, intra=False)
    assert inter_only["order_intra"] is None and inter_only["first_intra"] is None
    assert rr.same(inter_only, ppo_row_order_reference(np.ones((3, 4, 2), dtype=np.int8), [0, 1, 4], 2, 9, intra=False)) is None
    with pytest.raises(ValueError):
        ppo_row_order_reference((3, 4, 2), [0, 4], 2, 9)
    with pytest.raises(ValueError):
        ppo_row_order_reference(np.ones((3, 4, 2), dtype=np.int8), [0, 1, 4], 2, 9, per_slice=True)
    with pytest.raises(ValueError):
        ppo_row_order_reference(np.ones((3, 4, 2), dtype=np.int8), [0, 4], 2, 9, slip="unknown")


_TWINS = {}


def _twin_of(case):
    name, T, mask, pop, per_slice, epochs, seed = case
    if name not in _TWINS:
        _TWINS[name] = ppo_row_order_reference(rr.make_mask(mask, T), rr.POPULATIONS[pop], epochs, seed, per_slice=per_slice)
    return _TWINS[name]


@pytest.mark.parametrize("slip", adapters.PPO_ROW_SLIPS)
def test_every_planted_slip_fails_the_gpu_tests_comparison(slip):
    """A twin with one planted mistake differs from the true twin, under ``ppo_row_order_ref.same``, on at least one case of the GPU
    test -- and a slip that concerns one grouping alone is caught by a case of that grouping."""
    caught = []
    for case in rr.cases():
        name, T, mask, pop, per_slice, epochs, seed = case
        if T > 8 and caught:
            continue
        got = ppo_row_order_reference(rr.make_mask(mask, T), rr.POPULATIONS[pop], epochs, seed, per_slice=per_slice, slip=slip)
        if rr.same(got, _twin_of(case)) is not None:
            caught.append(case)
    print(f"{slip}: caught by {len(caught)} of {len(rr.cases())} cases, first {caught[0][0] if caught else None}")
    assert caught
    if slip == "slice_div":
        assert all(c[4] for c in caught)
    if slip == "member_shift":
        assert all(not c[4] and c[3] != "one" for c in caught)
    if slip == "no_epoch":
        assert all(c[5] > 1 for c in caught)


def test_the_gpu_cases_cover_what_the_issue_names():
    cases = rr.cases()
    assert len({c[0] for c in cases}) == len(cases)
    for T in (1, 8):
        for mask in rr.MASKS:
            for pop in rr.POPULATIONS:
                assert any(c[1] == T and c[2] == mask and c[3] == pop and not c[4] for c in cases)
            assert any(c[1] == T and c[2] == mask and c[4] for c in cases)
    for per_slice in (False, True):
        assert {c[5] for c in cases if c[4] == per_slice} == {1, 3} and {c[6] for c in cases if c[4] == per_slice} == set(rr.SEEDS)
    assert rr.T_SHORT * rr.B * rr.S == 8 * rr.CHUNK - 4 and rr.T_PAST * rr.B * rr.S == 7 * rr.CHUNK + 4
    assert rr.T_RUN_PAST * rr.B == rr.CHUNK + 4 and rr.T_RUN_SHORT * rr.B == 2 * rr.CHUNK - 4
    assert (rr.B * rr.S) % 4 == 0           # ... so no T lands nearer than 4 cells to a multiple of the chunk
    sizes = np.diff(rr.BIG["first_env"]) * rr.BIG["S"]
    assert sizes.tolist() == [rr.CHUNK - 3, rr.CHUNK + 2, 50]
    src = open(os.path.join(REPO, "intent_radio_sched_multi_slice_amd", "csrc", "ranenv_internal.h")).read()
    assert f"enum {{ ROWS_CHUNK = {rr.CHUNK} }};" in src
    # the high word of the seed matters
    a, b = ppo_row_permutation(264, 5, 0, 0, 0), ppo_row_permutation(264, 2 ** 33 + 5, 0, 0, 0)
    assert not np.array_equal(a, b)


# ---- the exports and the kernels ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.csrc import build
    build.build()
    return _lib.load()


def test_header_binding_and_library_agree_on_the_new_exports(lib):
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.csrc import build
    header = open(os.path.join(REPO, "include", "ranenv.h")).read()
    declared = set(re.findall(r"^int (ranenv_[a-z_]+)\s*\(", header, flags=re.M))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_EXPORTS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name) and hasattr(raw, name), name
        proto = re.search(r"^int " + name + r"\(([^)]*)\)", header, flags=re.M).group(1)
        assert len(_lib.FUNCTIONS[name][1]) == len(proto.split(",")), name
    assert [len(_lib.FUNCTIONS[n][1]) for n in NEW_EXPORTS] == [7, 9]
    assert "#define RANENV_PPO_ROWS_MEMBERS 0" in header and re.search(r"#define RANENV_PPO_ROWS_SLICES +1", header)
    assert (_lib.PPO_ROWS_MEMBERS, _lib.PPO_ROWS_SLICES) == (adapters.PPO_ROWS_MEMBERS, adapters.PPO_ROWS_SLICES) == (rr.MEMBERS, rr.SLICES) == (0, 1)
    assert "0x53485546" in header
    assert "ranenv_rows.hip" in build.SOURCES and any(u[1] == "ranenv_rows.hip" for u in build.UNITS)
    first = (ctypes.c_int32 * 65)()
    assert lib.ranenv_ppo_row_count(None, 1, None, 0, first, first, None) == E_INVALID
    assert lib.ranenv_ppo_row_order(None, 1, None, 0, 1, 0, None, None, None) == E_INVALID


def test_the_new_kernels_have_no_scratch_and_no_spills(lib):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_resources
    ks = [k for k in kernel_resources.kernel_resources() if "ranenv_rows_" in k["name"]]
    assert sorted(k["name"].split("(")[0] for k in ks) == ["ranenv_rows_compact_kernel", "ranenv_rows_count_kernel", "ranenv_rows_scan_kernel",
                                                           "ranenv_rows_shuffle_kernel"]
    for k in ks:
        assert k.get("private_segment_fixed_size", 0) == 0 and k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, k
        assert k.get("agpr_count", 0) == 0 and k["max_flat_workgroup_size"] == 256, k


def test_order_takes_device_and_no_other_string():
    from intent_radio_sched_multi_slice_amd.batched_env import BatchedRanEnv
    assert BatchedRanEnv._device_order("device") is True
    assert BatchedRanEnv._device_order(None) is False and BatchedRanEnv._device_order({"order_inter": None}) is False
    with pytest.raises(ValueError):
        BatchedRanEnv._device_order("torch")
    for method in ("ppo_row_order", "ppo_head_row_order"):
        assert callable(getattr(BatchedRanEnv, method))
