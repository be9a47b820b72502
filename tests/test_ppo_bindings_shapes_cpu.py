"""The grid of tests/ppo_bindings_shapes_ref.py without a GPU: the conditions its inputs must hold for the GPU modules' comparisons to
compare something -- no gradient tensor of the float64 twin is zero for any net of the grid (per slice for the per-slice cases), the
head cases' clip fraction lies strictly inside (0.1, 0.9) --, the per-slice cases' packed floats and LDS / wide-scratch figures and the
spread cases' ``ranenv_ppo_spread_bytes`` / ``ranenv_ppo_spread_plan`` answers against the formulas restated in the ref modules, what the
spread grid covers by its block counts, and two planted errors of the exact-reduce restatement -- a walk of tiles w, w + 1 and a
descending sum -- shown to change the expected gradient's bytes on a synthetic record through the float32 twin."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from intent_radio_sched_multi_slice_amd import _lib
from intent_radio_sched_multi_slice_amd import adapters as ad
from intent_radio_sched_multi_slice_amd import batched_env as be
from tests import ppo_bindings_shapes_ref as bs
from tests import ppo_head_ref as hd
from tests import ppo_head_shapes_ref as hg
from tests import ppo_spread_ref as sp
from tests import ppo_update_ref as ref
from tests import ppo_wide_ref as wd

ONE = dict(epochs=1, minibatch=ref.ALL, lr=0.0, grad_clip=0.0)
SPREAD_CASES = bs.SPREAD_SHAPES + (bs.LOPSIDED,) + bs.SPREAD_BEYOND + ("tanh40x24", "relu24")


def _no_zero_tensor(rec, kind, actor, critic, rows, act_a, act_c, layout, what):
    rows = torch.as_tensor(np.asarray(rows), dtype=torch.int64)
    assert rows.numel() >= 16, what
    t = ad.ppo_update_reference(rec, kind, ref.layers_of(actor), ref.layers_of(critic), rows[None, :], 0, rows.numel(), act_actor=act_a, act_critic=act_c,
                                layout=layout, **ONE)
    for net in ("actor", "critic"):
        for li, pair in enumerate(t["grad"][net]):
            for name, x in zip("Wb", pair):
                assert float(x.norm()) > 0.0, f"{what}: {kind} {net} layer {li} {name}: the twin's gradient is zero"


@pytest.mark.parametrize("case", bs.SLICE_SHAPES + bs.SLICE_BEYOND)
def test_no_gradient_tensor_of_the_twin_is_zero_for_any_slice_of_the_per_slice_cases(case):
    """Slice s's own pair on slice s's share of a synthetic record of the case's shape, and the inter pair on all rows"""
    S, Us, layout, (_, aa), (_, ca) = bs.slice_spec(case)
    nets = bs.slice_nets(case)
    rec = ref.synthetic_record(B=bs.SLICE_B, seed=11, T_=bs.SLICE_T, layout=layout, S=S, Us=Us)
    order = ad.ppo_row_order(rec, [0, bs.SLICE_B], 1, seed=3, per_slice=True)
    first, rows = order["first_intra"], order["order_intra"][0].numpy()
    _no_zero_tensor(rec, "inter", nets["inter"], nets["v_inter"], order["order_inter"][0].numpy(), aa, ca, layout, f"{case} inter")
    for s in range(S):
        _no_zero_tensor(rec, "intra", nets["intra"][s], nets["v_intra"][s], rows[first[s]:first[s + 1]], aa, ca, layout, f"{case} slice {s}")
    assert len({nets["intra"][s][0].weight.detach().numpy().tobytes() for s in range(S)}) == S, "the slices' nets are distinct"


@pytest.mark.parametrize("case", bs.SLICE_SPREAD_SHAPES + bs.SLICE_BEYOND)
def test_no_gradient_tensor_of_the_twin_is_zero_on_a_share_of_twenty_rows_at_24_steps(case):
    """The per-slice spread module's smallest share: tests/test_gpu_ppo_per_slice_spread_shapes.py gives 20 rows to the right neighbour of
    the slice with the most live rows, whichever that is on the device's record -- so every slice's own pair on 20 rows of its share of a
    synthetic record of T 24, and the inter pair on all 288 rows"""
    from tests import ppo_per_slice_spread_ref as ps
    S, Us, layout, (_, aa), (_, ca) = bs.slice_spec(case)
    nets = bs.slice_nets(case)
    rec = ref.synthetic_record(B=ps.B, seed=11, T_=ps.T, layout=layout, S=S, Us=Us)
    order = ad.ppo_row_order(rec, [0, ps.B], 1, seed=3, per_slice=True)
    first, rows = order["first_intra"], order["order_intra"][0].numpy()
    assert order["order_inter"].shape[1] == ps.B * ps.T == 288
    _no_zero_tensor(rec, "inter", nets["inter"], nets["v_inter"], order["order_inter"][0].numpy(), aa, ca, layout, f"{case} inter")
    for s in range(S):
        share = rows[first[s]:first[s + 1]]
        assert len(share) >= ps.SMALL, (case, s, len(share))
        _no_zero_tensor(rec, "intra", nets["intra"][s], nets["v_intra"][s], share[:ps.SMALL], aa, ca, layout, f"{case} slice {s}, 20 rows")
    assert len({nets["intra"][s][0].weight.detach().numpy().tobytes() for s in range(S)}) == S, "the slices' nets are distinct"


def test_what_the_per_slice_spread_grid_covers_by_its_block_counts():
    """One elementwise grid serves all units of a step, sized by the larger kind: the grid holds cases whose inter pair has more reduce /
    apply blocks than an intra pair, one the other way round (``intra_heavy``, why the grid has it), and an actor / critic boundary off
    the 1024-float block grid in both kinds; every case is named, so a case taken from the grid fails this"""
    cases = bs.SLICE_SPREAD_SHAPES + bs.SLICE_BEYOND
    claims = bs.slice_block_claims()
    print(claims)
    assert claims == bs.slice_block_claims(cases)
    assert claims["inter pair has more blocks"] == ["C", "F", "B"]
    assert claims["intra pair has more blocks"] == [bs.SLICE_LOPSIDED]
    assert claims["af off the block grid, inter"] == list(cases) == claims["af off the block grid, intra"] and len(cases) == 7
    assert not bs.slice_block_claims(bs.SLICE_SHAPES + bs.SLICE_BEYOND)["intra pair has more blocks"], "why the grid has the intra-heavy case"
    kf = bs.slice_kind_floats(bs.SLICE_LOPSIDED)
    assert bs.blocks_of(kf["inter"][1]) == bs.MIN_PAIR_BLOCKS == 5 and bs.blocks_of(kf["intra"][1]) == 40
    for case in cases:                           # (the counts are the library's own packed floats)
        for kind, (a, c) in bs.slice_dims(case).items():
            assert bs.slice_kind_floats(case)[kind] == (be.packed_net_floats(a), be.packed_net_floats(a) + be.packed_net_floats(c)), (case, kind)


@pytest.mark.parametrize("case", SPREAD_CASES)
def test_no_gradient_tensor_of_the_twin_is_zero_for_any_net_of_the_spread_cases(case):
    S, Us, layout, aa, ca, _ = bs.spread_spec(case)
    nets = bs.spread_nets(case)
    rec = ref.synthetic_record(B=bs.SPREAD_B, seed=11, T_=bs.SPREAD_T, layout=layout, S=S, Us=Us)
    order = ad.ppo_row_order(rec, [0, bs.SPREAD_B], 1, seed=3)
    for kind in ("inter", "intra"):
        _no_zero_tensor(rec, kind, nets[kind], nets["v_" + kind], order["order_" + kind][0].numpy(), aa, ca, layout, f"{case}")


@pytest.mark.parametrize("name", bs.HEAD_CASES)
def test_the_head_cases_clip_fraction_lies_strictly_inside(name):
    """On the 96 synthetic rows of every case of ppo_head_shapes_ref.CASES (hd.ratios asserts that no tensor of the twin is zero)"""
    case, lay, rec = hg.CASES[name], hg.layers(name), hg.synthetic_record(name)
    t64 = hd.twin(case, rec, hd.row_order(1), lay, **ONE, **hd.HP)
    t32 = hd.twin(case, rec, hd.row_order(1), lay, dtype=torch.float32, **ONE, **hd.HP)
    hd.ratios(hd.tensors(t32["grad"]), hd.tensors(t64["grad"]), hd.tensors(t32["grad"]))
    assert 0.1 < t64["clip_fracs"][0] < 0.9, t64["clip_fracs"]
    assert 0.1 < t64["stats"][0, 4] < 0.9


@pytest.mark.parametrize("case", bs.SLICE_SHAPES + bs.SLICE_BEYOND)
def test_per_slice_packed_floats_and_lds_figures_against_the_restated_formulas(case):
    S, Us, layout, (aw, _), (cw, _) = bs.slice_spec(case)
    nets, dims = bs.slice_nets(case), bs.slice_dims(case)
    for kind, (a, c) in dims.items():
        for role, d in ((kind, a), ("v_" + kind, c)):
            net = nets[role][0] if kind == "intra" else nets[role]
            assert be.packed_net_floats(ref.layers_of(net)) == be.packed_net_floats(d) == sp.packed_floats(d), (case, role)
        assert be.ppo_lds_bytes(a, c, wide=True) == wd.wide_lds_bytes(a, c) <= wd.WIDE_LDS_MAX, (case, kind)
        assert be.ppo_wide_scratch_floats(a, c) == wd.wide_scratch_floats(a, c), (case, kind)
    plain = max(be.ppo_lds_bytes(a, c) for a, c in dims.values())
    assert plain == ref.lds_bytes(S, Us, layout, aw, cw)
    assert (plain <= ref.LDS_MAX) == (case in bs.SLICE_SHAPES), "the plain-plan cases fit the LDS plan, the others do not"
    assert {bs.slice_spec(c)[0] for c in bs.SLICE_SHAPES} >= {1, 16}, "S 1 and S 16 per slice"


def _lib_plan(lib, n_rows, minibatch, epochs, slabs):
    steps, grid, tail = C.c_int64(-7), C.c_int32(-7), C.c_int32(-7)
    assert lib.ranenv_ppo_spread_plan(n_rows, minibatch, epochs, slabs, C.byref(steps), C.byref(grid), C.byref(tail)) == 0
    return steps.value, grid.value, tail.value


def test_spread_bytes_and_plans_of_the_grid_against_the_restated_formulas():
    """Every spread case's pairs at the slab counts the GPU module binds, plain and wide; and the schedules it runs: the 33- and 65-row
    cuts at one slab, all rows at three, the exact reduce's 128 and 256 rows at four slabs (one and two tiles per slab), the loop of the
    one-kind-alone test, and the 16 896 rows under 256 slabs as one minibatch (grid 256, 528 tiles) and as two of 8448 (264 tiles each)"""
    lib = _lib.load()
    for case in SPREAD_CASES:
        for kind, (a, c) in bs.spread_spec(case)[5].items():
            for slabs in (1, 3, bs.EXACT_SLABS, 5, sp.SLABS_MAX):
                for wide in (False, True):
                    assert be.ppo_spread_bytes(a, c, slabs, wide) == sp.spread_bytes(a, c, slabs, wide), (case, kind, slabs, wide)
    n_all = bs.ALL_SLABS_B * bs.ALL_SLABS_T
    for n_rows, minibatch, epochs, slabs in ((33, ref.ALL, 1, 1), (65, ref.ALL, 1, 1), (96, ref.ALL, 1, 3), (128, ref.ALL, 1, 4), (256, ref.ALL, 1, 4),
                                             (96, 40, 2, 3), (n_all, ref.ALL, 1, sp.SLABS_MAX), (n_all, bs.ALL_SLABS_MB, 1, sp.SLABS_MAX)):
        assert _lib_plan(lib, n_rows, minibatch, epochs, slabs) == sp.plan(n_rows, minibatch, epochs, slabs), (n_rows, minibatch, epochs, slabs)
    assert _lib_plan(lib, n_all, ref.ALL, 1, sp.SLABS_MAX) == (1, 256, 528) and n_all == 2 * bs.ALL_SLABS_MB
    assert _lib_plan(lib, n_all, bs.ALL_SLABS_MB, 1, sp.SLABS_MAX) == (2, 256, 264), "two minibatches, each on all 256 slabs"
    assert [len(t) for t in sp.walk(128, 4)] == [1] * 4 and sp.walk(256, 4) == [[w, w + 4] for w in range(4)]
    assert {len(t) for t in sp.walk(n_all, sp.SLABS_MAX)} == {2, 3} and {len(t) for t in sp.walk(bs.ALL_SLABS_MB, sp.SLABS_MAX)} == {1, 2}


def test_what_the_spread_grid_covers_by_its_block_counts():
    """No kind has one reduce / apply block (a padded layer is 1056 floats): a pair has at least 5.  The grid holds a kind with those 5, a kind
    with more than 256 (shape A), a case whose kinds differ by more than 10x and an actor / critic boundary off the block grid."""
    assert sp.packed_floats([1, 1, 1]) == 2 * 1056 > 2 * bs.SPREAD_BLOCK and bs.blocks_of(2 * sp.packed_floats([1, 1, 1])) == bs.MIN_PAIR_BLOCKS
    claims = bs.block_claims()
    print(claims)
    assert (bs.LOPSIDED, "intra") in claims["fewest blocks"]
    assert ("A", "inter") in claims["more than 256 blocks"] and ("A", "intra") in claims["more than 256 blocks"]
    assert bs.LOPSIDED in claims["kinds differ by more than 10x"]
    assert claims["af off the block grid"]
    assert not bs.block_claims(bs.SPREAD_SHAPES)["kinds differ by more than 10x"], "why the grid has the lopsided case"


def _flat(t):
    return np.concatenate([x.numpy().astype(np.float32).reshape(-1) for net in ("actor", "critic") for pair in t["grad"][net] for x in pair])


@pytest.mark.parametrize("kind", ["inter", "intra"])
def test_planted_errors_of_the_walk_and_of_the_reduce_change_the_expected_bytes(kind):
    """The exact-reduce test of tests/test_gpu_ppo_spread_shapes.py expects ((g_0 / 4 + g_1 / 4) + g_2 / 4) + g_3 / 4 with g_w the plain
    binding's gradient of slab w's rows in walk order.  Here g_w comes from the float32 twin on a synthetic record: the restatement with
    tiles w, w + 1 in place of w, w + 4 (256 rows, 4 slabs) and the one summed in descending order (128 and 256 rows) each give other
    bytes than the right one, so the device test's byte equality tells them apart."""
    case = "tanh40x24"
    widths, act, layout = ref.CASES[case]
    nets = sp.one_agent_nets(case)
    rec = ref.synthetic_record(B=bs.SPREAD_B, seed=13, T_=bs.EXACT_T, layout=layout)
    order = ad.ppo_row_order(rec, [0, bs.SPREAD_B], 1, seed=3)
    row = order["order_" + kind][0].numpy()
    assert len(row) >= 256

    def expected(rows, slip_walk=None, slip_sum=None):
        parts = []
        for share in bs.slab_rows(row[:rows], rows, bs.EXACT_SLABS, slip_walk):
            r = torch.as_tensor(share, dtype=torch.int64)
            parts.append(_flat(ad.ppo_update_reference(rec, kind, ref.layers_of(nets[kind]), ref.layers_of(nets["v_" + kind]), r[None, :], 0, r.numel(),
                                                       act_actor=act, act_critic=act, layout=layout, dtype=torch.float32, adv_norm=False, **ONE)))
        return bs.reduce_f32(parts, bs.EXACT_SLABS, slip_sum)

    for rows in (128, 256):
        right = expected(rows)
        assert right.any() and right.tobytes() == expected(rows).tobytes()
        assert right.tobytes() != expected(rows, slip_sum="descending").tobytes(), f"{rows} rows: a descending sum gives the same bytes"
    assert expected(256).tobytes() != expected(256, slip_walk="neighbour tiles").tobytes(), "a walk of tiles w, w + 1 gives the same bytes"
    shares = bs.slab_rows(row[:256], 256, bs.EXACT_SLABS)
    assert all(len(s) == 64 for s in shares) and np.array_equal(np.sort(np.concatenate(shares)), np.sort(row[:256]))
    assert np.array_equal(shares[1], np.concatenate([row[32:64], row[160:192]]))
