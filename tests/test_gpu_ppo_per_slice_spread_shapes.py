"""The per-slice spread PPO update (ranenv_ppo_bind_slices_spread; the kernels ranenv_ppo_spread_slices_pass_kernel, _pass_kernel_wide,
_reduce_kernel and _apply_kernel) across slice counts, net shapes and slab counts -- what tests/test_gpu_ppo_per_slice_spread.py checks
at S 3 and three narrow nets, here on the per-slice grid of tests/ppo_bindings_shapes_ref.py (``bs``): S 1 (two units), S 10, S 13 and
S 16 (17 units, ``mem`` up to 15 in every per-unit stride), actors and critics that differ in depth, both intra layouts, a 7-wide
bottleneck, two nets beyond the LDS plan at S 2 under ``wide=True``, and ``intra_heavy`` (S 3), the one case whose intra pairs have more
reduce / apply blocks than the inter pair (``bs.slice_block_claims``).

The figures are tests/ppo_per_slice_spread_ref.py's (``ps``), not the per-slice grid's own T 8 / minibatch 12 (one tile, where the slab
count could never matter): B 12, T 24 (288 inter rows), minibatch 72 = two full tiles and one of 8 rows, 2 epochs, S distinct pairs from
``bs.slice_nets``, the workload ``shaped_workload(S, Us, 12, seed=71)``.  ``bs.slice_order`` gives the slice with the most live rows
MID = 100 rows, its right neighbour SMALL = 20 and every other slice all its live rows; S 1 has one slice: 20 rows in the twin test, 100 in
the bit-for-bit test.  At T 24 every case's record gives its fullest slice 100 live rows and every other slice 32 (8 of the 12 envs play
scenarios with every slice active: 192 live cells per slice at least; ``bs.slice_order`` asserts it), so no case raises T (``T_OF``).

Comparisons and tolerances are tests/ppo_update_ref.py's: the gradient per layer tensor within 8x the float32-torch error of the float64
twin (floor 1e-6 relative) and strictly above 0, statistics 1e-6, Adam 4 float32 ulp of adam_step_f32 on the call's own dev_grad, byte
equality against a handle bound to ONE shared pair under ``ppo_bind(spread=True, slabs=N[, wide=True])`` and against the per-slice binding
at one slab.

The slab invariance at the stride's far end runs on case B (S 13): ``ranenv_ppo_slices_spread_bytes`` at 256 slabs is 433.0 MiB there;
case C (S 16), whose intra pair has the fewest packed floats of the cases with more than one slice (30 112 against B's 30 208), needs
520.9 MiB, beyond the 512 MiB the test allows itself.

Measured on one MI355X (printed by the tests):
    worst tensor's error / float32 twin's over the inter pair and every slice at 3 slabs (bound 8): D 0.306, C 0.755, F 0.949, B 0.929,
    intra_heavy 0.644; beyond the plan under per_slice + spread + wide: verybig 1.38, past_limit 0.752; the five statistics within
    1.4e-7 of the twin (bound 1e-6)
    one Adam step (weights / moments): 0 / 0 ulp on every slice of all seven cases"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from intent_radio_sched_multi_slice_amd import batched_env as be
from tests import ppo_bindings_shapes_ref as bs
from tests import ppo_per_slice_spread_ref as ps
from tests import ppo_spread_ref as sp
from tests import ppo_update_ref as ref
from tests.gpu_common import need_gpu, shaped_workload

pytestmark = pytest.mark.gpu

E_STATE = -3
B, MB, SMALL, MID, EPOCHS = ps.B, ps.MB, ps.SMALL, ps.MID, ps.EPOCHS
ALL = ref.ALL
HP = dict(lr=2e-3, clip=0.2, vf_coeff=0.5, ent_coeff=0.01, grad_clip=0.5)
STAT_NAMES = bs.STAT_NAMES
PLAIN, BEYOND = bs.SLICE_SPREAD_SHAPES, bs.SLICE_BEYOND
CASES = PLAIN + BEYOND
T_OF = {}                                # case -> T where ps.T = 24 does not give the shares their rows: none does
FAR_END_CAP = 512 << 20                  # bytes of slabs the far-end test allows itself at 256 slabs


def _T(case):
    return T_OF.get(case, ps.T)


def _wide(case):
    return dict(wide=True) if case in BEYOND else {}


def _spread(case, slabs):
    return dict(per_slice=True, spread=True, slabs=slabs, **_wide(case))


def _workload(case):
    need_gpu()
    S, Us = bs.slice_spec(case)[:2]
    return shaped_workload(S, Us, B, seed=71).env


def _set_nets(env, case, s=None):
    """The case's S distinct pairs (s None) or ONE shared intra pair, slice s's"""
    nets = bs.slice_nets(case)
    intra, v_intra = (nets["intra"], nets["v_intra"]) if s is None else (nets["intra"][s], nets["v_intra"][s])
    env.set_policy_network(nets["inter"], intra, stochastic=True, seed=ref.SEED, intra_input=bs.slice_spec(case)[2])
    env.set_value_network(nets["v_inter"], v_intra)


def _env(case, bind):
    """A reset env of the case's shape under its S distinct pairs, bound with ``ppo_bind(**bind)``"""
    env = _workload(case)
    _set_nets(env, case)
    env.ppo_bind(**bind)
    env.reset()
    return env


def _shared_env(case, s, **bind):
    """A reset env under ONE shared intra pair, slice s's nets, bound with ``ppo_bind(**bind)``"""
    env = _workload(case)
    _set_nets(env, case, s)
    env.ppo_bind(**bind)
    env.reset()
    return env


def _record(env, case):
    rec = env.collect(_T(case))
    torch.cuda.synchronize()
    assert rec["mask_inter"].shape == (_T(case), B, env.S)
    return rec


def _twin_records(env_a, env_b, case):
    rec_a, rec_b = _record(env_a, case), _record(env_b, case)
    for k in rec_a:
        assert torch.equal(rec_a[k], rec_b[k]), k
    return rec_a, rec_b


def _order(rec, epochs, only, empty=None):
    return bs.slice_order(rec, epochs, MB, SMALL, MID, empty, only=only)


def _checked(case):
    """The slices held against a shared handle: 0, 1, S // 2 and S - 1 (all where S <= 4)"""
    S = bs.slice_spec(case)[0]
    return sorted({0, min(1, S - 1), S // 2, S - 1})


def _states(env):
    return [bs.slice_state(env, s) for s in range(env.S)], bs.slice_state(env, None)


def _same_out(a, b, what, units=None):
    for u in range(a["rows"].shape[0]) if units is None else units:
        (sa, ga), (sb, gb) = bs.wg_row(a, u), bs.wg_row(b, u)
        assert sa.tobytes() == sb.tobytes(), f"{what}: statistics of unit {u}"
        assert ga.tobytes() == gb.tobytes(), f"{what}: last gradient of unit {u}"


def _same_run(a, b, what):
    """Two runs of a case: every unit's state, statistics and last gradient byte for byte"""
    assert a["counts"] == b["counts"]
    ref.same_state(a["inter"], b["inter"], f"{what} inter")
    for s in range(len(a["slices"])):
        ref.same_state(a["slices"][s], b["slices"][s], f"{what} slice {s}")
    _same_out(a["out"], b["out"], what)


# ---- the lists of the "who finishes first" runs ----------------------------------------------------------------------------------------------
def _cut_inter(order, n):
    """The call's lists with the inter list cut to its first n rows"""
    return dict(order, order_inter=order["order_inter"][:, :n].contiguous(), first_inter=np.array([0, n], dtype=np.int32))


def _no_intra(order):
    return {k: v for k, v in order.items() if not k.endswith("_intra")}


VARIANTS = {None: lambda o: o, "inter 20": lambda o: _cut_inter(o, SMALL), "inter 0": lambda o: _cut_inter(o, 0), "no intra": _no_intra}

_RUNS = {}


def _run(case, slabs, empty=None, variant=None, calls=1):
    """2 epochs x minibatches of 72 on a stochastic record under this binding (``calls`` times in a row), computed once"""
    key = (case, slabs, empty, variant, calls)
    if key not in _RUNS:
        S = bs.slice_spec(case)[0]
        env = _env(case, _spread(case, slabs))
        rec = _record(env, case)
        order, counts = _order(rec, EPOCHS, MID, empty)
        order = VARIANTS[variant](order)
        start, start_inter = _states(env)
        for _ in range(calls):
            out = env.ppo_update_per_slice(rec, epochs=EPOCHS, minibatch=MB, order=order, grad=True, **HP)
        slices, inter = _states(env)
        assert out["rows"].shape[0] == 1 + S and len(slices) == S
        _RUNS[key] = dict(rec=rec, order=order, counts=counts, out=out, start=start, start_inter=start_inter, slices=slices, inter=inter)
        env.close()
    return _RUNS[key]


def _against_shared_handles(case, run, slices, slabs, inter_rows=None, calls=1):
    """Slice s's weights, moments, counter, statistics and last gradient equal, byte for byte, those of a handle bound to the shared pair
    (net s) under ``ppo_bind(spread=True, slabs=N[, wide=True])`` and updated on the same record with an intra list of slice s's share; the
    inter pair equals that handle's inter kind; the counters read 2 x ceil(rows / 72)"""
    T = _T(case)
    inter_rows = T * B if inter_rows is None else inter_rows
    for n, s in enumerate(slices):
        shared = _shared_env(case, s, spread=True, slabs=slabs, **_wide(case))
        for _ in range(calls):
            o = shared.ppo_update(run["rec"], epochs=EPOCHS, minibatch=MB, order=bs.share(run["order"], s), grad=True, **HP)
        what = f"{case}, {slabs} slabs, slice {s}"
        ref.same_state(run["slices"][s], bs.plain_state(shared, 1), what)
        stats, grad = bs.wg_row(run["out"], 1 + s)
        assert stats.tobytes() == np.stack([o[name][0, 1] for name in STAT_NAMES], axis=-1).tobytes(), f"{what}: statistics"
        assert grad.tobytes() == o["grad"][0, 1].cpu().numpy().tobytes() and grad.any(), f"{what}: last gradient"
        steps = EPOCHS * -(-run["counts"][s] // MB)
        assert int(run["slices"][s]["intra/t"][0]) == int(run["slices"][s]["v_intra/t"][0]) == calls * steps > 0, what
        assert np.all(run["out"]["minibatches"][1 + s] == steps // EPOCHS) and np.all(run["out"]["rows"][1 + s] == run["counts"][s])
        if n == 0:
            ref.same_state(run["inter"], bs.plain_state(shared, 0), f"{case}, {slabs} slabs, inter pair")
            stats, grad = bs.wg_row(run["out"], 0)
            assert stats.tobytes() == np.stack([o[name][0, 0] for name in STAT_NAMES], axis=-1).tobytes(), f"{case}: inter statistics"
            assert grad.tobytes() == o["grad"][0, 0].cpu().numpy().tobytes() and grad.any() == (inter_rows > 0), f"{case}: inter gradient"
        shared.close()
    assert int(run["inter"]["inter/t"][0]) == int(run["inter"]["v_inter/t"][0]) == calls * EPOCHS * -(-inter_rows // MB)
    S = bs.slice_spec(case)[0]
    assert all(run["slices"][s][k].tobytes() != run["start"][s][k].tobytes() for s in range(S) for k in ("intra/w0", "v_intra/w0")), "a slice did not train"


def _shares_of(case, counts):
    """The shares the docstring promises: 20 and 100 rows, every other slice more than a minibatch; S 1: the one share"""
    S = bs.slice_spec(case)[0]
    if S == 1:
        assert counts == [MID]
        return
    rest = list(counts)
    rest.remove(SMALL)
    rest.remove(MID)
    assert len(counts) == S and counts.count(SMALL) >= 1 and counts.count(MID) >= 1 and all(c > MB for c in rest), counts


# ---- 0. what the grid covers -------------------------------------------------------------------------------------------------------------------
def test_the_grid_holds_both_ends_of_s_and_both_orders_of_the_kinds_block_counts():
    assert [bs.slice_spec(c)[0] for c in CASES] == [1, 16, 10, 13, 3, 2, 2]
    claims = bs.slice_block_claims(CASES)
    print(claims)
    assert claims["inter pair has more blocks"] == ["C", "F", "B"] and claims["intra pair has more blocks"] == [bs.SLICE_LOPSIDED]
    assert claims["af off the block grid, inter"] == list(CASES) == claims["af off the block grid, intra"]
    for case in bs.SLICE_SHAPES:
        _, _, _, (aw, _), (cw, _) = bs.slice_spec(case)
        assert len(aw) != len(cw), "a critic deeper or shallower than the actor"


# ---- 1. every slice against the float64 twin, then one Adam step -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_gradient_statistics_and_adam_step_of_every_slice_at_three_slabs_against_the_float64_twin(case):
    """ref.check_against_twin per slice on an lr = 0 call of one minibatch per policy (288 inter rows: nine tiles on three slabs), then
    ref.check_adam_step on the first real step from zero moments, on ALL S slices; S 1 runs its slice on the 20-row share here"""
    S, _, layout, (_, aa), (_, ca) = bs.slice_spec(case)
    bind = _spread(case, 3)
    env = _env(case, bind)
    rec = _record(env, case)
    order, counts = _order(rec, 1, SMALL)
    out = env.ppo_update_per_slice(rec, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, order=order, grad=True)
    views = [bs.SliceView(env, s) for s in range(S)]
    w0 = [v.weights() for v in views]
    misses, worst = [], 0.0
    for s, v in enumerate(views):
        lists = bs.share(order, s)
        # (the inter pair is unit 0 for every slice: its twin runs once, beside slice 0 -- a kind without twin rows is passed over)
        twin_lists = lists if s == 0 else dict(lists, first_inter=np.array([0, 0], dtype=np.int32))
        w, miss = ref.check_against_twin(rec, lists, v.out(out), w0[s], [0], f"{case} slice {s}", aa, ca, layout, twin_order=twin_lists)
        assert 0.0 < w <= 8.0
        worst, misses = max(worst, w), misses + miss
        assert out["rows"][1 + s, 0] == counts[s]
    assert not misses, misses
    assert out["rows"].shape[0] == 1 + S and out["rows"][0, 0] == _T(case) * B
    hp = dict(lr=[1e-3], grad_clip=[0.5], betas=(0.9, 0.999), eps=1e-8)
    env.ppo_bind(**bind)                         # (the lr = 0 call moved moments and counters: the later bind zeroes them)
    out = env.ppo_update_per_slice(rec, epochs=1, minibatch=ALL, lr=1e-3, grad_clip=0.5, order=order, grad=True)
    ulps = [ref.check_adam_step(v, v.out(out), w0[s], v.weights(), hp, 1, f"{case} slice {s}") for s, v in enumerate(views)]
    env.close()
    print(f"{case}: per slice at 3 slabs, worst gradient ratio {worst:.3g}, Adam worst ulp {max(u[0] for u in ulps)} (weights) {max(u[1] for u in ulps)} (moments)")


# ---- 2. bit for bit against the spread binding on one shared pair --------------------------------------------------------------------------------
@pytest.mark.parametrize("slabs", [2, 3])
@pytest.mark.parametrize("case", CASES)
def test_slices_bit_for_bit_against_the_spread_binding_on_one_shared_pair(case, slabs):
    """Slices 0, 1, S // 2 and S - 1 and the inter pair after two epochs of minibatches of 72 at fewer slabs than a minibatch's three
    tiles and at as many; every slice trained; the counters read 2 x ceil(n_s / 72)"""
    run = _run(case, slabs)
    _shares_of(case, run["counts"])
    _against_shared_handles(case, run, _checked(case), slabs)


# ---- 3. one slab, one minibatch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_one_slab_and_one_minibatch_give_the_per_slice_bindings_gradient_for_every_unit(case):
    """slabs=1, lr 0, one minibatch of every unit's rows: the tile order and the adds are the one-workgroup kernel's, so dev_grad of all
    1 + S units equals ``ppo_bind(per_slice=True[, wide=True])``'s byte for byte; the statistics (summed per slab) within 1e-6"""
    S = bs.slice_spec(case)[0]
    env_s, env_p = _env(case, _spread(case, 1)), _env(case, dict(per_slice=True, **_wide(case)))
    rec_s, rec_p = _twin_records(env_s, env_p, case)
    order, counts = _order(rec_s, 1, MID)
    hp = dict(epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, order=order, grad=True)
    out_s, out_p = env_s.ppo_update_per_slice(rec_s, **hp), env_p.ppo_update_per_slice(rec_p, **hp)
    assert out_s["grad"].shape == out_p["grad"].shape and out_s["grad"].shape[0] == 1 + S
    for u in range(1 + S):
        assert torch.equal(out_s["grad"][u], out_p["grad"][u]) and bool(out_s["grad"][u].any()), f"{case}: dev_grad of unit {u} differs from the per-slice binding's"
    for name in STAT_NAMES:
        assert np.allclose(out_s[name], out_p[name], rtol=1e-6, atol=1e-6), name
    assert np.array_equal(out_s["rows"][:, 0], [_T(case) * B] + counts) and np.all(out_s["minibatches"] == 1)
    env_s.close()
    env_p.close()


# ---- 4. slab invariance at the stride's far end ----------------------------------------------------------------------------------------------------
def _far_end_case():
    """The plain case with the most slices whose slabs at 256 stay under the cap, and its bytes there"""
    sized = {c: be.ppo_slices_spread_bytes(*bs.slice_dims(c)["inter"], *bs.slice_dims(c)["intra"], bs.slice_spec(c)[0], sp.SLABS_MAX) for c in PLAIN}
    fits = [c for c in PLAIN if sized[c] < FAR_END_CAP]
    case = max(fits, key=lambda c: bs.slice_spec(c)[0])
    return case, sized


def test_256_slabs_give_three_slabs_bytes_at_the_far_end_of_the_slab_stride():
    """256 slabs at three tiles per minibatch: unit 1 + s's slabs lie s x 256 x (the pair's floats) behind unit 1's, in an allocation of
    which 3 in 256 slabs are ever written; the result is a function of min(tiles, slabs), so every unit has the 3-slab run's bytes, and
    the 2-slab run (another sum order) has others"""
    case, sized = _far_end_case()
    S = bs.slice_spec(case)[0]
    floats = {c: bs.slice_kind_floats(c)["intra"][1] for c in PLAIN if bs.slice_spec(c)[0] > 1}
    assert min(floats, key=floats.get) == "C" and floats["C"] == 30112 and sized["C"] == 546209792 > FAR_END_CAP      # 520.9 MiB at S 16
    assert case == "B" and S == 13 and sized[case] == 454033408 < FAR_END_CAP                                         # 433.0 MiB
    assert sized[case] == ps.slices_spread_bytes(*bs.slice_dims(case)["inter"], *bs.slice_dims(case)["intra"], S, sp.SLABS_MAX, False)
    assert (S - 1) * sp.SLABS_MAX * floats[case] == 12 * 256 * 30208      # floats between unit 1's slabs and the last unit's
    three, far, two = _run(case, 3), _run(case, sp.SLABS_MAX), _run(case, 2)
    _same_run(three, far, f"{case}, 256 slabs against 3")
    assert np.array_equal(two["out"]["rows"], three["out"]["rows"]) and two["counts"] == three["counts"]
    assert two["inter"]["inter/w0"].tobytes() != three["inter"]["inter/w0"].tobytes()


# ---- 5. who finishes first -----------------------------------------------------------------------------------------------------------------------
WHO = "B"


def test_an_inter_pair_of_twenty_rows_is_through_while_the_slices_run_on():
    """``order_inter[:, :20]``: unit 0 takes 2 optimiser steps, the slices up to 2 x ceil(live / 72) -- the unit that has gone quiet is
    the one every other run keeps busy longest.  Slices 0 and S - 1 and the inter pair against shared handles given the same lists."""
    run, S = _run(WHO, 3, variant="inter 20"), bs.slice_spec(WHO)[0]
    assert run["order"]["order_inter"].shape == (EPOCHS, SMALL) and max(run["counts"]) > MB
    assert np.all(run["out"]["rows"][0] == SMALL) and np.all(run["out"]["minibatches"][0] == 1)
    _against_shared_handles(WHO, run, [0, S - 1], 3, inter_rows=SMALL)
    full = _run(WHO, 3)
    for s in range(S):                           # (a slice's bytes do not depend on how long the inter pair runs)
        ref.same_state(run["slices"][s], full["slices"][s], f"slice {s} beside a short inter list")
    _same_out(run["out"], full["out"], "beside a short inter list", range(1, 1 + S))


def test_an_inter_list_of_zero_rows_leaves_the_inter_pair_alone_and_trains_every_slice():
    """``n_inter`` 0, which the C entry admits: the inter pair's weights, moments and counter keep their bytes, its statistics row and
    gradient are zero, and every slice equals the full run's (and slices 0 and S - 1 their shared handles, given the same lists)"""
    run, S = _run(WHO, 3, variant="inter 0"), bs.slice_spec(WHO)[0]
    assert run["order"]["order_inter"].shape == (EPOCHS, 0) and run["order"]["first_inter"].tolist() == [0, 0]
    ref.same_state(run["inter"], run["start_inter"], "an inter pair without rows")
    assert int(run["inter"]["inter/t"][0]) == 0 and not run["inter"]["inter/m"].any() and not run["inter"]["v_inter/v"].any()
    stats, grad = bs.wg_row(run["out"], 0)
    assert not stats.any() and not grad.any()
    _against_shared_handles(WHO, run, [0, S - 1], 3, inter_rows=0)
    full = _run(WHO, 3)
    for s in range(S):
        ref.same_state(run["slices"][s], full["slices"][s], f"slice {s} beside an inter pair without rows")
    _same_out(run["out"], full["out"], "beside an inter pair without rows", range(1, 1 + S))


def test_without_intra_lists_the_inter_pair_trains_alone():
    """No ``order_intra``: one unit.  The inter pair equals the full run's and a shared handle's given the inter list alone; every slice
    keeps its bytes and has zero statistics and gradient rows"""
    run, S = _run(WHO, 3, variant="no intra"), bs.slice_spec(WHO)[0]
    assert "order_intra" not in run["order"]
    full = _run(WHO, 3)
    ref.same_state(run["inter"], full["inter"], "the inter pair alone")
    _same_out(run["out"], full["out"], "the inter pair alone", [0])
    assert int(run["inter"]["inter/t"][0]) == EPOCHS * -(-_T(WHO) * B // MB) == 8
    assert run["inter"]["inter/w0"].tobytes() != run["start_inter"]["inter/w0"].tobytes()
    shared = _shared_env(WHO, 0, spread=True, slabs=3)
    o = shared.ppo_update(run["rec"], epochs=EPOCHS, minibatch=MB, order=run["order"], grad=True, **HP)
    ref.same_state(run["inter"], bs.plain_state(shared, 0), "the inter pair alone against the shared handle")
    stats, grad = bs.wg_row(run["out"], 0)
    assert stats.tobytes() == np.stack([o[name][0, 0] for name in STAT_NAMES], axis=-1).tobytes()
    assert grad.tobytes() == o["grad"][0, 0].cpu().numpy().tobytes() and grad.any()
    shared.close()
    for s in range(S):
        ref.same_state(run["slices"][s], run["start"][s], f"slice {s} of a call without intra lists")
        assert int(run["slices"][s]["intra/t"][0]) == 0 and not run["slices"][s]["intra/m"].any()
        stats, grad = bs.wg_row(run["out"], 1 + s)
        assert not stats.any() and not grad.any()


def test_a_second_call_starts_every_unit_from_its_own_counter():
    """Two calls in a row with no bind between them: the second reads 1 + S counters that differ (2, 4, 6 and 8 steps behind the first
    call) through one t0 cell per unit.  The slices of 20 and of 100 rows, slices 0 and S - 1 and the inter pair against shared handles
    that ran the same two calls"""
    run, S = _run(WHO, 3, calls=2), bs.slice_spec(WHO)[0]
    counts = run["counts"]
    assert len({-(-c // MB) for c in counts} | {-(-_T(WHO) * B // MB)}) >= 3, counts
    _against_shared_handles(WHO, run, sorted({0, S - 1, counts.index(SMALL), counts.index(MID)}), 3, calls=2)
    once = _run(WHO, 3)
    assert all(int(run["slices"][s]["intra/t"][0]) == 2 * int(once["slices"][s]["intra/t"][0]) for s in range(S))
    assert all(run["slices"][s]["intra/w0"].tobytes() != once["slices"][s]["intra/w0"].tobytes() for s in range(S))


# ---- 6. an empty last slice at 16 slices ---------------------------------------------------------------------------------------------------------
def test_an_empty_last_slice_at_sixteen_slices_keeps_its_bytes_and_leaves_the_others_alone():
    """Case C, the last of 17 units without rows: its weights, moments and counter keep their bytes, its statistics rows are zero;
    slice 0, slice S - 2 and the inter pair equal the full run byte for byte"""
    case = "C"
    S = bs.slice_spec(case)[0]
    empty = S - 1
    full, run = _run(case, 3), _run(case, 3, empty=empty)
    assert S == 16 and run["counts"][empty] == 0 and run["counts"][:empty] == full["counts"][:empty]
    ref.same_state(run["slices"][empty], run["start"][empty], f"empty slice {empty}")
    assert int(run["slices"][empty]["intra/t"][0]) == 0
    stats, grad = bs.wg_row(run["out"], 1 + empty)
    assert not stats.any() and not grad.any()
    ref.same_state(run["inter"], full["inter"], "the inter pair beside an empty slice")
    for s in (0, S - 2):
        ref.same_state(run["slices"][s], full["slices"][s], f"slice {s} beside the empty slice {empty}")
    _same_out(run["out"], full["out"], f"beside the empty slice {empty}", [0, 1, S - 1])


# ---- 7. growth across binds ----------------------------------------------------------------------------------------------------------------------
def test_a_handle_grown_from_a_two_unit_spread_binding_equals_a_fresh_one_and_so_does_the_way_back():
    """Case F on one handle: a shared pair under ``ppo_bind(spread=True, slabs=2)`` and one update (2 units of doubles, 2 slabs of two
    pairs); then the S per-slice nets under ``per_slice=True, spread=True, slabs=8`` (11 units, 8 slabs of 11 pairs): its state and one
    update equal a fresh handle's; then the shared pair under ``spread=True, slabs=2`` again equals a fresh shared handle"""
    case = "F"
    S = bs.slice_spec(case)[0]
    env = _shared_env(case, 0, spread=True, slabs=2)
    fresh = _env(case, _spread(case, 8))
    rec = rec_f = _record(env, case)             # (one record for every handle here: the update reads no state of the env's)
    order, counts = _order(rec, EPOCHS, MID)
    shared_hp = dict(epochs=EPOCHS, minibatch=MB, order=bs.share(order, 0), grad=True, **HP)
    first = env.ppo_update(rec, **shared_hp)
    assert int(bs.plain_state(env, 1)["intra/t"][0]) == EPOCHS * -(-counts[0] // MB) and bs.plain_state(env, 0)["inter/m"].any()
    # ... grown: 2 -> 1 + S units, 2 -> 8 slabs, one intra pair -> S
    _set_nets(env, case)
    env.ppo_bind(**_spread(case, 8))

    def same(x, y, what):
        (sx, ix), (sy, iy) = _states(x), _states(y)
        ref.same_state(ix, iy, what)
        for s in range(S):
            ref.same_state(sx[s], sy[s], f"{what}, slice {s}")

    same(env, fresh, "the grown handle behind its bind")
    assert int(bs.slice_state(env, None)["inter/t"][0]) == 0 and not bs.slice_state(env, None)["inter/m"].any()
    hp = dict(epochs=EPOCHS, minibatch=MB, order=order, grad=True, **HP)
    out, out_f = env.ppo_update_per_slice(rec, **hp), fresh.ppo_update_per_slice(rec_f, **hp)
    same(env, fresh, "the grown handle behind one update")
    _same_out(out, out_f, "the grown handle's update")
    assert all(int(bs.slice_state(env, s)["intra/t"][0]) == EPOCHS * -(-counts[s] // MB) for s in range(S))
    fresh.close()
    # ... and back: the shared pair under 2 slabs, in allocations that stayed at their larger size
    _set_nets(env, case, 0)
    env.ppo_bind(spread=True, slabs=2)
    again = env.ppo_update(rec, **shared_hp)
    fresh = _shared_env(case, 0, spread=True, slabs=2)
    out_f = fresh.ppo_update(rec, **shared_hp)
    for kind in (0, 1):
        ref.same_state(bs.plain_state(env, kind), bs.plain_state(fresh, kind), f"the way back, kind {kind}")
    for name in STAT_NAMES:
        assert again[name].tobytes() == out_f[name].tobytes() == first[name].tobytes(), name
    assert torch.equal(again["grad"], out_f["grad"]) and torch.equal(again["grad"], first["grad"]) and bool(again["grad"].any())
    fresh.close()
    env.close()


# ---- 8. device row lists at the ends of S --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["D", "C"])
def test_device_row_lists_at_one_slice_and_at_sixteen(case):
    """``order="device", seed=9`` equals the explicit-list call given ``env.ppo_row_order(rec, epochs, 9, per_slice=True)`` on a twin
    handle, byte for byte; ``rows[1:, 0]`` reads the live cells per slice"""
    S = bs.slice_spec(case)[0]
    env_a, env_b = _env(case, _spread(case, 3)), _env(case, _spread(case, 3))
    rec_a, rec_b = _twin_records(env_a, env_b, case)
    lists = env_b.ppo_row_order(rec_b, EPOCHS, 9, per_slice=True)
    live = rec_a["mask_inter"].cpu().numpy().astype(bool).sum(axis=(0, 1))
    assert len(lists["first_intra"]) == S + 1 and np.array_equal(np.diff(lists["first_intra"]), live) and lists["first_inter"].tolist() == [0, _T(case) * B]
    hp = dict(epochs=EPOCHS, minibatch=MB, grad=True, **HP)
    out_a, out_b = env_a.ppo_update_per_slice(rec_a, order="device", seed=9, **hp), env_b.ppo_update_per_slice(rec_b, order=lists, **hp)
    _same_out(out_a, out_b, f"{case}: device lists")
    (sl_a, in_a), (sl_b, in_b) = _states(env_a), _states(env_b)
    ref.same_state(in_a, in_b, f"{case}: device lists, inter")
    for s in range(S):
        ref.same_state(sl_a[s], sl_b[s], f"{case}: device lists, slice {s}")
        assert int(sl_a[s]["intra/t"][0]) == EPOCHS * -(-int(live[s]) // MB) > 0
    assert np.array_equal(out_a["rows"][1:, 0], live) and out_a["rows"][0, 0] == _T(case) * B
    env_a.close()
    env_b.close()


# ---- 9. the refusal beyond the plan --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BEYOND)
def test_beyond_the_plan_the_bind_without_wide_is_refused_and_no_weight_moves(case):
    S, Us, layout, (aw, _), (cw, _) = bs.slice_spec(case)
    env = _workload(case)
    _set_nets(env, case)
    weights = lambda: [w.tobytes() + b.tobytes() for s in range(S) for r in ("intra", "v_intra") for w, b in bs.host(env.net_weights(r, slice=s))] + \
                      [w.tobytes() + b.tobytes() for r in ("inter", "v_inter") for w, b in bs.host(env.net_weights(r))]      # noqa: E731
    before = weights()
    code, text = ref.refusal(lambda: env.ppo_bind(per_slice=True, spread=True, slabs=3))
    need = ref.lds_bytes(S, Us, layout, aw, cw)
    assert need > ref.LDS_MAX and code == E_STATE and "LDS" in text, text
    assert weights() == before, "the refused bind moved a weight"
    env.close()
