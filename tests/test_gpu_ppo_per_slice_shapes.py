"""The per-slice PPO update (ranenv_ppo_bind_slices / ranenv_ppo_update_slices; the kernels ranenv_ppo_update_kernel_slices and
_slices_wide) across slice counts and net shapes -- what tests/test_gpu_ppo_per_slice.py checks at S 3 and three narrow nets, here on
the per-slice grid of tests/ppo_bindings_shapes_ref.py (``bs``): S 1 (two workgroups, ``i % S`` degenerate), S 10, S 13 and S 16 (17
workgroups), actors and critics that differ in depth and width, both intra layouts, and -- what a per-slice wide binding is for -- two
nets beyond the LDS plan at S 2, which no comparison had reached.

Every case: B 12, T 8, S distinct actor / critic pairs, explicit row lists with one share of 20 rows (a partial tile), one of 40 (a tile
and a quarter, a short last minibatch of 12) and every other slice all its live rows; the counts are asserted in ``bs.slice_order``.
Comparisons and tolerances are tests/ppo_update_ref.py's: the gradient per layer tensor within 8x the float32-torch error of the float64
twin (floor 1e-6 relative), statistics 1e-6, Adam 4 float32 ulp of adam_step_f32 on the call's own dev_grad, the norm 1e-9, byte
equality against a handle bound to one shared pair under ``ppo_bind()`` (``ppo_bind(wide=True)`` beyond the plan).

Measured on one MI355X (printed by the tests):
    worst tensor's error / float32 twin's over the inter pair and every slice (bound 8): D 0.215, C 0.494, F 1.02, B 0.597; beyond the
    plan under per_slice + wide: verybig 1.32, past_limit 0.745; the five statistics within 1.3e-7 of the twin (bound 1e-6)
    one Adam step (weights / moments): 0 / 0 ulp on every slice of all six cases"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import ppo_bindings_shapes_ref as bs
from tests import ppo_update_ref as ref
from tests import ppo_wide_ref as wd
from tests.gpu_common import _ordered, need_gpu, shaped_workload

pytestmark = pytest.mark.gpu

E_STATE = -3
B, T, MB, SMALL, BIG = bs.SLICE_B, bs.SLICE_T, bs.SLICE_MB, bs.SMALL, bs.BIG
ALL = ref.ALL
HP = dict(lr=2e-3, clip=0.2, vf_coeff=0.5, ent_coeff=0.01, grad_clip=0.5)
STAT_NAMES = bs.STAT_NAMES


def _workload(case):
    need_gpu()
    S, Us = bs.slice_spec(case)[:2]
    return shaped_workload(S, Us, B, seed=71).env


def _env(case, **bind):
    """A reset env of the case's shape under its S distinct pairs, bound with ``ppo_bind(per_slice=True, **bind)``"""
    env, nets = _workload(case), bs.slice_nets(case)
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=ref.SEED, intra_input=bs.slice_spec(case)[2])
    env.set_value_network(nets["v_inter"], nets["v_intra"])
    env.ppo_bind(per_slice=True, **bind)
    env.reset()
    return env


def _shared_env(case, s, **bind):
    """A reset env under ONE shared intra pair, slice s's nets, bound with ``ppo_bind(**bind)``"""
    env, nets = _workload(case), bs.slice_nets(case)
    env.set_policy_network(nets["inter"], nets["intra"][s], stochastic=True, seed=ref.SEED, intra_input=bs.slice_spec(case)[2])
    env.set_value_network(nets["v_inter"], nets["v_intra"][s])
    env.ppo_bind(**bind)
    env.reset()
    return env


def _record(env):
    rec = env.collect(T)
    torch.cuda.synchronize()
    assert rec["mask_inter"].shape == (T, B, env.S)
    return rec


def _order(rec, epochs, only, empty=None):
    return bs.slice_order(rec, epochs, MB, SMALL, BIG, empty, only=only)


def _checked(case):
    """The slices held against a shared handle: 0, one in the middle and S - 1 (all where S <= 3)"""
    S = bs.slice_spec(case)[0]
    return sorted({0, S // 2, S - 1})


def _twin_and_adam(case, **bind):
    """ref.check_against_twin per slice on an lr = 0 call of one minibatch per policy, then ref.check_adam_step on the first real step
    from zero moments; returns (worst gradient ratio, worst ulp of the weights, of the moments)"""
    S, _, layout, (_, aa), (_, ca) = bs.slice_spec(case)
    env = _env(case, **bind)
    rec = _record(env)
    order, counts = _order(rec, 1, SMALL)
    out = env.ppo_update_per_slice(rec, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, order=order, grad=True)
    views = [bs.SliceView(env, s) for s in range(S)]
    w0 = [v.weights() for v in views]
    misses, worst = [], 0.0
    for s, v in enumerate(views):
        lists = bs.share(order, s)
        # (the inter pair is workgroup 0 for every slice: its twin runs once, beside slice 0 -- a kind without twin rows is passed over)
        twin_lists = lists if s == 0 else dict(lists, first_inter=np.array([0, 0], dtype=np.int32))
        w, miss = ref.check_against_twin(rec, lists, v.out(out), w0[s], [0], f"{case} slice {s}", aa, ca, layout, twin_order=twin_lists)
        assert 0.0 < w <= 8.0
        worst, misses = max(worst, w), misses + miss
        assert out["rows"][1 + s, 0] == counts[s]
    assert not misses, misses
    assert out["rows"].shape[0] == 1 + S and out["rows"][0, 0] == T * B
    hp = dict(lr=[1e-3], grad_clip=[0.5], betas=(0.9, 0.999), eps=1e-8)
    env.ppo_bind(per_slice=True, **bind)           # (the lr = 0 call moved moments and counters: the later bind zeroes them)
    out = env.ppo_update_per_slice(rec, epochs=1, minibatch=ALL, lr=1e-3, grad_clip=0.5, order=order, grad=True)
    ulps = [ref.check_adam_step(v, v.out(out), w0[s], v.weights(), hp, 1, f"{case} slice {s}") for s, v in enumerate(views)]
    env.close()
    print(f"{case}: per slice, worst gradient ratio {worst:.3g}, Adam worst ulp {max(u[0] for u in ulps)} (weights) {max(u[1] for u in ulps)} (moments)")
    return worst, max(u[0] for u in ulps), max(u[1] for u in ulps)


_RUNS = {}


def _run(case, empty=None, **bind):
    """2 epochs x minibatches of 12 on a stochastic record under the per-slice binding, computed once"""
    key = (case, empty, tuple(sorted(bind.items())))
    if key not in _RUNS:
        S = bs.slice_spec(case)[0]
        env = _env(case, **bind)
        rec = _record(env)
        order, counts = _order(rec, 2, BIG, empty)
        start = [bs.slice_state(env, s) for s in range(S)]
        out = env.ppo_update_per_slice(rec, epochs=2, minibatch=MB, order=order, grad=True, **HP)
        _RUNS[key] = dict(rec=rec, order=order, counts=counts, out=out, start=start, slices=[bs.slice_state(env, s) for s in range(S)],
                          inter=bs.slice_state(env, None))
        env.close()
    return _RUNS[key]


def _against_shared_handles(case, run, slices, **shared_bind):
    """Slice s's weights, moments, counter, statistics and last gradient equal, byte for byte, those of a handle bound to the shared pair
    (net s) and updated on the same record with an intra list of slice s's share; the inter pair equals that handle's inter pair"""
    for n, s in enumerate(slices):
        shared = _shared_env(case, s, **shared_bind)
        o = shared.ppo_update(run["rec"], epochs=2, minibatch=MB, order=bs.share(run["order"], s), grad=True, **HP)
        ref.same_state(run["slices"][s], bs.plain_state(shared, 1), f"{case} slice {s}")
        stats, grad = bs.wg_row(run["out"], 1 + s)
        assert stats.tobytes() == np.stack([o[name][0, 1] for name in STAT_NAMES], axis=-1).tobytes(), f"{case} slice {s}: statistics"
        assert grad.tobytes() == o["grad"][0, 1].cpu().numpy().tobytes() and grad.any(), f"{case} slice {s}: last gradient"
        assert int(run["slices"][s]["intra/t"][0]) == 2 * -(-run["counts"][s] // MB)
        if n == 0:
            ref.same_state(run["inter"], bs.plain_state(shared, 0), f"{case} inter pair")
            stats, grad = bs.wg_row(run["out"], 0)
            assert stats.tobytes() == np.stack([o[name][0, 0] for name in STAT_NAMES], axis=-1).tobytes(), f"{case}: inter statistics"
            assert grad.tobytes() == o["grad"][0, 0].cpu().numpy().tobytes(), f"{case}: inter gradient"
        shared.close()
    S = bs.slice_spec(case)[0]
    assert all(run["slices"][s][k].tobytes() != run["start"][s][k].tobytes() for s in range(S) for k in ("intra/w0", "v_intra/w0")), "a slice did not train"


# ---- the plain plan: D (S 1), C (S 16), F (S 10), B (S 13) ---------------------------------------------------------------------------
def test_the_grid_holds_one_slice_and_sixteen():
    assert [bs.slice_spec(c)[0] for c in bs.SLICE_SHAPES] == [1, 16, 10, 13]
    for case in bs.SLICE_SHAPES:
        _, _, _, (aw, _), (cw, _) = bs.slice_spec(case)
        assert len(aw) != len(cw), "a critic deeper or shallower than the actor"


@pytest.mark.parametrize("case", bs.SLICE_SHAPES)
def test_gradient_statistics_and_adam_step_of_every_slice_against_the_float64_twin(case):
    """S 1 runs its one slice on the 20-row share here and on the 40-row share in the bit-for-bit test"""
    _twin_and_adam(case)


@pytest.mark.parametrize("case", bs.SLICE_SHAPES)
def test_slices_bit_for_bit_against_the_plain_kernel_on_one_shared_pair(case):
    """Slices 0, S // 2 and S - 1 and the inter pair after two epochs of minibatches of 12, against ``ppo_bind()`` handles"""
    run = _run(case)
    S = bs.slice_spec(case)[0]
    if S > 1:
        assert run["counts"].count(SMALL) >= 1 and run["counts"].count(BIG) >= 1 and min(run["counts"]) >= SMALL and len(run["counts"]) == S
    else:
        assert run["counts"] == [BIG]
    _against_shared_handles(case, run, _checked(case))


@pytest.mark.parametrize("case", bs.SLICE_SHAPES)
def test_the_wide_binding_gives_the_plain_per_slice_bytes(case):
    plain, wide = _run(case), _run(case, wide=True)
    S = bs.slice_spec(case)[0]
    ref.same_state(plain["inter"], wide["inter"], f"{case} inter")
    for s in range(S):
        ref.same_state(plain["slices"][s], wide["slices"][s], f"{case} slice {s}")
    for wg in range(1 + S):
        a, b = bs.wg_row(plain["out"], wg), bs.wg_row(wide["out"], wg)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), f"{case} workgroup {wg}"


@pytest.mark.parametrize("case", bs.SLICE_SHAPES)
def test_the_probe_returns_the_records_own_log_probabilities_for_every_live_cell(case):
    """lr = 0, one epoch, all live rows, probe_logp: intra cells to the bit, inter cells within 1 float32 ulp (the probe tolerance of
    tests/test_gpu_ppo_update.py).  The S nets are distinct: a slice -> net shift at this S re-evaluates a slice's rows with another net."""
    env = _env(case)
    rec = _record(env)
    out = env.ppo_update_per_slice(rec, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, seed=9, probe_logp=True)
    new, old, mask = out["logp"].cpu().numpy(), rec["logp"].cpu().numpy(), rec["mask_inter"].cpu().numpy() != 0
    assert mask.any(axis=(0, 1)).all(), "a slice without a live cell"
    assert np.array_equal(new[..., 1:][mask].view(np.int32), old[..., 1:][mask].view(np.int32)), "intra logp is not re-evaluated to the bit"
    assert np.abs(_ordered(new[..., 0]) - _ordered(old[..., 0])).max() <= 1
    assert np.array_equal(out["rows"][1:, 0], mask.sum(axis=(0, 1)))
    env.close()


def test_an_empty_last_slice_at_sixteen_slices_keeps_its_bytes_and_leaves_the_others_alone():
    """Case C, the last of 17 workgroups without rows: its weights, moments and counter keep their bytes, its statistics rows are zero;
    slice 0, slice S - 2 and the inter pair equal the full run byte for byte"""
    case = "C"
    S = bs.slice_spec(case)[0]
    empty = S - 1
    full, run = _run(case), _run(case, empty=empty)
    assert S == 16 and run["counts"][empty] == 0 and run["counts"][:empty] == full["counts"][:empty]
    ref.same_state(run["slices"][empty], run["start"][empty], f"empty slice {empty}")
    assert int(run["slices"][empty]["intra/t"][0]) == 0
    stats, grad = bs.wg_row(run["out"], 1 + empty)
    assert not stats.any() and not grad.any()
    ref.same_state(run["inter"], full["inter"], "the inter pair beside an empty slice")
    for s in (0, S - 2):
        ref.same_state(run["slices"][s], full["slices"][s], f"slice {s} beside the empty slice {empty}")
        assert bs.wg_row(run["out"], 1 + s)[0].tobytes() == bs.wg_row(full["out"], 1 + s)[0].tobytes()
        assert bs.wg_row(run["out"], 1 + s)[1].tobytes() == bs.wg_row(full["out"], 1 + s)[1].tobytes()


# ---- beyond the LDS plan: verybig and past_limit at S 2 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bs.SLICE_BEYOND)
def test_beyond_the_plan_every_slice_against_the_float64_twin_and_one_adam_step(case):
    """``ppo_bind(per_slice=True, wide=True)`` on two distinct pairs beyond the LDS plan: gradient and statistics of both slices and of the
    inter pair against the float64 twin, then one Adam step"""
    _twin_and_adam(case, wide=True)


@pytest.mark.parametrize("case", bs.SLICE_BEYOND)
def test_beyond_the_plan_both_slices_bit_for_bit_against_a_shared_wide_handle(case):
    run = _run(case, wide=True)
    assert sorted(run["counts"]) == [SMALL, BIG]
    _against_shared_handles(case, run, [0, 1], wide=True)


@pytest.mark.parametrize("case", bs.SLICE_BEYOND)
def test_beyond_the_plan_the_layout_is_the_wide_formula_and_the_plain_bind_is_refused(case):
    S, Us, layout, (aw, _), (cw, _) = bs.slice_spec(case)
    env = _env(case, wide=True)
    dims = bs.slice_dims(case)
    for s in range(S):
        assert env.ppo_member_layout(s, "intra")["lds_bytes"] == wd.wide_lds_bytes(*dims["intra"]) <= wd.WIDE_LDS_MAX
    assert env.ppo_member_layout(0, "inter")["lds_bytes"] == wd.wide_lds_bytes(*dims["inter"])
    weights = lambda: [w.tobytes() + b.tobytes() for s in range(S) for r in ("intra", "v_intra") for w, b in bs.host(env.net_weights(r, slice=s))]  # noqa: E731
    before = weights()
    code, text = ref.refusal(lambda: env.ppo_bind(per_slice=True))
    need = ref.lds_bytes(S, Us, layout, aw, cw)
    assert need > ref.LDS_MAX and code == E_STATE and "LDS" in text and str(need) in text, text
    assert weights() == before, "the refused bind moved a weight"
    env.close()
