"""The per-slice spread binding of the PPO update on the device (ranenv_ppo_bind_slices_spread; the kernels
ranenv_ppo_spread_slices_pass_kernel, _pass_kernel_wide, _reduce_kernel and _apply_kernel): the per-slice binding's 1 + S policies under
the spread binding's three launches per optimiser step.  Held bit for bit against the existing spread binding -- a handle bound to ONE
shared intra pair (slice s's nets) under ``ppo_bind(spread=True, slabs=N)`` and given slice s's share of the row list --, against the
per-slice binding at one slab, against the float64 twin ``adapters.ppo_update_reference`` through the comparisons of
tests/ppo_update_ref.py at its tolerances, and in its slab invariance, its empty slices, its wide twin, the next collect(), the device
row lists, the caps, the refusals and the re-binding rules.

The shape and the shares are tests/ppo_per_slice_spread_ref.py's (``ps``): S 3, Us 4, B 12, T 24, nets of ``ref.CASES``, S distinct
pairs, minibatch 72 (three tiles, the last of 8 rows), 2 epochs; shares of 20 rows, of 100 (72 + 28) and of all live rows beside 288
inter rows, so the four units take 2, 4, 2 x ceil(live / 72) and 8 optimiser steps and finish at different launches.

Measured on one MI355X (printed by the tests):
    worst tensor's error / float32 twin's over the inter pair and every slice at 3 slabs (bound 8): relu24 0.277, tanh40x24 0.318,
    tanh8x4 0.318; [512] x 3 under per_slice + spread + wide: 1.32; the statistics within 1e-7 of the twin (bound 1e-6)
    one Adam step (weights / moments): 0 / 0 ulp on every slice of all three cases
    the next collect()'s intra log-probabilities: 0.004 of collect_ref's bound from the float64 forward of the trained nets"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import ppo_bindings_shapes_ref as bs
from tests import ppo_per_slice_spread_ref as ps
from tests import ppo_update_ref as ref
from tests.gpu_common import need_gpu, shaped_workload, to_host

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -3
S, US, B, T, MB, EPOCHS = ps.S, ps.US, ps.B, ps.T, ps.MB, ps.EPOCHS
ALL = ref.ALL
HP = dict(lr=2e-3, clip=0.2, vf_coeff=0.5, ent_coeff=0.01, grad_clip=0.5)
STAT_NAMES = bs.STAT_NAMES
CASE = "tanh40x24"                       # the case of the tests that run on one


def _workload(n_slices=S, us=US, batch=B):
    need_gpu()
    return shaped_workload(n_slices, us, batch, seed=71).env


def _spread(slabs=3, **kw):
    return dict(per_slice=True, spread=True, slabs=slabs, **kw)


def _env(case, bind=None, nets=None):
    """A reset env under the case's non-shared nets, bound with ``ppo_bind(**bind)`` (default: this binding at 3 slabs)"""
    env, nets = _workload(), ps.nets(case) if nets is None else nets
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=ref.SEED, intra_input=ref.CASES[case][2])
    env.set_value_network(nets["v_inter"], nets["v_intra"])
    env.ppo_bind(**(_spread() if bind is None else bind))
    env.reset()
    return env


def _shared_env(case, s, **bind):
    """A reset env under ONE shared intra pair, slice s's nets, bound with ``ppo_bind(**bind)``"""
    env, nets = _workload(), ps.nets(case)
    env.set_policy_network(nets["inter"], nets["intra"][s], stochastic=True, seed=ref.SEED, intra_input=ref.CASES[case][2])
    env.set_value_network(nets["v_inter"], nets["v_intra"][s])
    env.ppo_bind(**bind)
    env.reset()
    return env


def _record(env, steps=T):
    rec = env.collect(steps)
    torch.cuda.synchronize()
    return rec


def _twin_records(env_a, env_b, steps=T):
    rec_a, rec_b = _record(env_a, steps), _record(env_b, steps)
    for k in rec_a:
        assert torch.equal(rec_a[k], rec_b[k]), k
    return rec_a, rec_b


def _states(env):
    return [bs.slice_state(env, s) for s in range(env.S)], bs.slice_state(env, None)


def _same_out(a, b, what, units=None):
    for u in range(a["rows"].shape[0]) if units is None else units:
        (sa, ga), (sb, gb) = bs.wg_row(a, u), bs.wg_row(b, u)
        assert sa.tobytes() == sb.tobytes(), f"{what}: statistics of unit {u}"
        assert ga.tobytes() == gb.tobytes(), f"{what}: last gradient of unit {u}"


_RUNS = {}


def _run(case, slabs, empty=None, wide=False):
    """2 epochs x minibatches of 72 on a stochastic record under this binding, computed once"""
    key = (case, slabs, empty, wide)
    if key not in _RUNS:
        env = _env(case, _spread(slabs, wide=wide))
        rec = _record(env)
        order, counts = ps.slice_order(rec, EPOCHS, empty)
        start, _ = _states(env)
        out = env.ppo_update_per_slice(rec, epochs=EPOCHS, minibatch=MB, order=order, grad=True, **HP)
        slices, inter = _states(env)
        _RUNS[key] = dict(rec=rec, order=order, counts=counts, out=out, start=start, slices=slices, inter=inter)
        env.close()
    return _RUNS[key]


# ---- 1. every unit against the spread binding on one shared pair ------------------------------------------------------------------------
@pytest.mark.parametrize("slabs", ps.SLABS)
@pytest.mark.parametrize("case", list(ref.CASES))
def test_every_unit_bit_for_bit_against_the_spread_binding_on_one_shared_pair(case, slabs):
    """Slice s's weights, moments, counter, statistics and last gradient equal, byte for byte, those of a handle bound to the shared pair
    (net s) under ``ppo_bind(spread=True, slabs=N)`` and updated with ``bs.share(order, s)``; the inter pair equals that handle's inter
    kind; every slice trained; the counters read 2 x ceil(n_s / 72) -- the units' step counts differ, and no unit runs another's"""
    run = _run(case, slabs)
    counts = run["counts"]
    assert ps.SMALL in counts and ps.MID in counts and len({-(-c // MB) for c in counts} | {-(-T * B // MB)}) >= 3, counts
    for s in range(S):
        shared = _shared_env(case, s, spread=True, slabs=slabs)
        o = shared.ppo_update(run["rec"], epochs=EPOCHS, minibatch=MB, order=bs.share(run["order"], s), grad=True, **HP)
        ref.same_state(run["slices"][s], bs.plain_state(shared, 1), f"{case}, {slabs} slabs, slice {s}")
        stats, grad = bs.wg_row(run["out"], 1 + s)
        assert stats.tobytes() == np.stack([o[n][0, 1] for n in STAT_NAMES], axis=-1).tobytes(), f"{case} slice {s}: statistics"
        assert grad.tobytes() == o["grad"][0, 1].cpu().numpy().tobytes() and grad.any(), f"{case} slice {s}: last gradient"
        assert int(run["slices"][s]["intra/t"][0]) == int(run["slices"][s]["v_intra/t"][0]) == EPOCHS * -(-counts[s] // MB)
        assert np.all(run["out"]["minibatches"][1 + s] == -(-counts[s] // MB)) and np.all(run["out"]["rows"][1 + s] == counts[s])
        if s == 0:
            ref.same_state(run["inter"], bs.plain_state(shared, 0), f"{case}, {slabs} slabs, inter pair")
            stats, grad = bs.wg_row(run["out"], 0)
            assert stats.tobytes() == np.stack([o[n][0, 0] for n in STAT_NAMES], axis=-1).tobytes(), f"{case}: inter statistics"
            assert grad.tobytes() == o["grad"][0, 0].cpu().numpy().tobytes() and grad.any(), f"{case}: inter gradient"
        shared.close()
    assert int(run["inter"]["inter/t"][0]) == EPOCHS * -(-T * B // MB) == 8
    assert all(run["slices"][s][k].tobytes() != run["start"][s][k].tobytes() for s in range(S) for k in ("intra/w0", "v_intra/w0")), "a slice did not train"


# ---- 2. one slab, one minibatch -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(ref.CASES))
def test_one_slab_and_one_minibatch_give_the_per_slice_bindings_gradient_bit_for_bit(case):
    """slabs=1, lr 0, one minibatch of every unit's rows: the tile order and the adds are the one-workgroup kernel's, so dev_grad of
    every unit equals ``ppo_bind(per_slice=True)``'s byte for byte; the statistics (summed per slab) within 1e-6"""
    env_s, env_p = _env(case, _spread(1)), _env(case, dict(per_slice=True))
    rec_s, rec_p = _twin_records(env_s, env_p)
    order, counts = ps.slice_order(rec_s, 1)
    hp = dict(epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, order=order, grad=True)
    out_s, out_p = env_s.ppo_update_per_slice(rec_s, **hp), env_p.ppo_update_per_slice(rec_p, **hp)
    assert out_s["grad"].shape[0] == 1 + S
    for u in range(1 + S):
        assert torch.equal(out_s["grad"][u], out_p["grad"][u]) and bool(out_s["grad"][u].any()), f"{case}: dev_grad of unit {u} differs from the per-slice binding's"
    for name in STAT_NAMES:
        assert np.allclose(out_s[name], out_p[name], rtol=1e-6, atol=1e-6), name
    assert np.array_equal(out_s["rows"][:, 0], [T * B] + counts) and np.all(out_s["minibatches"] == 1)
    env_s.close()
    env_p.close()


# ---- 3. three slabs against the twin ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(ref.CASES))
def test_gradient_statistics_and_adam_step_of_every_slice_at_three_slabs_against_the_float64_twin(case):
    """ref.check_against_twin (gradient per layer tensor within 8x the float32-torch yardstick of the float64 twin, statistics 1e-6) on an
    lr = 0 call of one minibatch per policy, per slice with slice s's nets and share; then ref.check_adam_step (4 float32 ulp of the
    stated arithmetic on the device's own gradient) on the first real step from zero moments"""
    env = _env(case)
    rec = _record(env)
    order, counts = ps.slice_order(rec, 1)
    act, layout = ref.CASES[case][1], ref.CASES[case][2]
    out = env.ppo_update_per_slice(rec, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, order=order, grad=True)
    views = [bs.SliceView(env, s) for s in range(S)]
    w0 = [v.weights() for v in views]
    misses = []
    for s, v in enumerate(views):
        worst, miss = ref.check_against_twin(rec, bs.share(order, s), v.out(out), w0[s], [0], f"{case} slice {s}", act, act, layout)
        assert 0.0 < worst <= 8.0
        misses += miss
        assert out["rows"][1 + s, 0] == counts[s]
    assert not misses, misses
    hp = dict(lr=[1e-3], grad_clip=[0.5], betas=(0.9, 0.999), eps=1e-8)
    env.ppo_bind(**_spread())                # (the lr = 0 call moved moments and counters: the later bind replaces the earlier one and zeroes them)
    out = env.ppo_update_per_slice(rec, epochs=1, minibatch=ALL, lr=1e-3, grad_clip=0.5, order=order, grad=True)
    for s, v in enumerate(views):
        ref.check_adam_step(v, v.out(out), w0[s], v.weights(), hp, 1, f"{case} slice {s}")
    env.close()


# ---- 4. slab invariance -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(ref.CASES))
def test_eight_slabs_give_three_slabs_bytes_at_three_tiles_per_minibatch(case):
    """No minibatch of 72 has more than three tiles: the result is a function of min(tiles, slabs) per unit alone"""
    a, b = _run(case, 3), _run(case, 8)
    assert a["counts"] == b["counts"]
    ref.same_state(a["inter"], b["inter"], f"{case} inter")
    for s in range(S):
        ref.same_state(a["slices"][s], b["slices"][s], f"{case} slice {s}")
    _same_out(a["out"], b["out"], case)
    two = _run(case, 2)                      # (... and fewer slabs than tiles is another sum order: equal rows, other bytes)
    assert np.array_equal(two["out"]["rows"], a["out"]["rows"]) and two["inter"]["inter/w0"].tobytes() != a["inter"]["inter/w0"].tobytes()


# ---- 5. an empty slice ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("empty", [0, 1, 2])
def test_an_empty_slice_keeps_its_bytes_and_leaves_the_others_alone(empty):
    """A slice whose share is empty returns at once in all three launches of every step: weights, moments and counter keep their bytes,
    its statistics rows are zero; the other units equal, byte for byte, the run with that slice present"""
    full, run = _run(CASE, 3), _run(CASE, 3, empty=empty)
    assert run["counts"][empty] == 0 and [c for s, c in enumerate(run["counts"]) if s != empty] == [c for s, c in enumerate(full["counts"]) if s != empty]
    ref.same_state(run["slices"][empty], run["start"][empty], f"empty slice {empty}")
    assert int(run["slices"][empty]["intra/t"][0]) == 0
    stats, grad = bs.wg_row(run["out"], 1 + empty)
    assert not stats.any() and not grad.any()
    ref.same_state(run["inter"], full["inter"], "the inter pair beside an empty slice")
    for s in range(S):
        if s != empty:
            assert torch.equal(bs.share(run["order"], s)["order_intra"], bs.share(full["order"], s)["order_intra"]), "the slice's lists are equal"
            ref.same_state(run["slices"][s], full["slices"][s], f"slice {s} beside the empty slice {empty}")
    _same_out(run["out"], full["out"], f"beside the empty slice {empty}", [u for u in range(1 + S) if u != 1 + empty])


# ---- 6. wide ----------------------------------------------------------------------------------------------------------------------------------
def test_the_wide_plan_gives_the_lds_plans_bytes_where_both_hold():
    plain, wide = _run(CASE, 3), _run(CASE, 3, wide=True)
    ref.same_state(plain["inter"], wide["inter"], "inter")
    for s in range(S):
        ref.same_state(plain["slices"][s], wide["slices"][s], f"slice {s}")
    _same_out(plain["out"], wide["out"], "wide against plain")


def test_beyond_the_lds_plan_every_slice_against_the_float64_twin():
    """``bs.SLICE_BEYOND[0]`` ([512] x 3, S 2, Us 5) under per_slice + spread + wide at 3 slabs: shares of 20 and 40 rows beside 96 inter
    rows (three tiles), one minibatch at lr 0 against the twin; without ``wide`` the bind is refused by the LDS plan"""
    case = bs.SLICE_BEYOND[0]
    n_slices, us, layout, (_, aa), (_, ca) = bs.slice_spec(case)
    env, nets = _workload(n_slices, us, bs.SLICE_B), bs.slice_nets(case)
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=ref.SEED, intra_input=layout)
    env.set_value_network(nets["v_inter"], nets["v_intra"])
    code, text = ref.refusal(lambda: env.ppo_bind(**_spread()))
    assert code == E_STATE and "LDS" in text, text
    env.ppo_bind(**_spread(wide=True))
    env.reset()
    rec = _record(env, bs.SLICE_T)
    order, counts = bs.slice_order(rec, 1, bs.SLICE_MB, bs.SMALL, bs.BIG)
    assert sorted(counts) == [bs.SMALL, bs.BIG]
    out = env.ppo_update_per_slice(rec, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, order=order, grad=True)
    misses = []
    for s in range(n_slices):
        v = bs.SliceView(env, s)
        lists = bs.share(order, s)
        twin_lists = lists if s == 0 else dict(lists, first_inter=np.array([0, 0], dtype=np.int32))      # (the inter pair's twin runs once)
        worst, miss = ref.check_against_twin(rec, lists, v.out(out), v.weights(), [0], f"{case} slice {s}", aa, ca, layout, twin_order=twin_lists)
        assert 0.0 < worst <= 8.0
        misses += miss
        assert out["rows"][1 + s, 0] == counts[s]
    assert not misses, misses
    env.close()


# ---- 7. determinism, the next collect(), the device lists ---------------------------------------------------------------------------------------
def test_the_same_call_gives_the_same_bytes_and_the_next_collect_and_the_device_lists():
    """Twin handles at 3 slabs: the same call gives the same bytes; the next collect(), with no re-bind, acts on the trained nets -- the
    recorded intra log-probabilities lie within collect_ref's bound of the float64 forward of ``net_weights(.., slice=s)``; and
    ``order="device"`` runs end to end and equals the explicit-list call given ``env.ppo_row_order(..., per_slice=True)``"""
    from tests import per_slice_policy_ref as pp
    act, layout = ref.CASES[CASE][1], ref.CASES[CASE][2]
    env_a, env_b = _env(CASE), _env(CASE)
    rec_a, rec_b = _twin_records(env_a, env_b)
    order, _ = ps.slice_order(rec_a, EPOCHS)
    start, _ = _states(env_a)
    hp = dict(epochs=EPOCHS, minibatch=MB, order=order, grad=True, **HP)
    out_a, out_b = env_a.ppo_update_per_slice(rec_a, **hp), env_b.ppo_update_per_slice(rec_b, **hp)
    (sl_a, in_a), (sl_b, in_b) = _states(env_a), _states(env_b)
    ref.same_state(in_a, in_b, "twin handles, inter")
    for s in range(S):
        ref.same_state(sl_a[s], sl_b[s], f"twin handles, slice {s}")
        assert sl_a[s]["intra/w0"].tobytes() != start[s]["intra/w0"].tobytes()
    _same_out(out_a, out_b, "twin handles")
    rec2 = to_host(env_a.collect(3))
    intras = [ref.as_sequential([(w.cpu(), b.cpu()) for w, b in env_a.net_weights("intra", slice=s)], act) for s in range(S)]
    for t in range(3):
        print(f"slot {t}: worst intra logp error / bound after the update: {pp.check_intra_logp(rec2, t, intras, layout):.3g}")
    untrained = [ref.as_sequential(ref.layers_of(n), act) for n in ps.nets(CASE)["intra"]]
    with pytest.raises(AssertionError):      # (the bound tells trained nets from the bound ones)
        for t in range(3):
            pp.check_intra_logp(rec2, t, untrained, layout)
    env_b.collect(3)
    # the device lists on the twins, which still hold the same bytes
    rec_a, rec_b = _twin_records(env_a, env_b, 8)
    lists = env_b.ppo_row_order(rec_b, EPOCHS, 9, per_slice=True)
    assert len(lists["first_intra"]) == S + 1 and int(lists["first_intra"][-1]) > MB
    hp = dict(epochs=EPOCHS, minibatch=MB, grad=True, **HP)
    out_a, out_b = env_a.ppo_update_per_slice(rec_a, order="device", seed=9, **hp), env_b.ppo_update_per_slice(rec_b, order=lists, **hp)
    _same_out(out_a, out_b, "device lists")
    (sl_a, in_a), (sl_b, in_b) = _states(env_a), _states(env_b)
    ref.same_state(in_a, in_b, "device lists, inter")
    for s in range(S):
        ref.same_state(sl_a[s], sl_b[s], f"device lists, slice {s}")
    assert np.array_equal(out_a["rows"][1:, 0], rec_a["mask_inter"].cpu().numpy().astype(bool).sum(axis=(0, 1)))
    env_a.close()
    env_b.close()


# ---- 8. the caps ----------------------------------------------------------------------------------------------------------------------------------
def test_the_row_cap_does_not_apply_and_the_steps_cap_does():
    """On the test's own record, ``force`` left false: a row cap below rows x epochs is ignored under this binding and refuses under the
    per-slice one; a steps cap of 1 refuses under this binding, and the refused call moves nothing"""
    from intent_radio_sched_multi_slice_amd._lib import RanEnvError
    env = _env(CASE)
    rec = _record(env)
    order, counts = ps.slice_order(rec, EPOCHS)
    upd = lambda **kw: env.ppo_update_per_slice(rec, epochs=EPOCHS, minibatch=MB, order=order, **dict(HP, **kw))  # noqa: E731
    env.PPO_ROW_EPOCHS_CAP = 2
    assert ps.SMALL * EPOCHS > env.PPO_ROW_EPOCHS_CAP
    out = upd()
    assert np.all(out["minibatches"][0] == 4) and int(bs.slice_state(env, None)["inter/t"][0]) == 8
    env.ppo_bind(per_slice=True)
    with pytest.raises(RanEnvError, match="rows x epochs"):
        upd()
    env.ppo_bind(**_spread())
    del env.PPO_ROW_EPOCHS_CAP
    env.PPO_STEPS_CAP = 1
    before = _states(env)
    with pytest.raises(RanEnvError, match="optimiser steps"):
        upd()
    after = _states(env)
    ref.same_state(before[1], after[1], "a refused update")
    for s in range(S):
        ref.same_state(before[0][s], after[0][s], "a refused update")
    upd(force=True)
    del env.PPO_STEPS_CAP
    assert int(bs.slice_state(env, None)["inter/t"][0]) == 8
    env.close()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_what_the_binding_refuses_by_code_and_message_with_the_weights_unmoved():
    """Shared intra nets, a population, bf16 nets, a missing inter critic: RANENV_E_STATE in ranenv_ppo_bind_slices' words; slabs
    outside 1..256: RANENV_E_INVALID; the nets keep their bytes across every refused bind"""
    nets, layout = ps.nets(CASE), ref.CASES[CASE][2]
    bind = lambda **kw: (lambda: env.ppo_bind(**_spread(**kw)))      # noqa: E731

    def kept(read, fn, code_want, word):
        before = read()
        code, text = ref.refusal(fn)
        assert code == code_want and word in text and len(text) > 20, (word, code, text)
        after = read()
        assert [x.tobytes() for x in before] == [x.tobytes() for x in after], f"a refused bind moved a weight ({word})"

    def per_slice_weights():
        return [x for s in range(S) for r in ("intra", "v_intra") for pair in bs.host(env.net_weights(r, slice=s)) for x in pair] + \
               [x for r in ("inter", "v_inter") for pair in bs.host(env.net_weights(r)) for x in pair]

    def one_net_weights(roles=ref.ROLES, members=1):
        return [x for r in roles for m in range(members) for pair in bs.host(env.net_weights(r, m)) for x in pair]

    env = _env(CASE, dict(per_slice=True))
    for slabs in (0, 257, -3):
        kept(per_slice_weights, bind(slabs=slabs), E_INVALID, f"slabs {slabs} (1..256)")
    # shared intra critic beside per-slice actors, then shared intra nets altogether
    env.set_value_network(nets["v_inter"], nets["v_intra"][0])
    kept(lambda: one_net_weights(("inter", "v_inter", "v_intra")), bind(), E_STATE, "no one owner")
    env.set_policy_network(nets["inter"], nets["intra"][0], stochastic=True, seed=ref.SEED, intra_input=layout)
    kept(one_net_weights, bind(), E_STATE, "per slice")
    env.close()
    # a missing inter critic
    env = _workload()
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=ref.SEED, intra_input=layout)
    kept(lambda: one_net_weights(("inter",)), bind(), E_STATE, "inter actor and inter critic")
    env.close()
    # bf16 nets
    env = _workload()
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=ref.SEED, intra_input=layout, precision="bf16")
    env.set_value_network(nets["v_inter"], nets["v_intra"], precision="bf16")
    code, text = ref.refusal(bind())
    assert code == E_STATE and "bf16" in text, text
    env.close()
    # a population
    env = _workload()
    env.set_population([0, 2, B])
    env.set_policy_network([nets["inter"]] * 2, [nets["intra"][0]] * 2, stochastic=True, seed=ref.SEED, intra_input=layout)
    env.set_value_network([nets["v_inter"]] * 2, [nets["v_intra"][0]] * 2)
    kept(lambda: one_net_weights(members=2), bind(), E_STATE, "population")
    for kw in (dict(mixed=True), dict(head=True), dict(bf16=True)):
        with pytest.raises(ValueError):
            env.ppo_bind(**_spread(**kw))
    with pytest.raises(ValueError, match="spread and per_slice"):      # (this form takes its slab count)
        env.ppo_bind(per_slice=True, spread=True)
    env.close()


# ---- 10. binds replace each other ---------------------------------------------------------------------------------------------------------------
def test_binds_replace_each_other_and_rebound_nets_restart_or_ask_for_a_bind():
    """This binding behind the per-slice one, and back, gives a fresh handle's state and bytes; a re-bound list of intra actors restarts
    all S optimisers and leaves the inter pair's; a re-bound list of larger nets, beyond what the bind allocated, leaves the update
    RANENV_E_STATE ("bind again") until the next bind"""
    from intent_radio_sched_multi_slice_amd.batched_env import NET_INPUTS
    layout, nets = ref.CASES[CASE][2], ps.nets(CASE)
    env_a, env_b, env_c = _env(CASE, dict(per_slice=True)), _env(CASE), _env(CASE, dict(per_slice=True))
    rec_a, rec_b = _twin_records(env_a, env_b)
    order, _ = ps.slice_order(rec_a, EPOCHS)
    hp = dict(epochs=EPOCHS, minibatch=MB, order=order, grad=True, **HP)

    def same(x, y, out_x, out_y, what):
        (sx, ix), (sy, iy) = _states(x), _states(y)
        ref.same_state(ix, iy, what)
        for s in range(S):
            ref.same_state(sx[s], sy[s], f"{what}, slice {s}")
        if out_x is not None:
            _same_out(out_x, out_y, what)

    env_a.ppo_update_per_slice(rec_a, epochs=1, minibatch=MB, lr=0.0, order=order)      # (moves moments and counters, no weight)
    assert int(bs.slice_state(env_a, None)["inter/t"][0]) == 4 and bs.slice_state(env_a, 0)["intra/m"].any()
    env_a.ppo_bind(**_spread())
    same(env_a, env_b, None, None, "this binding behind the per-slice one")
    same(env_a, env_b, env_a.ppo_update_per_slice(rec_a, **hp), env_b.ppo_update_per_slice(rec_b, **hp), "the same call behind the later bind")
    # ... and back: a fresh per-slice handle under the weights this one has now
    trained = {"inter": env_a.net_weights("inter"), "v_inter": env_a.net_weights("v_inter"),
               "intra": [env_a.net_weights("intra", slice=s) for s in range(S)], "v_intra": [env_a.net_weights("v_intra", slice=s) for s in range(S)]}
    act = ref.CASES[CASE][1]
    env_c.set_policy_network(trained["inter"], trained["intra"], stochastic=True, seed=ref.SEED, intra_input=layout, activation=act)
    env_c.set_value_network(trained["v_inter"], trained["v_intra"], activation=act)
    env_c.ppo_bind(per_slice=True)
    env_a.ppo_bind(per_slice=True)
    same(env_a, env_c, None, None, "the per-slice binding behind this one")
    hp1 = dict(hp, minibatch=ALL, epochs=1)
    same(env_a, env_c, env_a.ppo_update_per_slice(rec_a, **hp1), env_c.ppo_update_per_slice(rec_a, **hp1), "the per-slice call behind the later bind")
    env_c.close()
    # a re-bound list of intra actors under this binding: all S optimisers restart, the inter pair's stays
    env_a.ppo_bind(**_spread())
    env_a.ppo_update_per_slice(rec_a, **hp)
    moved, inter = _states(env_a)
    assert all(int(x["intra/t"][0]) > 0 and x["intra/m"].any() and x["v_intra/v"].any() for x in moved) and int(inter["inter/t"][0]) == 8
    _, in_intra = env_a.net_input_dims(layout)
    env_a._set_net_list("intra_policy_nets", "ranenv_set_intra_policy_networks", env_a._net_list(nets["intra"], None, in_intra, 3, NET_INPUTS[layout]))
    after, inter_after = _states(env_a)
    for s in range(S):
        for r in ("intra", "v_intra"):
            assert int(after[s][f"{r}/t"][0]) == 0 and not after[s][f"{r}/m"].any() and not after[s][f"{r}/v"].any(), (r, s)
        for k in moved[s]:
            if k.startswith("v_intra/") and k.split("/")[1][0] in "wb":
                assert after[s][k].tobytes() == moved[s][k].tobytes(), f"re-binding the actors moved the critics' {k}"
    ref.same_state(inter_after, inter, "the inter pair across a re-bind of the per-slice actors")
    out = env_a.ppo_update_per_slice(rec_a, **hp)
    assert np.all(np.isfinite(out["grad_norm"])) and int(bs.slice_state(env_a, 0)["intra/t"][0]) == int(moved[0]["intra/t"][0])
    env_a.close()
    env_b.close()
    # larger nets than the bind allocated slabs for, in slots whose moments hold them (the slots were bound to the larger nets before)
    bigger = [ref.make_role_nets(S, US, [96, 96], act, layout, 7000 + 10 * s) for s in range(S)]
    env_d = _workload()

    def set_nets(intra, v_intra):
        env_d.set_policy_network(nets["inter"], intra, stochastic=True, seed=ref.SEED, intra_input=layout)
        env_d.set_value_network(nets["v_inter"], v_intra)

    set_nets([p["intra"] for p in bigger], [p["v_intra"] for p in bigger])
    set_nets(nets["intra"], nets["v_intra"])
    env_d.ppo_bind(**_spread())
    env_d.reset()
    rec_d = _record(env_d)
    hp = dict(hp, order=ps.slice_order(rec_d, EPOCHS)[0])
    env_d.ppo_update_per_slice(rec_d, **hp)
    set_nets([p["intra"] for p in bigger], [p["v_intra"] for p in bigger])
    code, text = ref.refusal(lambda: env_d.ppo_update_per_slice(rec_d, **hp))
    assert code == E_STATE and "slab" in text and "bind again" in text, text
    env_d.ppo_bind(**_spread())
    out = env_d.ppo_update_per_slice(rec_d, **hp)
    assert np.all(np.isfinite(out["grad_norm"])) and int(bs.slice_state(env_d, 1)["intra/t"][0]) > 0
    env_d.close()
