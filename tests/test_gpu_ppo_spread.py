"""The SPREAD binding of the PPO update on the device (ranenv_ppo_bind_spread / ranenv_ppo_update; the kernels of
ranenv_ppo_spread.hip: pass, reduce, apply): one slab against the plain binding bit for bit; several slabs against the float64 twin;
one Adam step; the loop of optimiser steps against one call per chunk; determinism and the next collect(); the wide plan under the
spread binding; the boundary to the other bindings.

Every case: ONE agent on ref.native_workload(12), S 5 / Us 5, T 8 -- 96 inter rows (three tiles) and a few hundred live intra rows.
Comparisons and tolerances are tests/ppo_update_ref.py's: the gradient within 8x the float32-torch error of the float64 twin (floor
1e-6 relative), statistics 1e-6, Adam 4 float32 ulp of adam_step_f32 on the call's own dev_grad, the norm 1e-9, bit equality between
bindings and schedules."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import collect_ref as cr
from tests import ppo_spread_ref as sp
from tests import ppo_update_ref as ref
from tests import ppo_wide_ref as wd
from tests.gpu_common import need_gpu, to_host

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -3
ALL, B = ref.ALL, 12
CASES = ["tanh40x24", "relu24"]
FIRST = [0, B]
HP_LOOP = dict(lr=2e-3, clip=0.2, vf_coeff=0.5, ent_coeff=0.01, grad_clip=0.5)
STAT_NAMES = ("policy_loss", "value_loss", "entropy", "kl", "clip_frac")


def _nets(case):
    if case in ref.CASES:
        return sp.one_agent_nets(case), ref.CASES[case][1], ref.CASES[case][2]
    nets = wd.beyond_nets(case, n=1)
    return {r: nets[r][0] for r in ref.ROLES}, wd.BEYOND[case][1], wd.BEYOND[case][2]


def _env(case, stochastic=True, **bind):
    """A reset env of the native shape under ONE agent of the case's nets, bound as ``bind`` says (empty: the plain binding)"""
    need_gpu()
    env = ref.native_workload(B)
    nets, _, layout = _nets(case)
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=stochastic, seed=ref.SEED, intra_input=layout)
    env.set_value_network(nets["v_inter"], nets["v_intra"])
    env.ppo_bind(**bind)
    env.reset()
    return env


def _twin_records(env_a, env_b, T=ref.T):
    rec_a, rec_b = env_a.collect(T), env_b.collect(T)
    torch.cuda.synchronize()
    for k in rec_a:
        assert torch.equal(rec_a[k], rec_b[k]), k
    return rec_a, rec_b


def _order(rec, epochs, seed=3):
    from intent_radio_sched_multi_slice_amd.adapters import ppo_row_order
    return ppo_row_order(rec, FIRST, epochs, seed)


def _cut(order, n):
    """The first n entries of the first epoch's list of both kinds"""
    out = {}
    for kind in ("inter", "intra"):
        assert int(order["first_" + kind][1]) >= n
        out["order_" + kind], out["first_" + kind] = order["order_" + kind][:1, :n].contiguous(), np.array([0, n], dtype=np.int32)
    return out


def _same_call(env_a, out_a, env_b, out_b, what):
    """Weights, m, v, counters, all eight statistics and dev_grad of two handles behind the same call, byte for byte"""
    ref.same_state(ref.state(env_a, 1), ref.state(env_b, 1), what)
    assert out_a.keys() == out_b.keys()
    for name in out_a:
        if name == "grad":
            assert torch.equal(out_a[name], out_b[name]), f"{what}: dev_grad differs"
            assert bool(out_a[name].any())
        else:
            assert np.asarray(out_a[name]).tobytes() == np.asarray(out_b[name]).tobytes(), f"{what}: statistics {name} differ"


# ---- 1. one slab ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_one_slab_gives_the_plain_bindings_gradient_bit_for_bit(case):
    """slabs=1: the tile order and the adds are the plain kernel's.  One minibatch of all rows at lr 0, both kinds; then lists of 1,
    31, 32, 33, 64 and 65 rows, and a list of 65 with entries outside the record at its head, its 33rd place and its tail: dev_grad of
    the spread handle equals the plain twin handle's byte for byte, the statistics within 1e-6 (they are summed per slab)."""
    env_s, env_p = _env(case, spread=True, slabs=1), _env(case)
    rec_s, rec_p = _twin_records(env_s, env_p)
    order = _order(rec_s, 1)
    assert int(order["first_inter"][1]) == 96 and int(order["first_intra"][1]) > 130
    T, _, S = rec_s["mask_inter"].shape
    lists = [("all rows", order)] + [(f"{n} rows", _cut(order, n)) for n in (1, 31, 32, 33, 64, 65)]
    outside = _cut(order, 65)
    for kind, n_record in (("inter", T * B), ("intra", T * B * S)):
        o = outside["order_" + kind].clone()
        o[0, 0], o[0, 32], o[0, 64] = -1, n_record, 2 ** 31 - 1
        outside["order_" + kind] = o
    lists.append(("entries outside the record", outside))
    for what, lst in lists:
        hp = dict(epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, order=lst, grad=True)
        out_s, out_p = env_s.ppo_update(rec_s, **hp), env_p.ppo_update(rec_p, **hp)
        assert torch.equal(out_s["grad"], out_p["grad"]), f"{case}, {what}: dev_grad differs from the plain binding's"
        assert bool(out_s["grad"][0, 0].any()) and bool(out_s["grad"][0, 1].any())
        for name in STAT_NAMES + ("grad_norm",):
            assert np.allclose(out_s[name], out_p[name], rtol=1e-6, atol=1e-6), (what, name)
        assert np.array_equal(out_s["rows"], out_p["rows"]) and np.array_equal(out_s["minibatches"], out_p["minibatches"])
    assert np.all(out_s["rows"][0, :, 0] == 62)
    env_s.close()
    env_p.close()


# ---- 2. several slabs against the twin ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_several_slabs_against_the_float64_twin(case):
    """slabs 2, 3, 5 and 32 (more than the inter kind's three tiles), one minibatch of all rows at lr 0: dev_grad per layer tensor within
    8x the float32-torch yardstick of the float64 twin, the statistics within 1e-6; 5 and 32 slabs give the same bytes on the inter
    kind, whose grid is min(3, slabs) = 3 under both."""
    _, act, layout = _nets(case)
    env = _env(case, spread=True, slabs=2)
    rec = env.collect(ref.T)
    order = _order(rec, 1)
    weights = ref.weights(env, 1)
    outs = {}
    for slabs in (2, 3, 5, 32):
        env.ppo_bind(spread=True, slabs=slabs)
        out = env.ppo_update(rec, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, order=order, grad=True)
        worst, misses = ref.check_against_twin(rec, order, out, weights, range(1), f"{case}, {slabs} slabs", act, act, layout)
        assert 0.0 < worst <= 8.0
        assert not misses, misses
        outs[slabs] = out
    assert torch.equal(outs[5]["grad"][0, 0], outs[32]["grad"][0, 0]), "the inter kind: 5 and 32 slabs differ on three tiles"
    for name in STAT_NAMES + ("grad_norm", "rows", "minibatches"):
        assert outs[5][name][0, 0].tobytes() == outs[32][name][0, 0].tobytes(), name
    env.close()


# ---- 3. one Adam step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_one_adam_step_at_three_slabs(case):
    env = _env(case, spread=True, slabs=3)
    rec = env.collect(ref.T)
    order = _order(rec, 1)
    w0 = ref.weights(env, 1)
    hp = dict(lr=np.array([1e-3]), grad_clip=np.array([0.05]), betas=(0.9, 0.999), eps=1e-8)
    out = env.ppo_update(rec, epochs=1, minibatch=ALL, order=order, grad=True, **hp)
    w1 = ref.weights(env, 1)
    ref.check_adam_step(env, out, w0, w1, hp, 1, f"{case}, 3 slabs")
    for r in ref.ROLES:
        assert all(not np.array_equal(x[0], y[0]) for x, y in zip(w0[r][0], w1[r][0])), f"a layer of {r} did not move"
    env.close()


# ---- 4. the loop ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("minibatch", [12, 40])
def test_the_loop_of_steps_equals_one_call_per_chunk(minibatch):
    """2 epochs of minibatches of 12 (a partial tile) and of 40 (a tile and a quarter) at 3 slabs in ONE call against the same chunks one
    call each on a twin handle: weights, moments and counters bit for bit -- a stale slab, a stale weight or a counter race would show
    here -- and every epoch's statistics equal to the chunks' own, added up by rows, within 1e-6."""
    case, E = "tanh40x24", 2
    env_a, env_b = _env(case, spread=True, slabs=3), _env(case, spread=True, slabs=3)
    rec_a, rec_b = _twin_records(env_a, env_b)
    order = _order(rec_a, E)
    start = ref.state(env_a, 1)
    out = env_a.ppo_update(rec_a, epochs=E, minibatch=minibatch, order=order, **HP_LOOP)
    n_rows = [int(order["first_" + k][1]) for k in ("inter", "intra")]
    n_chunks = [-(-n // minibatch) for n in n_rows]
    assert min(n_chunks) >= 2 and n_chunks[0] != n_chunks[1] and (minibatch != 40 or n_rows[0] % minibatch == 16)      # (96 = 40 + 40 + 16)
    sums = np.zeros((2, E, len(STAT_NAMES) + 1))
    for ep in range(E):
        for i in range(max(n_chunks)):
            o = env_b.ppo_update(rec_b, epochs=1, minibatch=ALL, order=ref.chunk_order(order, 1, minibatch, ep, i), **HP_LOOP)
            for kind_i in range(2):
                if i < n_chunks[kind_i]:
                    rows = min(minibatch, n_rows[kind_i] - i * minibatch)
                    sums[kind_i, ep] += rows * np.array([o[name][0, kind_i, 0] for name in STAT_NAMES + ("grad_norm",)])
    a, b = ref.state(env_a, 1), ref.state(env_b, 1)
    ref.same_state(a, b, f"minibatch {minibatch}: one call against one call per chunk")
    assert all(a[k].tobytes() != start[k].tobytes() for k in a if k.split("/")[-1][0] == "w"), "a weight matrix did not move"
    for kind_i, kind in enumerate(("inter", "intra")):
        assert int(a[f"{kind}/0/t"][0]) == int(a[f"v_{kind}/0/t"][0]) == E * n_chunks[kind_i]
        assert np.all(out["minibatches"][0, kind_i, :] == n_chunks[kind_i])
        for ep in range(E):
            for j, name in enumerate(STAT_NAMES + ("grad_norm",)):
                got, want = out[name][0, kind_i, ep], sums[kind_i, ep, j] / n_rows[kind_i]
                assert abs(got - want) <= 1e-6 * max(1.0, abs(want)), (kind, ep, name, got, want)
    env_a.close()
    env_b.close()


# ---- 5. determinism and the next collect ------------------------------------------------------------------------------------------------
def test_the_same_call_gives_the_same_bytes_and_the_next_collect_acts_on_the_trained_nets():
    """Twin handles at 3 slabs, a deterministic collect(8): the re-evaluated logp (probe_logp) equals the recorded one to the bit at
    unchanged weights; the same training call gives the same bytes on both; and a second collect, with no rebind, records what the
    float64 checks of tests/collect_ref.py accept for the weights read back."""
    case = "tanh40x24"
    layout = ref.CASES[case][2]
    env_a, env_b = _env(case, stochastic=False, spread=True, slabs=3), _env(case, stochastic=False, spread=True, slabs=3)
    rec_a, rec_b = _twin_records(env_a, env_b)
    order = _order(rec_a, 2)
    probe = env_a.ppo_update(rec_a, epochs=1, minibatch=40, lr=0.0, grad_clip=None, order=order, probe_logp=True)
    env_b.ppo_update(rec_b, epochs=1, minibatch=40, lr=0.0, grad_clip=None, order=order)
    new, old, mask = probe["logp"].cpu().numpy(), rec_a["logp"].cpu().numpy(), rec_a["mask_inter"].cpu().numpy() != 0
    assert np.array_equal(new[..., 0].view(np.int32), old[..., 0].view(np.int32))
    assert np.array_equal(new[..., 1:][mask].view(np.int32), old[..., 1:][mask].view(np.int32))
    assert np.all(probe["clip_frac"][:, :, 0] == 0.0)
    start = ref.state(env_a, 1)
    hp = dict(epochs=2, minibatch=40, lr=3e-3, order=order, grad=True)
    _same_call(env_a, env_a.ppo_update(rec_a, **hp), env_b, env_b.ppo_update(rec_b, **hp), "the same spread call on twin handles")
    trained = ref.state(env_a, 1)
    assert all(trained[k].tobytes() != start[k].tobytes() for k in trained if k.split("/")[-1][0] == "w")
    v = env_a.views()
    episode, step0 = v["episode_number"].cpu().numpy().copy(), v["step_number"].cpu().numpy().copy()
    rec2 = to_host(env_a.collect(3))
    seq = {r: ref.as_sequential([(w.cpu(), b.cpu()) for w, b in env_a.net_weights(r)], env_a.net_activation(r)) for r in ref.ROLES}
    for t in range(3):
        r, _ = cr.check_actor_record(rec2, t, seq["inter"], seq["intra"], False, ref.SEED, episode, step0 + t, layout)
        r["vf"] = cr.check_values(rec2["vf"][t], rec2["obs_inter"][t], rec2["obs_intra"][t], rec2["mask_intra"][t], seq["v_inter"], seq["v_intra"], layout)
        print(f"slot {t}: worst error / bound after the spread update: {r}")
    env_a.close()
    env_b.close()


# ---- 6. wide --------------------------------------------------------------------------------------------------------------------------
def test_verybig_under_spread_and_wide_against_the_float64_twin():
    """[512, 512, 512] tanh actors and critics, inter and intra, 3 slabs, one minibatch of all rows at lr 0: dev_grad within 8x the
    float32-torch yardstick of the float64 twin, the statistics within 1e-6; without ``wide`` the pair is refused as ppo_bind refuses it."""
    case = "verybig"
    _, act, layout = _nets(case)
    env = _env(case, spread=True, slabs=3, wide=True)
    rec = env.collect(ref.T)
    order = _order(rec, 1)
    out = env.ppo_update(rec, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, order=order, grad=True)
    worst, misses = ref.check_against_twin(rec, order, out, ref.weights(env, 1), range(1), "verybig, 3 slabs, wide", act, act, layout)
    assert 0.0 < worst <= 8.0
    assert not misses, misses
    for kind, dims in wd.kind_dims(wd.BEYOND[case][0], layout).items():
        assert env.ppo_member_layout(0, kind)["lds_bytes"] == wd.wide_lds_bytes(*dims)
    code, text = ref.refusal(lambda: env.ppo_bind(spread=True, slabs=3))
    assert code == E_STATE and "LDS" in text and "219648" in text, text
    env.close()


def test_spread_and_wide_equals_spread_alone_where_both_plans_hold():
    """tanh40x24, 3 slabs, two epochs of minibatches of 40 on twin handles, one bound wide: weights, moments, counters, statistics and
    dev_grad byte for byte"""
    case = "tanh40x24"
    env_w, env_p = _env(case, spread=True, slabs=3, wide=True), _env(case, spread=True, slabs=3)
    rec_w, rec_p = _twin_records(env_w, env_p)
    order = _order(rec_w, 2)
    hp = dict(epochs=2, minibatch=40, order=order, grad=True, **HP_LOOP)
    _same_call(env_w, env_w.ppo_update(rec_w, **hp), env_p, env_p.ppo_update(rec_p, **hp), "spread + wide against spread")
    assert env_w.ppo_member_layout(0, "inter")["lds_bytes"] < env_p.ppo_member_layout(0, "inter")["lds_bytes"]
    env_w.close()
    env_p.close()


# ---- 7. the boundary ------------------------------------------------------------------------------------------------------------------
def test_what_the_spread_binding_refuses():
    """A population of several members, a mixed population, intra nets per slice, bf16 nets, the head policy and slabs outside 1..256,
    by code and message; the handle's weights keep their bytes"""
    from intent_radio_sched_multi_slice_amd import _lib
    case = "tanh40x24"
    env = _env(case)
    nets, _, layout = _nets(case)
    w_before = ref.weights(env, 1)
    spread = lambda **kw: env.ppo_bind(spread=True, **kw)      # noqa: E731
    for slabs in (0, 257, -3):
        code, text = ref.refusal(lambda: spread(slabs=slabs))
        assert code == E_INVALID and f"slabs {slabs} (1..256)" in text, text
    # intra nets per slice
    env.set_policy_network(nets["inter"], [nets["intra"]] * env.S, stochastic=True, seed=1, intra_input=layout)
    code, text = ref.refusal(spread)
    assert code == E_STATE and "per slice" in text, text
    # bf16
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=1, intra_input=layout, precision="bf16")
    code, text = ref.refusal(spread)
    assert code == E_STATE and "bf16" in text, text
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=ref.SEED, intra_input=layout)
    w_after = ref.weights(env, 1)
    for r in ref.ROLES:
        for (w0, b0), (w1, b1) in zip(w_before[r][0], w_after[r][0]):
            assert w0.tobytes() == w1.tobytes() and b0.tobytes() == b1.tobytes(), f"a refused binding moved {r}"
    # the head policy: the plain entry's words
    env.set_policy(_lib.POLICY_HEAD_NETWORK)
    code, plain_text = ref.refusal(env.ppo_bind)
    code_s, text_s = ref.refusal(spread)
    assert code == code_s == E_STATE and "RANENV_POLICY_HEAD_NETWORK" in text_s
    assert text_s.split(": ", 1)[1] == plain_text.split(": ", 1)[1]
    env.set_policy(_lib.POLICY_NETWORK)
    # a population of three members, uniform and then mixed
    pop = ref.member_nets(case, 3)
    env.set_population(ref.FIRST)
    env.set_policy_network(pop["inter"], pop["intra"], stochastic=True, seed=1, intra_input=layout)
    env.set_value_network(pop["v_inter"], pop["v_intra"])
    code, text = ref.refusal(spread)
    assert code == E_STATE and "no population" in text and "3" in text, text
    env.ppo_bind()                             # (the plain binding still takes it)
    mixed = wd.mixed_nets()
    env.set_policy_network(mixed["inter"], mixed["intra"], stochastic=True, seed=1, intra_input=wd.MIXED_LAYOUT, mixed=True)
    env.set_value_network(mixed["v_inter"], mixed["v_intra"], mixed=True)
    code, text = ref.refusal(lambda: spread(wide=True))
    assert code == E_STATE and "does not train a mixed population" in text, text
    env.close()


def test_binds_replace_each_other_and_a_rebound_net_restarts():
    """A plain ppo_bind() behind a spread one gives the state and bytes of a fresh plain handle; a spread bind behind a plain one
    restarts the optimiser; actors re-bound under the spread binding restart their moments, their partner critics' and the two counters,
    and the critics keep their weights."""
    case = "tanh40x24"
    env_a, env_b = _env(case, spread=True, slabs=3), _env(case)
    rec_a, rec_b = _twin_records(env_a, env_b)
    order = _order(rec_a, 1)
    env_a.ppo_update(rec_a, epochs=1, minibatch=40, lr=0.0, order=order)       # (moves moments and counters, no weight)
    assert int(ref.state(env_a, 1)["inter/0/t"][0]) == 3
    env_a.ppo_bind()
    ref.same_state(ref.state(env_a, 1), ref.state(env_b, 1), "a plain bind behind a spread one")
    hp = dict(epochs=1, minibatch=40, order=order, grad=True, **HP_LOOP)
    _same_call(env_a, env_a.ppo_update(rec_a, **hp), env_b, env_b.ppo_update(rec_b, **hp), "the plain binding behind a spread one")
    # a spread bind behind the plain one, whose update has moved moments and counters
    moved = ref.state(env_a, 1)
    assert moved["inter/0/m"].any() and int(moved["intra/0/t"][0]) > 0
    env_a.ppo_bind(spread=True, slabs=5)
    fresh = ref.state(env_a, 1)
    for r in ref.ROLES:
        assert not fresh[f"{r}/0/m"].any() and not fresh[f"{r}/0/v"].any() and int(fresh[f"{r}/0/t"][0]) == 0, r
    assert all(fresh[k].tobytes() == moved[k].tobytes() for k in fresh if k.split("/")[-1][0] in "wb")
    # the two actors re-bound: both pairs restart
    env_a.ppo_update(rec_a, epochs=1, minibatch=40, lr=1e-3, order=order)
    before = ref.state(env_a, 1)
    assert before["v_inter/0/m"].any() and int(before["inter/0/t"][0]) == 3 and int(before["intra/0/t"][0]) > 3
    nets, _, layout = _nets(case)
    env_a.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=ref.SEED, intra_input=layout)
    after = ref.state(env_a, 1)
    for r in ref.ROLES:
        assert not after[f"{r}/0/m"].any() and not after[f"{r}/0/v"].any() and int(after[f"{r}/0/t"][0]) == 0, r
    for k in after:
        if k.startswith("v_") and k.split("/")[-1][0] in "wb":
            assert after[k].tobytes() == before[k].tobytes(), f"re-binding the actors moved {k}"
    out = env_a.ppo_update(rec_a, epochs=1, minibatch=40, lr=1e-3, order=order)
    assert int(ref.state(env_a, 1)["inter/0/t"][0]) == 3 and np.all(np.isfinite(out["grad_norm"]))
    env_a.close()
    env_b.close()
