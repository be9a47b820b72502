"""The SPREAD form of the head binding on the device (ranenv_ppo_bind_head_spread / ranenv_ppo_update_head; the kernels
ranenv_ppo_spread_head_pass / _reduce / _apply of ranenv_ppo_spread.hip): one slab against the plain head binding byte for byte; several
slabs against the float64 twin; one Adam step; the loop of optimiser steps against one call per minibatch; determinism and the next
collect_head(); the boundary to the other bindings.

Records, nets, tolerances and comparison functions are tests/ppo_head_ref.py's (``hd``), tests/ppo_update_ref.py's (``ref``) and
tests/ppo_head_shapes_ref.py's (``hg``): the 96-row record (three tiles) and the 288-row one (nine tiles), the gradient within 8 x the
float32 twin's error of the float64 twin (floor 1e-6), statistics 1e-6, Adam 4 ulp of ref.adam_step_f32 on the call's own dev_grad, the
norm 1e-9, byte equality between bindings and schedules.  S 1 is hd.CASES' "deg", S 16 its "sb3" and hg.CASES' "S16_edge".

Measured on one MI355X (printed by the tests):
    several slabs, base case, 288 rows, worst tensor's error / float32 twin's (bound 8): 2 slabs 1.16, 3 slabs 1.16, 5 slabs 1.17,
    9 slabs 1.16, 32 slabs 1.16; the five statistics within 2.9e-7 of the twin at every slab count (bound 1e-6)
    one Adam step at 3 slabs (weights and log_std / moments): 0 / 0 ulp at base, sb3, deg and inter"""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import ppo_bindings_shapes_ref as bs
from tests import ppo_head_ref as hd
from tests import ppo_update_ref as ref
from tests.gpu_common import need_gpu

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -3
ONE = dict(epochs=1, minibatch=hd.ALL, lr=0.0, grad_clip=None, clip=0.2, vf_coeff=0.5, ent_coeff=0.01)      # one minibatch, weights unchanged
TRAIN = dict(lr=3e-4, grad_clip=0.5, clip=0.2, vf_coeff=0.5, ent_coeff=0.01)
STAT_NAMES = ("policy_loss", "value_loss", "entropy", "kl", "clip_frac")


_spec, _env, _bind, _dev, _twins = bs.head_spec, bs.head_env, bs.head_bind, bs.to_dev, bs.head_twins


# ---- 1. one slab ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(hd.CASES) + ["S16_edge"])
def test_one_slab_gives_the_plain_head_bindings_gradient_byte_for_byte(case):
    """slabs=1: the tile order and the adds are the one-workgroup kernel's.  All 96 rows in one minibatch under adv_norm; lists of 1,
    31, 32, 33, 64 and 65 rows and a list with -1, n_record and 2^31 - 1 between live rows (advantages as given): dev_grad -- the
    log_std tail included -- byte for byte, the five statistics within 1e-12 (same adds in the same order; values are O(1))."""
    env_s, rec_s, env_p, rec_p, lay = _twins(case, 1, None)
    S = hd.spec(_spec(case))[0]
    full = hd.row_order(1)
    lists = [("all rows", full, ONE)]
    lists += [(f"{n} rows", full[:, :n].contiguous(), dict(ONE, adv_norm=None)) for n in (1, 31, 32, 33, 64, 65)]
    dead = torch.tensor([-1, hd.N, 2 ** 31 - 1], dtype=torch.int32)
    mixed = torch.cat([full[0, :7], dead[:1], full[0, 7:33], dead[1:2], full[0, 33:40], dead[2:]])[None, :].contiguous()
    lists.append(("entries outside the record", mixed, dict(ONE, adv_norm=None)))
    for what, order, hp in lists:
        out_s = env_s.ppo_update_head(rec_s, order=_dev(order, env_s), grad=True, **hp)
        out_p = env_p.ppo_update_head(rec_p, order=_dev(order, env_p), grad=True, **hp)
        gs, gp = out_s["grad"].cpu().numpy(), out_p["grad"].cpu().numpy()
        assert gs.tobytes() == gp.tobytes(), f"{case}, {what}: dev_grad differs from the plain head binding's"
        assert gs[:-S].any() and gs[-S:].any(), f"{case}, {what}: a zero gradient compares nothing"
        for name in STAT_NAMES:
            assert abs(out_s[name][0] - out_p[name][0]) <= 1e-12, (case, what, name, out_s[name][0], out_p[name][0])
        assert out_s["rows"][0] == out_p["rows"][0] and out_s["minibatches"][0] == out_p["minibatches"][0] == 1
    assert out_s["rows"][0] == 40
    env_s.close()
    env_p.close()


# ---- 2. several slabs against the twin ------------------------------------------------------------------------------------------------
def test_several_slabs_against_the_float64_twin():
    """The 288-row record (nine tiles) in one minibatch at lr 0 under 2, 3, 5, 9 and 32 slabs (grids 2, 3, 5, 9, 9): dev_grad per tensor
    -- log_std a tensor of its own -- within 8 x the float32 twin's error, the statistics within 1e-6; 9 and 32 slabs give the same bytes."""
    env, lay, rec = _env("base", 2, T=hd.T_LONG)
    assert rec["logp"].numel() == hd.N_LONG
    order = hd.row_order(1, n=hd.N_LONG)
    outs, worsts = {}, {}
    for slabs in (2, 3, 5, 9, 32):
        _bind(env, slabs)
        out = env.ppo_update_head(rec, order=_dev(order, env), grad=True, **ONE)
        worsts[slabs], misses = hd.check_head_against_twin("base", rec, order, out, lay, f"base, 288 rows, {slabs} slabs")
        assert not misses, misses
        assert out["rows"][0] == hd.N_LONG and 0.1 < out["clip_frac"][0] < 0.9
        outs[slabs] = out
    print("several slabs: worst ratios " + ", ".join(f"{s}: {w:.3g}" for s, w in worsts.items()))
    assert outs[9]["grad"].cpu().numpy().tobytes() == outs[32]["grad"].cpu().numpy().tobytes(), "9 and 32 slabs differ on nine tiles"
    for name in STAT_NAMES + ("grad_norm", "rows", "minibatches"):
        assert np.asarray(outs[9][name]).tobytes() == np.asarray(outs[32][name]).tobytes(), name
    assert outs[2]["grad"].cpu().numpy().tobytes() != outs[9]["grad"].cpu().numpy().tobytes(), "2 and 9 slabs add in another order"
    env.close()


# ---- 3. one Adam step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(hd.CASES))
def test_one_adam_step_at_three_slabs(case):
    """One minibatch of the 96 rows with lr > 0 from zero moments at 3 slabs: weights, log_std, m and v within 4 ulp of
    ref.adam_step_f32 on the call's own dev_grad; grad_norm within 1e-9 of the restatement's and further than 100 x that from the norm
    without log_std's gradient"""
    env, lay, rec = _env(case, 3)
    S = hd.CASES[case][0]
    hp = dict(ONE, lr=1e-3, grad_clip=0.05)
    out = env.ppo_update_head(rec, order=_dev(hd.row_order(1), env), grad=True, eps=1e-5, **hp)
    bs.check_head_adam_step(env, lay, out, S, f"{case}, 3 slabs", 1e-3, 0.05, 1e-5)
    env.close()


# ---- 4. the loop ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("minibatch", [12, 40])
def test_the_loop_of_steps_equals_one_call_per_minibatch(minibatch):
    """2 epochs of minibatches of 12 (one tile) and of 40 (two tiles; 96 = 40 + 40 + a 16-row tail) at 3 slabs in ONE call against one
    call per minibatch on a twin handle under the same binding: weights, log_std, moments and counter byte for byte -- a stale weight,
    log_std, running sum or counter across launches fails here -- and an epoch's statistics the row-weighted means of its minibatches'."""
    env, rec, twin_env, rec2, lay = _twins("base", 3, 3)
    order = hd.row_order(2)
    names = STAT_NAMES + ("grad_norm",)
    out = env.ppo_update_head(rec, epochs=2, minibatch=minibatch, order=_dev(order, env), **TRAIN)
    sums, n_mb = np.zeros((2, len(names))), 0
    for ep in range(2):
        for c0 in range(0, hd.N, minibatch):
            chunk = order[ep:ep + 1, c0:c0 + minibatch].contiguous()
            one = twin_env.ppo_update_head(rec2, epochs=1, minibatch=minibatch, order=_dev(chunk, twin_env), **TRAIN)
            assert one["rows"][0] == chunk.shape[1] and one["minibatches"][0] == 1
            sums[ep] += chunk.shape[1] * np.array([one[name][0] for name in names])
            n_mb += 1
    assert minibatch != 40 or hd.N % minibatch == 16
    a, b = hd.head_state(env), hd.head_state(twin_env)
    ref.same_state(a, b, f"minibatch {minibatch}: one call against one call per minibatch")
    assert int(a["actor/t"][0]) == n_mb and a["log_std"].tobytes() != lay[1].numpy().tobytes() and a["actor/w0"].tobytes() != lay[0][0][0].numpy().tobytes()
    for ep in range(2):
        assert out["minibatches"][ep] == n_mb // 2 and out["rows"][ep] == hd.N
        for j, name in enumerate(names):
            got, want = out[name][ep], sums[ep, j] / hd.N
            assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (ep, name, got, want)
    assert 0.0 < out["clip_frac"][0] < 1.0
    env.close()
    twin_env.close()


# ---- 5. determinism and the next collect ------------------------------------------------------------------------------------------------
def test_the_same_call_gives_the_same_bytes_and_the_next_collect_head_acts_on_the_trained_policy():
    """Two fresh handles at 3 slabs given the same call hold the same bytes, dev_grad and statistics included; a third handle freshly
    bound to head_net_weights / head_log_std of the trained one records the same collect_head bytes as the trained one does"""
    env, rec, other, rec2, lay = _twins("base", 3, 3)
    order = hd.row_order(2)
    outs = [e.ppo_update_head(r, epochs=2, minibatch=40, order=_dev(order, e), grad=True, **dict(TRAIN, lr=1e-2)) for e, r in ((env, rec), (other, rec2))]
    ref.same_state(hd.head_state(env), hd.head_state(other), "twin handles")
    for name in outs[0]:
        x, y = (o[name].cpu().numpy() if name == "grad" else np.asarray(o[name]) for o in outs)
        assert x.tobytes() == y.tobytes(), name
    trained = hd.head_weights(env)
    assert not torch.equal(trained[1], lay[1])
    fresh, _ = hd.make_env("base")
    hd.collect(fresh, "base")                        # (the same TTIs under the same nets and seed: the same env state)
    hd.bind_nets(fresh, "base", trained)
    want, got = hd.collect(env, "base"), hd.collect(fresh, "base")
    for k in want:
        assert want[k].cpu().numpy().tobytes() == got[k].cpu().numpy().tobytes(), k
    assert not torch.equal(want["action"], rec["action"])
    for e in (env, other, fresh):
        e.close()


# ---- 6. the boundary ------------------------------------------------------------------------------------------------------------------
def _after_name(text):
    return text.split(": ", 1)[1]


def test_what_the_spread_head_binding_refuses():
    """slabs outside 1..256 by code and message; GAUSS_TANH, a bf16 head net and a missing head critic in ranenv_ppo_bind_head's words,
    the handle's weights keeping their bytes; the ValueError combinations; the caps"""
    from intent_radio_sched_multi_slice_amd._lib import RanEnvError
    need_gpu()
    env, lay = hd.make_env("base", ppo=False)
    spread = lambda slabs=64, **kw: env.ppo_bind(head=True, spread=True, slabs=slabs, **kw)      # noqa: E731
    plain = lambda: env.ppo_bind(head=True)                               # noqa: E731
    critic0 = [(w.cpu().numpy().tobytes(), b.cpu().numpy().tobytes()) for w, b in env.head_net_weights("critic")]
    for slabs in (0, 257, -3):
        code, text = ref.refusal(lambda: spread(slabs=slabs))
        assert code == E_INVALID and f"slabs {slabs} (1..256)" in text, text
    S = env.S
    env.set_head_policy_network(lay[0], "gauss_clip", lay[1], stochastic=True, seed=1, activation="relu", precision="bf16")
    (code, text), (code_p, text_p) = ref.refusal(spread), ref.refusal(plain)
    assert code == code_p == E_STATE and "bf16" in text and _after_name(text) == _after_name(text_p), text
    tanh_actor = ref.layers_of(hd.hr.mlp([10 * S, 24, 2 * S], "relu", 5))
    env.set_head_policy_network(tanh_actor, "gauss_tanh", None, stochastic=True, seed=1, activation="relu")
    (code, text), (code_p, text_p) = ref.refusal(spread), ref.refusal(plain)
    assert code == code_p == E_STATE and "GAUSS_TANH" in text and _after_name(text) == _after_name(text_p), text
    wide = ref.layers_of(hd.hr.mlp([10 * S, 512, 512, 96, S], "tanh", 6))
    env.set_head_policy_network(wide, "gauss_clip", lay[1], stochastic=True, seed=1, activation="tanh")
    (code, text), (code_p, text_p) = ref.refusal(spread), ref.refusal(plain)
    assert code == code_p == E_STATE and "LDS" in text and _after_name(text) == _after_name(text_p), text
    assert critic0 == [(w.cpu().numpy().tobytes(), b.cpu().numpy().tobytes()) for w, b in env.head_net_weights("critic")]
    env.close()
    env, lay = hd.make_env("base", bind=False)
    env.set_head_policy_network(lay[0], "gauss_clip", lay[1], stochastic=True, seed=1, activation="relu")
    spread = lambda slabs=64, **kw: env.ppo_bind(head=True, spread=True, slabs=slabs, **kw)      # noqa: E731
    (code, text), (code_p, text_p) = ref.refusal(spread), ref.refusal(lambda: env.ppo_bind(head=True))
    assert code == code_p == E_STATE and "critic" in text and _after_name(text) == _after_name(text_p), text
    for (w, b), (w0, b0) in zip(env.head_net_weights("actor"), lay[0]):
        assert torch.equal(w.cpu(), w0) and torch.equal(b.cpu(), b0), "a refused binding moved the actor"
    for kw in (dict(wide=True), dict(mixed=True), dict(per_slice=True), dict(wide=True, spread=False), dict(mixed=True, spread=False), dict(per_slice=True, spread=False)):
        with pytest.raises(ValueError):
            env.ppo_bind(**dict(dict(head=True, spread=True, slabs=64), **kw))
    with pytest.raises(ValueError, match="spread and head"):      # (the spread form of the head binding takes its slab count)
        env.ppo_bind(head=True, spread=True)
    env.close()
    # the caps: rows x epochs does not apply under the spread head binding, the steps cap does
    env, lay, rec = _env("base", 3)
    order = _dev(hd.row_order(1), env)
    upd = lambda **kw: env.ppo_update_head(rec, order=order, **dict(dict(TRAIN, epochs=1, minibatch=32), **kw))  # noqa: E731
    env.PPO_ROW_EPOCHS_CAP = 2
    out = upd()
    assert out["minibatches"][0] == 3 and int(hd.head_state(env)["actor/t"][0]) == 3
    env.ppo_bind(head=True)
    with pytest.raises(RanEnvError, match="rows x epochs"):
        upd()
    _bind(env, 3)
    del env.PPO_ROW_EPOCHS_CAP
    env.PPO_STEPS_CAP = 2
    before = hd.head_state(env)
    with pytest.raises(RanEnvError, match="optimiser steps"):
        upd()
    ref.same_state(before, hd.head_state(env), "a refused update")
    upd(force=True)
    del env.PPO_STEPS_CAP
    assert int(hd.head_state(env)["actor/t"][0]) == 3
    env.close()


def test_head_binds_replace_each_other_and_a_rebound_actor_restarts():
    """A plain ppo_bind(head=True) behind a spread one gives a fresh plain handle's state and bytes; a spread bind behind a plain one
    restarts the optimiser; a head actor re-bound under the spread binding restarts the moments of both nets and of log_std and the
    counter, and one that outgrows what the bind allocated is refused until the next bind"""
    env_a, rec_a, env_b, rec_b, lay = _twins("base", 3, None)
    order = hd.row_order(1)
    env_a.ppo_update_head(rec_a, epochs=1, minibatch=40, order=_dev(order, env_a), **dict(TRAIN, lr=0.0))      # (moves moments and counter, no weight)
    moved = hd.head_state(env_a)
    assert int(moved["actor/t"][0]) == 3 and moved["log_std/m"].any() and moved["critic/v"].any()
    env_a.ppo_bind(head=True)
    ref.same_state(hd.head_state(env_a), hd.head_state(env_b), "a plain head bind behind a spread one")
    hp = dict(epochs=1, minibatch=40, grad=True, **TRAIN)
    out_a, out_b = env_a.ppo_update_head(rec_a, order=_dev(order, env_a), **hp), env_b.ppo_update_head(rec_b, order=_dev(order, env_b), **hp)
    ref.same_state(hd.head_state(env_a), hd.head_state(env_b), "the plain head binding behind a spread one")
    for name in out_a:
        x, y = (o[name].cpu().numpy() if name == "grad" else np.asarray(o[name]) for o in (out_a, out_b))
        assert x.tobytes() == y.tobytes(), name
    # a spread bind behind the plain one, whose update has moved weights, moments and the counter
    moved = hd.head_state(env_a)
    _bind(env_a, 5)
    fresh = hd.head_state(env_a)
    for k in fresh:
        if k.endswith("/m") or k.endswith("/v") or k.endswith("/t"):
            assert not fresh[k].any(), k
        else:
            assert fresh[k].tobytes() == moved[k].tobytes(), k
    # the actor re-bound under the spread binding
    env_a.ppo_update_head(rec_a, epochs=1, minibatch=40, order=_dev(order, env_a), **TRAIN)
    before = hd.head_state(env_a)
    assert int(before["actor/t"][0]) == 3 and before["critic/m"].any() and before["log_std/v"].any()
    env_a.set_head_policy_network(lay[0], "gauss_clip", lay[1], stochastic=True, seed=hd.SEED, activation="relu")
    after = hd.head_state(env_a)
    assert int(after["actor/t"][0]) == 0
    for which in ("actor", "critic", "log_std"):
        assert not after[f"{which}/m"].any() and not after[f"{which}/v"].any(), which
    for k in before:
        if k.startswith("critic/w") or k.startswith("critic/b"):
            assert after[k].tobytes() == before[k].tobytes(), f"re-binding the actor moved {k}"
    out = env_a.ppo_update_head(rec_a, epochs=1, minibatch=40, order=_dev(order, env_a), **TRAIN)
    assert int(hd.head_state(env_a)["actor/t"][0]) == 3 and np.isfinite(out["grad_norm"][0])
    bigger = ref.layers_of(hd.hr.mlp([10 * env_a.S, 64, 64, env_a.S], "relu", 8))
    env_a.set_head_policy_network(bigger, "gauss_clip", lay[1], stochastic=True, seed=1, activation="relu")
    code, text = ref.refusal(lambda: env_a.ppo_update_head(rec_a, epochs=1, minibatch=40, order=_dev(order, env_a), **TRAIN))
    assert code == E_STATE and ("bind again" in text or "ranenv_ppo_bind_head" in text), text
    _bind(env_a, 5)
    env_a.ppo_update_head(rec_a, epochs=1, minibatch=40, order=_dev(order, env_a), **TRAIN)
    env_a.close()
    env_b.close()


def test_both_spread_bindings_on_one_handle_leave_each_other_alone():
    """ppo_bind(spread=True) and ppo_bind(head=True, spread=True) on ONE handle: ppo_update gives the bytes of a handle that holds only
    the IBSched spread binding, ppo_update_head those of a handle that holds only the head spread binding -- no buffer is shared"""
    from intent_radio_sched_multi_slice_amd import _lib
    need_gpu()
    nets = ref.member_nets("relu24", 1)
    layout = ref.CASES["relu24"][2]
    lay = hd.layers("base")

    def ibsched(env):
        env.set_policy_network(nets["inter"][0], nets["intra"][0], stochastic=True, seed=ref.SEED, intra_input=layout)
        env.set_value_network(nets["v_inter"][0], nets["v_intra"][0])
        env.ppo_bind(spread=True, slabs=3)

    def head(env):
        env.enable_heads(hd.hr.usecase_of(env.tables))
        env.set_head_policy_network(lay[0], "gauss_clip", lay[1], stochastic=True, seed=hd.SEED, activation="relu", allow_sorted=True)
        env.set_head_value_network(lay[2], activation="tanh")
        env.ppo_bind(head=True, spread=True, slabs=5)

    both, only_ib, only_head = (ref.native_workload(hd.B) for _ in range(3))
    ibsched(both)
    both.reset()
    rec_ib = {k: v.clone() for k, v in both.collect(hd.T).items()}
    head(both)
    rec = hd.with_noise(hd.collect(both, "base"))
    order = hd.row_order(2)
    hp = dict(epochs=2, minibatch=40, **TRAIN)
    both.ppo_update_head(rec, order=_dev(order, both), **hp)
    head_state = hd.head_state(both)
    assert int(head_state["actor/t"][0]) == 6
    both.set_policy(_lib.POLICY_NETWORK, _lib.INTRA_PF)
    both.ppo_update(rec_ib, epochs=2, minibatch=40, seed=1)
    ib_state = ref.state(both, 1)
    assert int(ib_state["inter/0/t"][0]) == 6
    ref.same_state(head_state, hd.head_state(both), "the head spread binding across an IBSched spread update")
    ibsched(only_ib)
    only_ib.reset()
    only_ib.ppo_update(rec_ib, epochs=2, minibatch=40, seed=1)
    ref.same_state(ib_state, ref.state(only_ib, 1), "ppo_update beside the head spread binding")
    head(only_head)
    only_head.reset()
    only_head.ppo_update_head(rec, order=_dev(order, only_head), **hp)
    ref.same_state(head_state, hd.head_state(only_head), "ppo_update_head beside the IBSched spread binding")
    for e in (both, only_ib, only_head):
        e.close()
