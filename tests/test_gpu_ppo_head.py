"""The PPO update of the head policies on the device (ranenv_ppo_bind_head / ranenv_ppo_update_head) on the cases of tests/ppo_head_ref.py:
the gradient and the statistics of one minibatch against the float64 twin, one Adam step against the numpy float32 restatement, the loop
inside a launch against one-minibatch calls on a twin handle, row tails, entries outside the record, the re-evaluated log-probability at
unchanged weights, the next collect_head on the trained policy, determinism, the coexistence with the IBSched binding, refusals and re-binds.

The record of a test is a real ``collect_head()`` record whose logp carries ppo_head_ref's seeded noise (ppo_head_ref.with_noise).

Measured on one MI355X (printed by the tests; the bound on the gradient is 8 x the float32 twin's error, floor 1e-6):
    case    gradient, worst tensor   Adam step (weights, log_std, m, v)
    base    2.02                     0 ulp
    sb3     0.49                     0 ulp
    deg     1.66                     0 ulp
    inter   0.18                     0 ulp
    row tails at base (1, 31, 32, 33, 65 rows): 5.11, 0.92, 1.09, 1.06, 1.41; entries outside the record: 0.95
The five statistics of the 96-row calls lie within 2.4e-7 of the twin (bound 1e-6).  A ONE-row minibatch's approx-KL is 1.2e-5 and its
policy loss 7e-5 off the float64 twin -- one row's float32 forward, averaged with nothing -- so the row tails hold these two statistics
to 1e-6 plus ppo_head_ref.forward_bounds (the rigorous bound of policy_ref.mlp64 carried through logp: 2.3e-3 / 1.4e-2 at one row)."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import ppo_head_ref as hd
from tests import ppo_update_ref as ref
from tests.gpu_common import _ordered, need_gpu

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -3
ONE = dict(epochs=1, minibatch=hd.ALL, lr=0.0, grad_clip=None, clip=0.2, vf_coeff=0.5, ent_coeff=0.01)      # one minibatch, weights unchanged
TRAIN = dict(lr=3e-4, grad_clip=0.5, clip=0.2, vf_coeff=0.5, ent_coeff=0.01)


def _case_env(case, **kw):
    need_gpu()
    env, lay = hd.make_env(case, **kw)
    return env, lay, hd.with_noise(hd.collect(env, case))


def _dev(order, env):
    return order.to(env.device).contiguous()


@pytest.mark.parametrize("case", list(hd.CASES))
def test_gradient_and_statistics_of_one_minibatch_against_the_twin(case):
    """All 96 rows in one minibatch, weights unchanged (lr 0): dev_grad per tensor -- log_std a tensor of its own -- within 8 x the
    float32 twin's error, its padding exact zeros, the five statistics within 1e-6; the "inter" case runs under observation="inter"."""
    env, lay, rec = _case_env(case)
    order = hd.row_order(1)
    out = env.ppo_update_head(rec, order=_dev(order, env), grad=True, **ONE)
    worst, misses = hd.check_head_against_twin(case, rec, order, out, lay, case)
    assert not misses, misses
    assert 0.1 < out["clip_frac"][0] < 0.9
    after = hd.head_weights(env)
    assert torch.equal(after[1], lay[1]) and all(torch.equal(w, w0) and torch.equal(b, b0) for (w, b), (w0, b0) in zip(after[0] + after[2], lay[0] + lay[2]))
    assert int(env.ppo_head_state("actor")["t"].cpu()[0]) == 1
    env.close()


@pytest.mark.parametrize("case", list(hd.CASES))
def test_one_adam_step_is_the_float32_restatement_on_the_devices_own_gradient(case):
    """One minibatch with lr > 0 from zero moments: weights, log_std, m and v within 4 ulp of ppo_update_ref.adam_step_f32 applied to the
    call's own dev_grad; the joint norm covers log_std"""
    env, lay, rec = _case_env(case)
    S = hd.CASES[case][0]
    hp = dict(ONE, lr=1e-3, grad_clip=0.05)
    out = env.ppo_update_head(rec, order=_dev(hd.row_order(1), env), grad=True, eps=1e-5, **hp)
    g = hd.unpack_head_grad(out["grad"].cpu().numpy(), lay[0], lay[2], S, dtype=np.float32)
    none = np.zeros(0, dtype=np.float32)
    w0 = [(w.numpy(), b.numpy()) for w, b in lay[0] + lay[2]] + [(lay[1].numpy(), none)]
    want, norm, want_m, want_v = ref.adam_step_f32(w0, g["actor"] + g["critic"] + [(g["log_std"], none)], 1, 1e-3, 0.05, (0.9, 0.999), 1e-5, moments=True)
    assert abs(out["grad_norm"][0] - norm) <= 1e-9 * norm and norm > 0.05
    no_ls = float(np.sqrt(sum(float((x.astype(np.float64) ** 2).sum()) for pair in g["actor"] + g["critic"] for x in pair)))
    assert abs(out["grad_norm"][0] - no_ls) > 100 * 1e-9 * norm, "the bound above would not see a norm without log_std's gradient"
    a1, ls1, c1 = hd.head_weights(env)
    got = [(w.numpy(), b.numpy()) for w, b in a1 + c1] + [(ls1.numpy(), none)]
    worst = 0
    for (xw, xb), (yw, yb) in zip(want, got):
        for x, y in ((xw, yw), (xb, yb)):
            if x.size:
                worst = max(worst, int(np.abs(_ordered(x) - _ordered(y)).max()))
    st = {k: env.ppo_head_state(k) for k in ("actor", "critic", "log_std")}
    assert st["log_std"]["m"].numel() == S and int(st["actor"]["t"].cpu()[0]) == 1
    worst_mv = 0
    for name, want_x in (("m", want_m), ("v", want_v)):
        nets = ref.unpack_grad(np.concatenate([st["actor"][name].cpu().numpy(), st["critic"][name].cpu().numpy()]), lay[0], lay[2], dtype=np.float32)
        got_x = nets["actor"] + nets["critic"] + [(st["log_std"][name].cpu().numpy(), none)]
        for (xw, xb), (yw, yb) in zip(want_x, got_x):
            for x, y in ((xw, yw), (xb, yb)):
                if x.size:
                    worst_mv = max(worst_mv, int(np.abs(_ordered(x) - _ordered(y)).max()))
    print(f"{case}: Adam step, worst ulp distance {worst} (weights, log_std), {worst_mv} (moments)")
    assert worst <= 4 and worst_mv <= 4
    assert not np.array_equal(ls1.numpy(), lay[1].numpy())
    env.close()


@pytest.mark.parametrize("case", ["base", "inter"])
def test_the_loop_inside_a_launch_equals_one_minibatch_calls(case):
    """One call of 2 epochs x minibatch 12 equals 16 one-minibatch calls on a twin handle, bit for bit in weights, log_std, moments and
    counter: a stale weight or log_std read inside the launch fails here.  An epoch's clip fraction is the mean of its minibatches'.
    (On a real record sixteen steps of 3e-4 move the policy further than on the CPU file's synthetic one: only the first minibatch's
    clip fraction is held inside (0.1, 0.9) here; that file holds the twin's on all sixteen.)"""
    env, lay, rec = _case_env(case)
    twin_env, _, rec2 = _case_env(case)
    for k in rec:
        assert torch.equal(rec[k], rec2[k]), k
    order = hd.row_order(2)
    out = env.ppo_update_head(rec, epochs=2, minibatch=hd.MINIBATCH, order=_dev(order, env), **TRAIN)
    fr = []
    for ep in range(2):
        for c0 in range(0, hd.N, hd.MINIBATCH):
            one = twin_env.ppo_update_head(rec2, epochs=1, minibatch=hd.MINIBATCH, order=_dev(order[ep:ep + 1, c0:c0 + hd.MINIBATCH], twin_env), **TRAIN)
            fr.append(one["clip_frac"][0])
    a, b = hd.head_state(env), hd.head_state(twin_env)
    ref.same_state(a, b, case)
    assert int(a["actor/t"][0]) == 16 and a["log_std"].tobytes() != lay[1].numpy().tobytes()
    print(f"{case}: clip fractions of the 16 minibatches: {[round(float(f), 3) for f in fr]}")
    assert 0.1 < fr[0] < 0.9 and min(fr) > 0.0
    assert abs(out["clip_frac"][0] - np.mean(fr[:8])) < 1e-12 and out["minibatches"][1] == 8 and out["rows"][0] == hd.N
    env.close()
    twin_env.close()


def test_row_tails_and_entries_outside_the_record():
    """Minibatches of 1, 31, 32, 33 and 65 rows at the base case (advantages as given: a one-row minibatch has no deviation) against the
    twin; then a list in which -1, n_record and 2^31 - 1 stand between live rows: they count as rows and contribute nothing; a list of
    nothing else leaves weights and log_std byte for byte and advances the counter."""
    env, lay, rec = _case_env("base")
    hp = dict(ONE, adv_norm=None)
    full = hd.row_order(1)
    for nb in (1, 31, 32, 33, 65):
        order = full[:, :nb].contiguous()
        out = env.ppo_update_head(rec, order=_dev(order, env), grad=True, **hp)
        _, misses = hd.check_head_against_twin("base", rec, order, out, lay, f"{nb} rows", hp=dict(hd.HP, adv_norm=False), forward_bound=True)
        assert not misses, misses
    live = full[:, :40]
    dead = torch.tensor([-1, hd.N, 2 ** 31 - 1], dtype=torch.int32)
    mixed = torch.cat([live[0, :7], dead[:1], live[0, 7:33], dead[1:2], live[0, 33:], dead[2:]])[None, :].contiguous()
    out = env.ppo_update_head(rec, order=_dev(mixed, env), grad=True, **hp)
    assert out["rows"][0] == 40 and out["minibatches"][0] == 1
    _, misses = hd.check_head_against_twin("base", rec, mixed, out, lay, "entries outside the record", hp=dict(hd.HP, adv_norm=False),
                                           twin_order=live.contiguous(), scale=40.0 / 43.0, forward_bound=True)
    assert not misses, misses
    env.ppo_bind(head=True)              # (zero moments again: the calls above left theirs, which a step of lr > 0 would apply)
    before = hd.head_state(env)
    assert int(before["actor/t"][0]) == 0 and not before["actor/m"].any() and not before["log_std/v"].any()
    out = env.ppo_update_head(rec, order=_dev(dead[None, :].contiguous(), env), **dict(TRAIN, epochs=1, minibatch=2))
    after = hd.head_state(env)
    assert out["rows"][0] == 0 and out["minibatches"][0] == 2 and out["grad_norm"][0] == 0.0
    assert int(after["actor/t"][0]) == int(before["actor/t"][0]) + 2
    for k in before:
        if not k.endswith("/t"):
            assert after[k].tobytes() == before[k].tobytes(), k
    env.close()


def test_logp_at_unchanged_weights_is_the_collectors_to_the_bit():
    """A deterministic collect_head record, 96 epochs of one row each at lr 0: statistic [3] of epoch e is logp_old - logp of row e, and
    the float32 of the re-evaluated logp is the recorded one.  A stochastic, unmodified record: the first minibatch clips nothing."""
    need_gpu()
    env, lay = hd.make_env("base", stochastic=False)
    rec = hd.collect(env, "base")
    order = torch.arange(hd.N, dtype=torch.int32)[:, None].contiguous()
    out = env.ppo_update_head(rec, epochs=hd.N, minibatch=1, order=_dev(order, env), adv_norm=None, **{k: v for k, v in ONE.items() if k not in ("epochs", "minibatch")})
    lp_old = rec["logp"].reshape(-1).cpu().numpy()
    lp = lp_old.astype(np.float64) - out["kl"]
    assert np.array_equal(lp.astype(np.float32), lp_old) and np.all(out["clip_frac"] == 0.0) and np.all(out["rows"] == 1)
    env.close()
    env, lay = hd.make_env("base")
    rec = hd.collect(env, "base")
    out = env.ppo_update_head(rec, order=_dev(hd.row_order(1), env), **ONE)
    assert out["clip_frac"][0] == 0.0 and abs(out["kl"][0]) < 1e-6
    env.close()


def test_the_next_collect_head_acts_on_the_trained_policy_and_handles_are_deterministic():
    """Twin handles given the same update hold the same bytes; a third handle freshly bound to head_net_weights / head_log_std of the
    trained one records the same collect_head bytes as the trained one does"""
    env, lay, rec = _case_env("base")
    other, _, rec2 = _case_env("base")
    order = hd.row_order(2)
    for e, r in ((env, rec), (other, rec2)):
        e.ppo_update_head(r, epochs=2, minibatch=hd.MINIBATCH, order=_dev(order, e), **dict(TRAIN, lr=1e-2))
    ref.same_state(hd.head_state(env), hd.head_state(other), "twin handles")
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


def test_the_ibsched_binding_and_the_head_binding_leave_each_other_alone():
    """IBSched nets trained by ppo_update and head nets trained by ppo_update_head on one handle: each update leaves the other
    binding's weights, moments and counters byte for byte"""
    from intent_radio_sched_multi_slice_amd import _lib
    need_gpu()
    env = ref.native_workload(hd.B)
    nets = ref.member_nets("relu24", 1)
    layout = ref.CASES["relu24"][2]
    env.set_policy_network(nets["inter"][0], nets["intra"][0], stochastic=True, seed=ref.SEED, intra_input=layout)
    env.set_value_network(nets["v_inter"][0], nets["v_intra"][0])
    env.ppo_bind()
    env.reset()
    rec_ib = {k: v.clone() for k, v in env.collect(hd.T).items()}
    env.ppo_update(rec_ib, epochs=1, minibatch=32, seed=1)
    ib = ref.state(env, 1)
    env.enable_heads(hd.hr.usecase_of(env.tables))
    lay = hd.layers("base")
    env.set_head_policy_network(lay[0], "gauss_clip", lay[1], stochastic=True, seed=hd.SEED, activation="relu", allow_sorted=True)
    env.set_head_value_network(lay[2], activation="tanh")
    env.ppo_bind(head=True)
    rec = hd.with_noise(hd.collect(env, "base"))
    env.ppo_update_head(rec, epochs=1, minibatch=32, order=_dev(hd.row_order(1), env), **TRAIN)
    head = hd.head_state(env)
    assert int(head["actor/t"][0]) == 3 and head["log_std"].tobytes() != lay[1].numpy().tobytes()
    code, text = ref.refusal(lambda: env.ppo_update(rec_ib, epochs=1, minibatch=32, seed=1))
    assert code == E_STATE and "HEAD_NETWORK" in text
    env.set_policy(_lib.POLICY_NETWORK, _lib.INTRA_PF)
    ref.same_state(ib, ref.state(env, 1), "the IBSched binding across a head update")
    env.ppo_update(rec_ib, epochs=1, minibatch=32, seed=2)
    assert int(ref.state(env, 1)["inter/0/t"][0]) > int(ib["inter/0/t"][0])
    ref.same_state(head, hd.head_state(env), "the head binding across an IBSched update")
    env.close()


def test_refusals_leave_the_state_as_it_was():
    need_gpu()
    env, lay = hd.make_env("base", ppo=False)
    rec = hd.collect(env, "base")
    order = _dev(hd.row_order(1), env)
    upd = lambda **kw: env.ppo_update_head(rec, order=order, **dict(dict(TRAIN, epochs=1, minibatch=32), **kw))  # noqa: E731
    # update without a bind
    code, text = ref.refusal(upd)
    assert code == E_STATE and "ranenv_ppo_bind_head" in text
    # bf16
    env.set_head_policy_network(lay[0], "gauss_clip", lay[1], stochastic=True, seed=1, activation="relu", precision="bf16")
    code, text = ref.refusal(lambda: env.ppo_bind(head=True))
    assert code == E_STATE and "bf16" in text
    # GAUSS_TANH
    S = env.S
    tanh_actor = ref.layers_of(hd.hr.mlp([10 * S, 24, 2 * S], "relu", 5))
    env.set_head_policy_network(tanh_actor, "gauss_tanh", None, stochastic=True, seed=1, activation="relu")
    code, text = ref.refusal(lambda: env.ppo_bind(head=True))
    assert code == E_STATE and "GAUSS_TANH" in text
    # beyond the LDS plan
    wide = ref.layers_of(hd.hr.mlp([10 * S, 512, 512, 96, S], "tanh", 6))
    env.set_head_policy_network(wide, "gauss_clip", lay[1], stochastic=True, seed=1, activation="tanh")
    code, text = ref.refusal(lambda: env.ppo_bind(head=True))
    assert code == E_STATE and "LDS" in text
    assert ref.refusal(upd)[0] == E_STATE
    env.close()
    # no head critic
    env, lay = hd.make_env("base", bind=False)
    env.set_head_policy_network(lay[0], "gauss_clip", lay[1], stochastic=True, seed=1, activation="relu")
    code, text = ref.refusal(lambda: env.ppo_bind(head=True))
    assert code == E_STATE and "critic" in text
    env.close()
    # a bound handle: minibatch 0, epochs beyond the lists, the caps, an outgrowing re-bind
    env, lay, rec = _case_env("base")
    order = _dev(hd.row_order(1), env)
    before = hd.head_state(env)
    code, text = ref.refusal(lambda: upd(minibatch=0))
    assert code == E_INVALID and "minibatch" in text
    assert ref.refusal(lambda: env.ppo_update_head({k: v for k, v in rec.items() if k != "adv"}, epochs=1, order=order))[0] == E_INVALID
    from intent_radio_sched_multi_slice_amd._lib import RanEnvError
    for cap, word in (("PPO_ROW_EPOCHS_CAP", "rows x epochs"), ("PPO_STEPS_CAP", "optimiser steps")):
        setattr(env, cap, 2)            # (an instance attribute over the class's: this handle alone)
        with pytest.raises(RanEnvError, match=word):
            upd()
        delattr(env, cap)
    with pytest.raises(ValueError):
        env.ppo_bind(mixed=True, head=True)
    ref.same_state(before, hd.head_state(env), "refusals")
    env.PPO_ROW_EPOCHS_CAP, env.PPO_STEPS_CAP = 2, 2
    upd(force=True)
    del env.PPO_ROW_EPOCHS_CAP, env.PPO_STEPS_CAP
    assert int(hd.head_state(env)["actor/t"][0]) == 3
    bigger = ref.layers_of(hd.hr.mlp([10 * env.S, 64, 64, env.S], "relu", 8))
    env.set_head_policy_network(bigger, "gauss_clip", lay[1], stochastic=True, seed=1, activation="relu")
    code, text = ref.refusal(upd)
    assert code == E_STATE and "ranenv_ppo_bind_head" in text
    env.ppo_bind(head=True)
    upd()
    env.close()


def test_rebinding_the_critic_alone_restarts_the_whole_optimiser():
    env, lay, rec = _case_env("base")
    env.ppo_update_head(rec, epochs=1, minibatch=32, order=_dev(hd.row_order(1), env), **TRAIN)
    trained = hd.head_state(env)
    assert int(trained["actor/t"][0]) == 3 and trained["actor/m"].any() and trained["log_std/m"].any() and trained["critic/v"].any()
    env.set_head_value_network(lay[2], activation="tanh")
    after = hd.head_state(env)
    assert int(after["actor/t"][0]) == 0
    for which in ("actor", "critic", "log_std"):
        assert not after[f"{which}/m"].any() and not after[f"{which}/v"].any(), which
    for k in trained:
        if k == "log_std" or k.startswith("actor/w") or k.startswith("actor/b"):
            assert after[k].tobytes() == trained[k].tobytes(), f"re-binding the critic moved {k}"
    # the source of the rows is no part of the binding
    env.ppo_update_head(rec, epochs=1, minibatch=32, order=_dev(hd.row_order(1), env), **TRAIN)
    trained = hd.head_state(env)
    for source in (1, 0):
        assert env._lib.ranenv_set_head_policy_source(env._h, source) == 0
        ref.same_state(trained, hd.head_state(env), f"source {source}")
    env.close()
