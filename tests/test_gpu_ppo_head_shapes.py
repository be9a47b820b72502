"""The PPO update of the head policies on the device (ranenv_ppo_update_kernel_head) across the shape grid of
tests/ppo_head_shapes_ref.py -- S 6, 8, 10 (under both sources) and 16; widths up to 512, the LDS plan's edge, four hidden layers on
either side --, and, at ppo_head_ref's base case, a record of 288 rows: one minibatch of all of them (nine tiles, the advantage passes'
second stride) and minibatches of 257 and 31 rows inside one launch.

The record of a test is a real ``collect_head()`` record whose logp carries ppo_head_ref's seeded noise (ppo_head_ref.with_noise).  The
bound on a gradient tensor is 8 x the float32 twin's error (floor 1e-6), ``log_std`` a tensor of its own; the statistics lie within 1e-6.

Measured on one MI355X (printed by the tests):
    case             gradient, worst tensor   Adam step (weights, log_std, m, v)
    S10_sb3          0.24                     0 ulp
    S10_sb3_head     0.86                     0 ulp
    S16_edge         0.78                     0 ulp
    S8_deep_critic   0.98                     0 ulp
    S6_deep_actor    2.01                     0 ulp
    base, 288 rows in one minibatch: 1.16; 2 epochs of 257 + 31 rows: the state bit for bit that of four one-minibatch calls, clip
    fractions 0.46, 0.71, 0.74, 0.68 (an epoch's statistic is their ROW-weighted mean: 0.4896 for the first epoch, not 0.586)"""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import ppo_head_ref as hd
from tests import ppo_head_shapes_ref as hg
from tests import ppo_update_ref as ref
from tests.gpu_common import _ordered, need_gpu

pytestmark = pytest.mark.gpu

ONE = dict(epochs=1, minibatch=hd.ALL, lr=0.0, grad_clip=None, clip=0.2, vf_coeff=0.5, ent_coeff=0.01)      # one minibatch, weights unchanged
TRAIN = dict(lr=3e-4, grad_clip=0.5, clip=0.2, vf_coeff=0.5, ent_coeff=0.01)


def _case_env(name):
    need_gpu()
    env, lay = hg.make_env(name)
    return env, lay, hd.with_noise(hd.collect(env, hg.CASES[name]))


def _dev(order, env):
    return order.to(env.device).contiguous()


@pytest.mark.parametrize("name", list(hg.CASES))
def test_gradient_and_statistics_of_one_minibatch_against_the_twin(name):
    """All 96 rows in one minibatch, weights unchanged (lr 0): dev_grad per tensor -- log_std a tensor of its own -- within 8 x the
    float32 twin's error, its padding exact zeros, the five statistics within 1e-6; the launch's LDS bytes are the plan's formula."""
    env, lay, rec = _case_env(name)
    assert env.ppo_head_layout()["lds_bytes"] == hg.lds_bytes(name)
    order = hd.row_order(1)
    out = env.ppo_update_head(rec, order=_dev(order, env), grad=True, **ONE)
    worst, misses = hd.check_head_against_twin(hg.CASES[name], rec, order, out, lay, name)
    assert not misses, misses
    assert 0.1 < out["clip_frac"][0] < 0.9
    after = hd.head_weights(env)
    assert torch.equal(after[1], lay[1]) and all(torch.equal(w, w0) and torch.equal(b, b0) for (w, b), (w0, b0) in zip(after[0] + after[2], lay[0] + lay[2]))
    assert int(env.ppo_head_state("actor")["t"].cpu()[0]) == 1
    env.close()


@pytest.mark.parametrize("name", list(hg.CASES))
def test_one_adam_step_is_the_float32_restatement_on_the_devices_own_gradient(name):
    """One minibatch with lr > 0 from zero moments: weights, log_std, m and v within 4 ulp of ppo_update_ref.adam_step_f32 applied to the
    call's own dev_grad; the joint norm covers log_std"""
    env, lay, rec = _case_env(name)
    S = hg.CASES[name][0]
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
    for which, want_x in (("m", want_m), ("v", want_v)):
        nets = ref.unpack_grad(np.concatenate([st["actor"][which].cpu().numpy(), st["critic"][which].cpu().numpy()]), lay[0], lay[2], dtype=np.float32)
        got_x = nets["actor"] + nets["critic"] + [(st["log_std"][which].cpu().numpy(), none)]
        for (xw, xb), (yw, yb) in zip(want_x, got_x):
            for x, y in ((xw, yw), (xb, yb)):
                if x.size:
                    worst_mv = max(worst_mv, int(np.abs(_ordered(x) - _ordered(y)).max()))
    print(f"{name}: Adam step, worst ulp distance {worst} (weights, log_std), {worst_mv} (moments)")
    assert worst <= 4 and worst_mv <= 4
    assert not np.array_equal(ls1.numpy(), lay[1].numpy())
    env.close()


def test_one_step_past_the_edge_is_refused():
    """[512, 480] on both sides at S 16: one step of 32 past S16_edge, beyond the plan; the bind says so"""
    need_gpu()
    S, _, aa, _, ca = hg.CASES["S16_edge"][:5]
    env, lay = hg.make_env("S16_edge", bind=False)
    env.set_head_policy_network(ref.layers_of(hd.hr.mlp([10 * S] + hg.PAST_EDGE + [S], aa, 6)), "gauss_clip", lay[1], stochastic=True, seed=1, activation=aa)
    env.set_head_value_network(ref.layers_of(hd.hr.mlp([10 * S] + hg.PAST_EDGE + [1], ca, 7)), activation=ca)
    code, text = ref.refusal(lambda: env.ppo_bind(head=True))
    assert code == -3 and "LDS" in text, (code, text)
    env.close()


def _long_env():
    need_gpu()
    env, lay = hd.make_env("base")
    rec = hd.with_noise(hd.collect(env, "base", T=hg.T_LONG))
    assert rec["logp"].numel() == hg.N_LONG
    return env, lay, rec


def test_one_minibatch_of_288_rows_against_the_twin():
    """Base case, B 12 x T 24: all 288 rows in one minibatch under adv_norm -- nine tiles, and the advantage passes take a second stride
    (tests/test_ppo_head_shapes_cpu.py: statistics over the first 256 entries alone lie > 1000 x the yardstick away)."""
    env, lay, rec = _long_env()
    order = hd.row_order(1, n=hg.N_LONG)
    out = env.ppo_update_head(rec, order=_dev(order, env), grad=True, **ONE)
    worst, misses = hd.check_head_against_twin("base", rec, order, out, lay, "base, 288 rows")
    assert not misses, misses
    assert out["rows"][0] == hg.N_LONG and 0.1 < out["clip_frac"][0] < 0.9
    env.close()


def test_minibatches_of_257_and_31_rows_inside_a_launch_equal_one_minibatch_calls():
    """One call of 2 epochs x minibatch 257 on the 288-row record -- a 257-row and a 31-row minibatch per epoch -- equals the same four
    minibatches as one-minibatch calls on a twin handle, bit for bit in weights, log_std, moments and counter; every minibatch's clip
    fraction lies inside (0.1, 0.9)."""
    env, lay, rec = _long_env()
    twin_env, _, rec2 = _long_env()
    for k in rec:
        assert torch.equal(rec[k], rec2[k]), k
    order = hd.row_order(2, n=hg.N_LONG)
    out = env.ppo_update_head(rec, epochs=2, minibatch=hg.LONG_MINIBATCH, order=_dev(order, env), **TRAIN)
    fr, rows = [], []
    for ep, c0, nb in hg.long_chunks(order):
        one = twin_env.ppo_update_head(rec2, epochs=1, minibatch=hd.ALL, order=_dev(order[ep:ep + 1, c0:c0 + nb], twin_env), **TRAIN)
        fr.append(one["clip_frac"][0])
        rows.append(int(one["rows"][0]))
    a, b = hd.head_state(env), hd.head_state(twin_env)
    ref.same_state(a, b, "base, 2 epochs of 257 + 31 rows")
    assert rows == [257, 31, 257, 31] and int(a["actor/t"][0]) == 4 and a["log_std"].tobytes() != lay[1].numpy().tobytes()
    print(f"base, 288 rows: clip fractions of the 4 minibatches: {[round(float(f), 3) for f in fr]}")
    assert all(0.1 < f < 0.9 for f in fr), fr
    # (an epoch's statistics are ROW-weighted means, include/ranenv.h: with minibatches of unequal size not the mean of theirs)
    assert abs(out["clip_frac"][0] - (257 * fr[0] + 31 * fr[1]) / hg.N_LONG) < 1e-12 and abs(out["clip_frac"][1] - (257 * fr[2] + 31 * fr[3]) / hg.N_LONG) < 1e-12
    assert abs(out["clip_frac"][0] - np.mean(fr[:2])) > 1e-3, "minibatches of equal clip fraction would not tell the two means apart"
    assert out["minibatches"][1] == 2 and out["rows"][0] == out["rows"][1] == hg.N_LONG
    env.close()
    twin_env.close()
