"""The SAC update on the device (ranenv_sac.hip) across the shape grid of tests/sac_update_shapes_ref.py -- S 3, 8, 10 and 16; widths up
to 512, the LDS plan's edge, five layers on both sides --, and, at sac_update_ref's base case, tile walks of five tiles under 1, 2, 3, 5
and 32 slabs and the high words of the Philox counter and key.

One env per case, B 12, a ring of 4 TTIs, 96 rows.  The bound on a gradient tensor is 8 x the float32 twin's error (floor 1e-6):
tests/sac_update_ref.py states the yardstick; tests/sac_update_shapes_ref.py states the conditions on the inputs, tests/test_sac_update_shapes_cpu.py
holds them on the synthetic rows, and the tests here compute the tie margin on the ring's rows themselves.

Measured on one MI355X (worst device / yardstick ratio over the gradient tensors; the bound is 8; printed by the tests):
    case            ring rows   synthetic rows   lr 1e-2, actor   tie margin of the ring rows (the condition: >= 1000)
    S3_96x160_33    0.39        0.20                              3.3e5
    S8_255_511x3    1.09        0.16                              1.1e4
    S10_sb3         0.32        0.22             0.32             3.3e5
    S16_edge        0.72        0.34                              1.3e4
    S16_deep        0.53        0.35             1.00             5.8e3
    base, 129 / 160 rows under 1, 2, 3 and 32 slabs: 0.93 - 0.98, dev_target 0.07 - 0.08; 32 and 5 slabs: the same bytes
    base under seed (5 << 32) | 9, draw 4, first_row 2^32 + 7: 0.93, dev_target 0.05 (tie margin 5.4e3)
One Adam step: 0 ulp from the numpy restatement in every weight, moment and the scalar at every case; polyak: bit for bit.
The ring's rows alone would not do: at S10_sb3 the first critic is the smaller one on all 96 of them, which is why every case also
runs on the synthetic rows, where each critic is the smaller one on at least a quarter."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import ppo_update_ref as pu
from tests import sac_update_ref as su
from tests import sac_update_shapes_ref as sg
from tests.gpu_common import _ordered, need_gpu

pytestmark = pytest.mark.gpu

LEC = float(np.float32(np.log(su.ENT_INIT)))
STEP = dict(gamma=su.GAMMA, tau=su.TAU, seed=su.SEED, draw=su.DRAW)
BIND = "auto_%g" % su.ENT_INIT


def _env(case, **kw):
    need_gpu()
    return su.make_env(case, **kw)


def _ring_rows(name, env, n=su.ROWS, **noise):
    """``n`` rows of the ring under the case's recorded sample seed; fails loudly if a row of them lies near a tie of the live critics"""
    case = sg.CASES[name]
    batch = su.sample(env, n, seed=sg.SAMPLE_SEED[name])
    ratio, gap, err = sg.tie_margin(case, batch, sg.five(su.device_nets(env)), **noise)
    print(f"{name}: ring rows, tie margin {ratio:.3g} (smallest |Q1 - Q2| {gap:.3g}, largest float32 error of a Q {err:.3g})")
    assert ratio >= sg.TIE_MARGIN, (f"{name}: a ring row under sample seed {sg.SAMPLE_SEED[name]} lies near a tie of the critics: choose another "
                                    f"seed in sac_update_shapes_ref.SAMPLE_SEED", ratio, gap, err)
    return batch


@pytest.mark.parametrize("name", list(sg.CASES))
def test_gradients_and_statistics_of_one_step_against_the_twin(name):
    """All 96 rows in one minibatch at lr 0: every gradient tensor and log_ent_coef's within 8 x the float32 twin's error, the padding
    of dev_grad exact zeros (unpack_grad), the eight statistics within their bound.  Once on the synthetic rows that the CPU file holds
    to every condition, once on a ``replay_sample`` of the real ring, whose tie margin is computed here from the device's own nets."""
    case = sg.CASES[name]
    env, _ = _env(case)
    assert env.sac_layout()["lds_bytes"] == sg.lds_bytes(name)
    synthetic = {k: v.to(env.device) for k, v in su.synthetic_batch(case).items()}
    sg.step_against_twin(case, env, synthetic, su.ROWS, 0.0, name + " (synthetic rows)")
    assert all(int(env.sac_state(k)["t"].cpu()[0]) == 1 for k in ("actor", "q1", "q2", "log_ent_coef"))
    env.sac_bind(ent_coef=BIND)
    batch = _ring_rows(name, env)
    sg.step_against_twin(case, env, batch, su.ROWS, 0.0, name + " (ring rows)")
    env.close()


def test_one_step_past_the_edge_is_refused():
    """[512, 480] on both sides at S 16: one step of 32 past S16_edge, beyond the plan; the bind says so and binds nothing"""
    from tests import head_policy_ref as hr
    S, _, aact, _, qact = sg.CASES["S16_edge"]
    env, _ = _env(sg.CASES["S16_edge"], bind=False)
    env.set_head_policy_network(hr.mlp([10 * S] + sg.PAST_EDGE + [2 * S], aact, 1), "gauss_tanh", stochastic=True, seed=1)
    env.set_sac_critics(hr.mlp([11 * S] + sg.PAST_EDGE + [1], qact, 2), hr.mlp([11 * S] + sg.PAST_EDGE + [1], qact, 3))
    got, text = pu.refusal(lambda: env.sac_bind())
    assert got == -3 and "LDS" in text, (got, text)
    got, text = pu.refusal(lambda: env.sac_update(su.sample(env, 32), 1, minibatch=32))
    assert got == -3 and "ranenv_sac_bind" in text, (got, text)
    env.close()


def _ulp(a, b):
    return int(np.abs(_ordered(np.ascontiguousarray(a, dtype=np.float32)) - _ordered(np.ascontiguousarray(b, dtype=np.float32))).max()) if np.size(a) else 0


@pytest.mark.parametrize("name", list(sg.CASES))
def test_one_adam_step_and_polyak_bit_for_bit(name):
    """One step at lr 1e-3 from zero moments: weights, m and v of actor, q1, q2 and the scalar 0 ulp from adam_step_f32 (no clip) on the
    device's own dev_grad; the targets bit for bit the numpy float32 polyak rule on the device's new critics."""
    case = sg.CASES[name]
    env, _ = _env(case)
    batch = su.sample(env, su.ROWS, seed=sg.SAMPLE_SEED[name])
    w0 = su.device_nets(env)
    out = env.sac_update(batch, 1, minibatch=su.ROWS, lr=1e-3, grad=True, **STEP)
    w1 = su.device_nets(env)
    g = su.unpack_grad(out["grad"].cpu().numpy(), w0["actor"], w0["q1"], dtype=np.float32)
    worst = 0
    for tensor in su.TENSORS:
        start = [(w.numpy(), b.numpy()) for w, b in w0[tensor]]
        want, _, want_m, want_v = pu.adam_step_f32(start, g[tensor], 1, 1e-3, 0.0, moments=True)
        st = env.sac_state(tensor)
        got_m = pu.unpack_grad(st["m"].cpu().numpy(), w0[tensor], [], dtype=np.float32)["actor"]
        got_v = pu.unpack_grad(st["v"].cpu().numpy(), w0[tensor], [], dtype=np.float32)["actor"]
        for want_x, got_x in ((want, [(w.numpy(), b.numpy()) for w, b in w1[tensor]]), (want_m, got_m), (want_v, got_v)):
            for (xw, xb), (yw, yb) in zip(want_x, got_x):
                worst = max(worst, _ulp(xw, yw), _ulp(xb, yb))
        assert int(st["t"].cpu()[0]) == 1
        assert any(not torch.equal(a, b) for (a, _), (b, _) in zip(w0[tensor], w1[tensor])), tensor
    ge = np.array([g["log_ent_coef"]], dtype=np.float32)
    none = np.zeros(0, dtype=np.float32)
    want, _, want_m, want_v = pu.adam_step_f32([(np.array([LEC], dtype=np.float32), none)], [(ge, none)], 1, 1e-3, 0.0, moments=True)
    st = env.sac_state("log_ent_coef")
    worst = max(worst, _ulp(want[0][0], env.sac_log_ent_coef().cpu().numpy()), _ulp(want_m[0][0], st["m"].cpu().numpy()), _ulp(want_v[0][0], st["v"].cpu().numpy()))
    print(f"{name}: Adam step, worst ulp distance from the numpy restatement {worst}")
    assert worst == 0
    omt, tf = np.float32(1.0 - su.TAU), np.float32(su.TAU)
    for q, tq in (("q1", "q1_target"), ("q2", "q2_target")):
        for (t0, tb0), (w, b), (t1, tb1) in zip(w0[tq], w1[q], w1[tq]):
            assert (omt * t0.numpy() + tf * w.numpy()).astype(np.float32).tobytes() == t1.numpy().tobytes(), tq
            assert (omt * tb0.numpy() + tf * b.numpy()).astype(np.float32).tobytes() == tb1.numpy().tobytes(), tq
        assert any(not torch.equal(t0, t1) for (t0, _), (t1, _) in zip(w0[tq], w1[tq]))
    env.close()


@pytest.mark.parametrize("name", ("S10_sb3", "S16_deep"))
def test_the_actor_pass_sees_the_updated_critics(name):
    """One step at lr 1e-2: the actor's gradient meets the yardstick against the twin's full step, whose actor pass runs under the
    critics the step has just updated (tests/test_sac_update_cpu.py: under the stale ones the gradient lies > 1000 x outside)."""
    case = sg.CASES[name]
    env, _ = _env(case)
    batch = _ring_rows(name, env)
    sg.step_against_twin(case, env, batch, su.ROWS, 1e-2, f"{name} lr 1e-2", names=("actor",), stats=False)
    env.close()


def test_the_loop_inside_a_call_is_the_sequence_of_one_step_calls():
    """S10_sb3: one call of 3 steps of 40 rows against 3 one-step calls on a twin handle with first_row advanced: the five nets, the
    moments, the scalar and the counters bit for bit, and the statistics."""
    name = "S10_sb3"
    env, _ = _env(sg.CASES[name])
    other, _ = _env(sg.CASES[name])
    n = 40
    batch = su.sample(env, 3 * n, seed=sg.SAMPLE_SEED[name])
    pu.same_state(su.device_state(env), su.device_state(other), "twin handles before the update")
    whole = env.sac_update(batch, 3, minibatch=n, lr=1e-3, **STEP)
    for g in range(3):
        part = other.sac_update({k: v[g * n:(g + 1) * n] for k, v in batch.items()}, 1, minibatch=n, lr=1e-3, first_row=g * n, **STEP)
        assert all(part[k][0] == whole[k][g] for k in sg.stat_names()), (g, {k: (part[k][0], whole[k][g]) for k in sg.stat_names()})
    a, b = su.device_state(env), su.device_state(other)
    pu.same_state(a, b, "3 steps in one call and in three")
    assert int(a["actor/t"][0]) == int(a["q1/t"][0]) == int(a["q2/t"][0]) == int(a["log_ent_coef/t"][0]) == 3
    env.close()
    other.close()


def test_uneven_tile_walks():
    """Base case, 160 rows of the ring (separated by sac_update_ref.conditions' rigorous bound): minibatches of 129 and 160 rows -- five
    tiles, the last of one row at 129 -- under 1, 2, 3 and 32 slabs, each against the twin: under 2 slabs one workgroup walks three
    tiles and the other two, under 3 slabs two, two and one.  Handles bound with 32 slabs and with exactly 5 give the same bytes in
    dev_grad, dev_target and the statistics: only used slabs are summed."""
    env, _ = _env("base")
    most = max(sg.TILE_ROWS)
    batch = su.sample(env, most, seed=sg.TILE_SAMPLE_SEED)
    for n in sg.TILE_ROWS:
        cond = su.conditions("base", su.head(batch, n), sg.five(su.device_nets(env)), LEC)
        print(f"base, {n} rows: {cond}")
        assert cond["separated"], cond
    for slabs in sg.TILE_SLABS:
        for n in sg.TILE_ROWS:
            env.sac_bind(ent_coef=BIND, slabs=slabs)
            sg.step_against_twin("base", env, batch, n, 0.0, f"slabs {slabs} rows {n}", target=True)
    for n in sg.TILE_ROWS:
        assert (n + 31) // 32 == sg.TILE_EXACT
        got = []
        for slabs in (32, sg.TILE_EXACT):
            env.sac_bind(ent_coef=BIND, slabs=slabs)
            out = env.sac_update(su.head(batch, n), 1, minibatch=n, lr=0.0, grad=True, target=True, **dict(STEP, tau=0.0))
            got.append((out["grad"].cpu().numpy().tobytes(), out["target"].cpu().numpy().tobytes(), np.array([out[k][0] for k in sg.stat_names()]).tobytes()))
        assert got[0] == got[1], f"{n} rows: 32 slabs and {sg.TILE_EXACT} slabs differ"
    env.close()


def test_the_high_words_of_the_philox_counter_and_key():
    """Base case, one step at lr 0 under seed (5 << 32) | 9, draw 4, first_row 2^32 + 7: gradients, statistics and dev_target against
    the twin called with the same three values.  tests/test_sac_update_shapes_cpu.py shows that a seed or a first_row cut to its low word
    moves every row's draws and puts the twin's gradients and targets > 1000 x the yardstick away."""
    env, _ = _env("base")
    batch = su.sample(env, su.ROWS, seed=sg.PHILOX_SAMPLE_SEED)
    ratio, gap, err = sg.tie_margin("base", batch, sg.five(su.device_nets(env)), **sg.PHILOX)
    print(f"base under {sg.PHILOX}: tie margin {ratio:.3g}")
    assert ratio >= sg.TIE_MARGIN, (ratio, gap, err)
    sg.step_against_twin("base", env, batch, su.ROWS, 0.0, "base, high Philox words", target=True, **sg.PHILOX)
    # ... and the low words alone give other targets on the device too
    env.sac_bind(ent_coef=BIND)
    full = env.sac_update(batch, 1, minibatch=su.ROWS, lr=0.0, target=True, **dict(STEP, **sg.PHILOX))["target"].cpu().numpy()
    for cut in (dict(sg.PHILOX, seed=sg.PHILOX["seed"] & sg.LOW32), dict(sg.PHILOX, first_row=sg.PHILOX["first_row"] & sg.LOW32)):
        env.sac_bind(ent_coef=BIND)
        low = env.sac_update(batch, 1, minibatch=su.ROWS, lr=0.0, target=True, **dict(STEP, **cut))["target"].cpu().numpy()
        live = batch["done"].cpu().numpy() == 0          # (a terminal row's target is its reward)
        assert live.any() and (low[live] != full[live]).all(), cut
    env.close()
