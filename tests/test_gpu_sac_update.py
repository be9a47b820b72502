"""The SAC update on the device (ranenv_sac_bind / ranenv_sac_update) on the cases of tests/sac_update_ref.py: the gradients and the
statistics of one step against the torch twin, row tails and slab counts, one Adam step and the polyak rule against numpy float32
restatements bit for bit, the loop inside a call against one-step calls on a twin handle, the actor pass under the critics the same step
updated, the wiring to ``sac_targets`` and ``collect_replay``, a fixed coefficient, refusals, re-binds and the coexistence with the
IBSched PPO binding.

A test's batch is a ``replay_sample`` of a ring that a real ``collect_replay`` filled (B 12, four TTIs).  The bound on a gradient tensor
is 8 x the float32 twin's error (floor 1e-6): tests/sac_update_ref.py states the yardstick; the tests print the ratios they find.

Measured on one MI355X (worst device / yardstick ratio over the gradient tensors; the bound is 8):
    case        ring rows   synthetic rows   lr 1e-2, actor
    base        1.22        0.18             1.00
    deg         2.95        0.91
    stride      0.45        0.14             0.42
    two_pair    0.27        0.16
    base, minibatches of 1 / 31 / 32 / 33 / 65 / 96 rows: 1.9 - 2.1 / 0.67 / 0.67 / 1.0 / 1.3 / 1.2, the same under 1, 2 and 32 slabs
One Adam step: 0 ulp from the numpy restatement in every weight, moment and the scalar; polyak: bit for bit."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import ppo_update_ref as pu
from tests import sac_update_ref as su
from tests.gpu_common import _ordered, need_gpu

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -3
LEC = float(np.float32(np.log(su.ENT_INIT)))
STEP = dict(gamma=su.GAMMA, tau=su.TAU, seed=su.SEED, draw=su.DRAW)


def _env(case, **kw):
    need_gpu()
    return su.make_env(case, **kw)


def _five(nets):
    """(actor, q1, q2, q1_target, q2_target) layer lists of a ``device_nets`` dict"""
    return tuple(nets[k] for k in ("actor", "q1", "q2", "q1_target", "q2_target"))


def _against_twin(case, env, batch, n, lr, what, names=su.TENSORS + ("log_ent_coef",), stats=True):
    """One step on the first n rows from the nets as they are on the device now: dev_grad and the statistics against the twins"""
    start = _five(su.device_nets(env))
    lec = float(env.sac_log_ent_coef().cpu()[0])
    out = env.sac_update(su.head(batch, n), 1, minibatch=n, lr=lr, grad=True, **STEP)
    dev = su.unpack_grad(out["grad"].cpu().numpy(), start[0], start[1])
    kw = dict(steps=1, minibatch=n, lr=lr)
    t64, t32 = su.twin(case, su.head(batch, n), start, lec, **kw), su.twin(case, su.head(batch, n), start, lec, torch.float32, **kw)
    worst = su.check_grads(dev, t64["grad"], t32["grad"], what, names)
    if stats:
        su.check_stats([out[k][0] for k in _stat_names()], t64["stats"][0], t32["stats"][0], what)
    return worst, out, start


def _stat_names():
    from intent_radio_sched_multi_slice_amd import _lib
    return _lib.SAC_STATS


@pytest.mark.parametrize("case", list(su.CASES))
def test_gradients_and_statistics_of_one_step_against_the_twin(case):
    """All 96 rows in one minibatch at lr 0: every gradient tensor and log_ent_coef's within 8 x the float32 twin's error, the padding
    of dev_grad exact zeros (unpack_grad), the eight statistics within their bound; no row of the batch is near a tie of the critics.
    Once on the ring's rows, once on the CPU tests' synthetic rows."""
    env, _ = _env(case)
    batch = su.sample(env, su.ROWS)
    cond = su.conditions(case, batch, _five(su.device_nets(env)), LEC)
    print(case, cond)
    assert cond["separated"], cond
    _against_twin(case, env, batch, su.ROWS, 0.0, case)
    assert all(int(env.sac_state(k)["t"].cpu()[0]) == 1 for k in ("actor", "q1", "q2", "log_ent_coef"))
    # ... and on the synthetic rows that tests/test_sac_update_cpu.py holds to every condition (both clamps met, each critic the smaller
    # one on a good share of the rows), whatever the ring's rows happen to meet
    env.sac_bind(ent_coef="auto_%g" % su.ENT_INIT)
    _against_twin(case, env, {k: v.to(env.device) for k, v in su.synthetic_batch(case).items()}, su.ROWS, 0.0, case + " (synthetic rows)")
    env.close()


def test_row_tails_and_slab_counts():
    """Base case: minibatches of 1, 31, 32, 33, 65 and 96 rows under 1 slab (one workgroup walks every tile), 2 (a workgroup walks two
    tiles at 96 rows) and 32 (most slabs unused), each against the twin; and a handle bound with 32 slabs gives the bytes of one bound
    with exactly as many slabs as the minibatch has tiles: only used slabs are summed."""
    env, _ = _env("base")
    batch = su.sample(env, su.ROWS)
    for slabs in (1, 2, 32):
        for n in (1, 31, 32, 33, 65, 96):
            env.sac_bind(ent_coef="auto_%g" % su.ENT_INIT, slabs=slabs)
            # (one row: the float32 twin's own error is the floor nearly everywhere; the statistics' bound holds as it stands)
            _against_twin("base", env, batch, n, 0.0, f"slabs {slabs} rows {n}")
    for n, tiles in ((33, 2), (96, 3)):
        got = []
        for slabs in (32, tiles):
            env.sac_bind(ent_coef="auto_%g" % su.ENT_INIT, slabs=slabs)
            out = env.sac_update(su.head(batch, n), 1, minibatch=n, lr=0.0, grad=True, target=True, **dict(STEP, tau=0.0))
            got.append((out["grad"].cpu().numpy().tobytes(), out["target"].cpu().numpy().tobytes(), np.array([out[k][0] for k in _stat_names()]).tobytes()))
        assert got[0] == got[1], f"{n} rows: 32 slabs and {tiles} slabs differ"
    env.close()


def _ulp(a, b):
    return int(np.abs(_ordered(np.ascontiguousarray(a, dtype=np.float32)) - _ordered(np.ascontiguousarray(b, dtype=np.float32))).max()) if np.size(a) else 0


@pytest.mark.parametrize("case", ("base", "stride"))
def test_one_adam_step_and_polyak_bit_for_bit(case):
    """One step at lr 1e-3 from zero moments: weights, m and v of actor, q1, q2 and the scalar 0 ulp from adam_step_f32 (no clip) on the
    device's own dev_grad; the targets bit for bit the numpy float32 polyak rule on the device's new critics."""
    env, _ = _env(case)
    batch = su.sample(env, su.ROWS)
    w0 = su.device_nets(env)
    out = env.sac_update(batch, 1, minibatch=su.ROWS, lr=1e-3, grad=True, **STEP)
    w1 = su.device_nets(env)
    g = su.unpack_grad(out["grad"].cpu().numpy(), w0["actor"], w0["q1"], dtype=np.float32)
    worst = 0
    for name in su.TENSORS:
        start = [(w.numpy(), b.numpy()) for w, b in w0[name]]
        want, _, want_m, want_v = pu.adam_step_f32(start, g[name], 1, 1e-3, 0.0, moments=True)
        st = env.sac_state(name)
        got_m = pu.unpack_grad(st["m"].cpu().numpy(), w0[name], [], dtype=np.float32)["actor"]
        got_v = pu.unpack_grad(st["v"].cpu().numpy(), w0[name], [], dtype=np.float32)["actor"]
        for want_x, got_x in ((want, [(w.numpy(), b.numpy()) for w, b in w1[name]]), (want_m, got_m), (want_v, got_v)):
            for (xw, xb), (yw, yb) in zip(want_x, got_x):
                worst = max(worst, _ulp(xw, yw), _ulp(xb, yb))
        assert int(st["t"].cpu()[0]) == 1
    ge = np.array([g["log_ent_coef"]], dtype=np.float32)
    none = np.zeros(0, dtype=np.float32)
    want, _, want_m, want_v = pu.adam_step_f32([(np.array([LEC], dtype=np.float32), none)], [(ge, none)], 1, 1e-3, 0.0, moments=True)
    st = env.sac_state("log_ent_coef")
    worst = max(worst, _ulp(want[0][0], env.sac_log_ent_coef().cpu().numpy()), _ulp(want_m[0][0], st["m"].cpu().numpy()), _ulp(want_v[0][0], st["v"].cpu().numpy()))
    print(f"{case}: Adam step, worst ulp distance from the numpy restatement {worst}")
    assert worst == 0
    omt, tf = np.float32(1.0 - su.TAU), np.float32(su.TAU)
    for q, tq in (("q1", "q1_target"), ("q2", "q2_target")):
        for (t0, tb0), (w, b), (t1, tb1) in zip(w0[tq], w1[q], w1[tq]):
            assert (omt * t0.numpy() + tf * w.numpy()).astype(np.float32).tobytes() == t1.numpy().tobytes(), tq
            assert (omt * tb0.numpy() + tf * b.numpy()).astype(np.float32).tobytes() == tb1.numpy().tobytes(), tq
        assert any(not torch.equal(t0, t1) for (t0, _), (t1, _) in zip(w0[tq], w1[tq]))
    env.close()


@pytest.mark.parametrize("case", ("base", "two_pair"))
def test_the_loop_inside_a_call_is_the_sequence_of_one_step_calls(case):
    """One call of 3 steps of 40 rows against 3 one-step calls on a twin handle with first_row advanced: the five nets, the moments,
    the scalar and the counters bit for bit, and the statistics."""
    env, _ = _env(case)
    other, _ = _env(case)
    n = 40
    batch = su.sample(env, 3 * n)
    su_state = su.device_state
    pu.same_state(su_state(env), su_state(other), "twin handles before the update")
    whole = env.sac_update(batch, 3, minibatch=n, lr=1e-3, **STEP)
    for g in range(3):
        part = other.sac_update({k: v[g * n:(g + 1) * n] for k, v in batch.items()}, 1, minibatch=n, lr=1e-3, first_row=g * n, **STEP)
        assert all(part[k][0] == whole[k][g] for k in _stat_names()), (g, {k: (part[k][0], whole[k][g]) for k in _stat_names()})
    a, b = su_state(env), su_state(other)
    pu.same_state(a, b, "3 steps in one call and in three")
    assert int(a["actor/t"][0]) == int(a["q1/t"][0]) == int(a["q2/t"][0]) == int(a["log_ent_coef/t"][0]) == 3
    env.close()
    other.close()


@pytest.mark.parametrize("case", ("base", "stride"))
def test_the_actor_pass_sees_the_updated_critics(case):
    """One step at lr 1e-2: the actor's gradient meets the yardstick against the twin's full step, whose actor pass runs under the
    critics the step has just updated (tests/test_sac_update_cpu.py: under the stale ones the gradient lies > 1000 x outside)."""
    env, _ = _env(case)
    batch = su.sample(env, su.ROWS)
    _against_twin(case, env, batch, su.ROWS, 1e-2, f"{case} lr 1e-2", names=("actor",), stats=False)
    env.close()


def test_wiring_to_sac_targets_and_collect_replay():
    """dev_target of a 2-step call is sac_targets on the same rows under the coefficient the step used, bit for bit on all rows; a
    handle freshly bound to the trained actor records the same collect_replay bytes as the trained handle does without a re-bind;
    sac_targets after an update runs under the polyak-averaged critics."""
    env, _ = _env("base")
    other, _ = _env("base")
    n = 48
    batch = su.sample(env, 2 * n)
    tg = lambda e, coef: e.sac_targets(batch["next_obs"], batch["reward"], batch["done"], gamma=su.GAMMA, ent_coef=coef, stochastic=True,  # noqa: E731
                                       seed=su.SEED, draw=su.DRAW, outputs=("target",))["target"].cpu().numpy()
    out = env.sac_update(batch, 2, minibatch=n, lr=1e-2, target=True, **STEP)
    got = out["target"].cpu().numpy()
    before = tg(other, float(out["ent_coef"][0]))
    other.sac_update(su.head(batch, n), 1, minibatch=n, lr=1e-2, **STEP)
    between = tg(other, float(out["ent_coef"][1]))
    assert got[:n].tobytes() == before[:n].tobytes() and got[n:].tobytes() == between[n:].tobytes()
    assert abs(out["ent_coef"][0] - np.exp(np.float64(LEC))) <= 1e-15
    assert before[n:].tobytes() != between[n:].tobytes()          # (step 1's targets ran under the nets step 0 left)
    # the trained actor acts with no re-bind
    fresh, _ = _env("base", bind=False)
    fresh.set_head_policy_network(env.sac_net_weights("actor"), "gauss_tanh", stochastic=True, seed=1, activation=su.CASES["base"][2])
    other.close()
    ring, ring_fresh = env._keep["replay"], fresh._keep["replay"]
    env.collect_replay(su.RING_SLOTS)
    fresh.collect_replay(su.RING_SLOTS)
    torch.cuda.synchronize()
    for k in ring:
        assert torch.equal(ring[k], ring_fresh[k]), k
    # sac_targets reads the averaged critics
    nets = su.device_nets(env)
    fresh.set_sac_critics(nets["q1_target"], nets["q2_target"], activation=su.CASES["base"][4])
    assert tg(env, 0.2).tobytes() == tg(fresh, 0.2).tobytes()
    fresh.set_sac_critics(*su.case_layers("base")[1:], activation=su.CASES["base"][4])
    assert tg(env, 0.2).tobytes() != tg(fresh, 0.2).tobytes()
    env.close()
    fresh.close()


def test_a_fixed_coefficient_has_no_optimiser():
    """ent_coef a float: the scalar, its moments and its counter stay, statistic [2] is 0, the scalar's gradient 0; twin handles are
    bit-identical."""
    env, _ = _env("base", ent_coef=0.2)
    other, _ = _env("base", ent_coef=0.2)
    batch = su.sample(env, su.ROWS)
    outs = [e.sac_update(batch, 2, minibatch=48, lr=1e-3, grad=True, **STEP) for e in (env, other)]
    a, b = su.device_state(env), su.device_state(other)
    pu.same_state(a, b, "twin handles")
    assert outs[0]["grad"].cpu().numpy().tobytes() == outs[1]["grad"].cpu().numpy().tobytes()
    assert a["log_ent_coef"].tobytes() == np.array([np.log(0.2)], dtype=np.float32).tobytes()
    assert not a["log_ent_coef/m"].any() and not a["log_ent_coef/v"].any() and int(a["log_ent_coef/t"][0]) == 0 and int(a["actor/t"][0]) == 2
    assert (outs[0]["ent_coef_loss"] == 0.0).all() and float(outs[0]["grad"][-1]) == 0.0
    assert abs(outs[0]["ent_coef"][1] - np.exp(np.float64(np.float32(np.log(0.2))))) <= 1e-15
    env.close()
    other.close()


def test_refusals_leave_the_state_as_it_was():
    """Code and word of every refusal, before any device call: the state is byte for byte what it was."""
    from tests import head_policy_ref as hr
    env, _ = _env("two_pair")
    batch = su.sample(env, 64)
    env.sac_update(batch, 1, minibatch=64, lr=1e-3, **STEP)
    env.set_head_value_network(hr.mlp([160, 24, 1], "tanh", 9))      # (ranenv_ppo_bind_head looks at the distribution once both head nets are there)
    state = su.device_state(env)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stats = torch.zeros((1, 8), dtype=torch.float64, device=env.device)

    def raw(n_steps=1, minibatch=64, first_row=0, obs=batch["obs"], st=stats):
        args = [None if t is None else p(t) for t in (obs, batch["action"], batch["reward"], batch["next_obs"], batch["done"])]
        env._check(env._lib.ranenv_sac_update(env._h, n_steps, minibatch, first_row, *args, 1e-3, su.GAMMA, su.TAU, su.SEED, su.DRAW,
                                              None if st is None else p(st), None, None, env._stream()), "ranenv_sac_update")

    for fn, code, word in ((lambda: raw(n_steps=0), E_INVALID, "n_steps"), (lambda: raw(minibatch=0), E_INVALID, "minibatch"),
                           (lambda: raw(obs=None), E_INVALID, "obs"), (lambda: raw(st=None), E_INVALID, "dev_stats"),
                           (lambda: raw(first_row=-1), E_INVALID, "first_row"),
                           (lambda: env.sac_bind(slabs=0), E_INVALID, "slabs"), (lambda: env.sac_bind(slabs=257), E_INVALID, "slabs"),
                           (lambda: env.ppo_bind(head=True), E_STATE, "GAUSS_TANH")):      # (the two head bindings cannot meet)
        got, text = pu.refusal(fn)
        assert got == code and word in text, (got, text)
        pu.same_state(state, su.device_state(env), text)
    # beyond the LDS plan: [512, 512] on both sides at S 16 needs 170 KB
    S = 16
    assert env.sac_lds_bytes([10 * S, 512, 512, 2 * S], [11 * S, 512, 512, 1]) > pu.LDS_MAX
    env.set_head_policy_network(hr.mlp([10 * S, 512, 512, 2 * S], "relu", 1), "gauss_tanh", stochastic=True, seed=1)
    env.set_sac_critics(hr.mlp([11 * S, 512, 512, 1], "relu", 2), hr.mlp([11 * S, 512, 512, 1], "relu", 3))
    for fn in (lambda: env.sac_bind(), lambda: env.sac_update(batch, 1, minibatch=64)):
        got, text = pu.refusal(fn)
        assert got == E_STATE and ("LDS" in text or "ranenv_sac_bind" in text), (got, text)
    got, text = pu.refusal(lambda: env.sac_bind())
    assert got == E_STATE and "LDS" in text, (got, text)
    env.close()
    # no binding; a bf16 actor; a GAUSS_CLIP actor; no critics
    env, _ = _env("base", bind=False)
    got, text = pu.refusal(lambda: env.sac_update(su.sample(env, 32), 1, minibatch=32))
    assert got == E_STATE and "ranenv_sac_bind" in text, (got, text)
    actor, q1, q2 = su.nets("base")
    env.set_head_policy_network(actor, "gauss_tanh", stochastic=True, seed=1, precision="bf16")
    got, text = pu.refusal(lambda: env.sac_bind())
    assert got == E_STATE and "bf16" in text, (got, text)
    env.set_head_policy_network(hr.mlp([50, 24, 5], "tanh", 1), "gauss_clip", log_std=torch.zeros(5), stochastic=True, seed=1)
    got, text = pu.refusal(lambda: env.sac_bind())
    assert got == E_STATE and "GAUSS_TANH" in text, (got, text)
    env.close()
    bare = hr.make_env(su.ENV_SHAPES[5], "64x64", "gauss_tanh", su.B, bind=False)[1]
    bare.set_head_policy_network(actor, "gauss_tanh", stochastic=True, seed=1)
    got, text = pu.refusal(lambda: bare.sac_bind())
    assert got == E_STATE and "critics" in text, (got, text)
    bare.close()


def test_rebinding_restarts_that_tensor_and_another_size_ends_the_binding():
    env, _ = _env("base")
    batch = su.sample(env, su.ROWS)
    env.sac_update(batch, 2, minibatch=48, lr=1e-3, **STEP)
    before = su.device_state(env)
    assert before["actor/m"].any() and before["q1/m"].any()
    # the actor again (the same shape): its moments and counter start again, nothing else moves
    actor, q1, q2 = su.nets("base")
    env.set_head_policy_network(actor, "gauss_tanh", stochastic=True, seed=1)
    after = su.device_state(env)
    assert not after["actor/m"].any() and not after["actor/v"].any() and int(after["actor/t"][0]) == 0
    for k in before:
        if not k.startswith("actor/"):
            assert before[k].tobytes() == after[k].tobytes(), k
    # the critics again: the live ones are copies of the new targets, their moments and counters start again
    other = su.nets("base", seed=77)
    env.set_sac_critics(other[1], other[2])
    after = su.device_state(env)
    for q in ("q1", "q2"):
        assert not after[f"{q}/m"].any() and not after[f"{q}/v"].any() and int(after[f"{q}/t"][0]) == 0
        for i, (w, b) in enumerate(su.layers(other[1 if q == "q1" else 2])):
            for k in (q, q + "_target"):
                assert after[f"{k}/w{i}"].tobytes() == w.numpy().tobytes() and after[f"{k}/b{i}"].tobytes() == b.numpy().tobytes(), (k, i)
    assert int(after["log_ent_coef/t"][0]) == 2 and after["log_ent_coef"].tobytes() == before["log_ent_coef"].tobytes()
    out = env.sac_update(batch, 1, minibatch=48, lr=1e-3, **STEP)
    assert np.isfinite(out["critic_loss"][0])
    t = su.device_state(env)
    assert int(t["actor/t"][0]) == 1 and int(t["q1/t"][0]) == 1 and int(t["log_ent_coef/t"][0]) == 3
    # an actor of another packed size ends the binding
    from tests import head_policy_ref as hr
    env.set_head_policy_network(hr.mlp([50, 40, 10], "relu", 5), "gauss_tanh", stochastic=True, seed=1)
    got, text = pu.refusal(lambda: env.sac_update(batch, 1, minibatch=48))
    assert got == E_STATE and "ranenv_sac_bind" in text, (got, text)
    env.sac_bind()
    env.sac_update(batch, 1, minibatch=48, lr=1e-3, **STEP)
    env.close()


def test_the_ibsched_ppo_binding_keeps_its_bytes_across_a_sac_update():
    need_gpu()
    env = pu.native_workload(su.B)
    nets = pu.member_nets("relu24", 1)
    env.set_policy_network(nets["inter"][0], nets["intra"][0], stochastic=True, seed=pu.SEED, intra_input=pu.CASES["relu24"][2])
    env.set_value_network(nets["v_inter"][0], nets["v_intra"][0])
    env.ppo_bind()
    env.reset()
    rec = {k: v.clone() for k, v in env.collect(8).items()}
    env.ppo_update(rec, epochs=1, minibatch=32, seed=1)
    ib = pu.state(env, 1)
    actor, q1, q2 = su.nets("base")
    env.set_head_policy_network(actor, "gauss_tanh", stochastic=True, seed=1, observation="inter")
    env.set_sac_critics(q1, q2)
    env.bind_replay(su.RING_SLOTS)
    env.collect_replay(su.RING_SLOTS)
    env.sac_bind(ent_coef="auto_%g" % su.ENT_INIT)
    start = su.device_state(env)
    env.sac_update(su.sample(env, su.ROWS), 2, minibatch=48, lr=1e-3, **STEP)
    assert su.device_state(env)["actor/w0"].tobytes() != start["actor/w0"].tobytes()
    from intent_radio_sched_multi_slice_amd import _lib
    env.set_policy(_lib.POLICY_NETWORK, _lib.INTRA_PF)
    pu.same_state(ib, pu.state(env, 1), "the IBSched binding across a SAC update")
    env.close()
