"""The PPO update on the device (ranenv_ppo_bind / ranenv_ppo_update, the kernel ranenv_ppo_update_kernel) against its float64
torch-autograd twin (adapters.ppo_update_reference, tests/ppo_update_ref.py): the gradient, the re-evaluated log-probabilities, Adam,
the loop inside one launch, the members' independence, determinism, the next collect(), and the refusals.

Native-shape workload (S 5, U 25), B 12, T 8, members of 2, 4 and 6 envs -- 16, 32 and 48 inter rows: a partial tile, a tile, a tile
and a half -- minibatch 12 (every member has a short tail), nets [24] relu, [40, 24] tanh and [8, 8, 8, 8] tanh: every width off the 32
grid."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import collect_ref as cr
from tests import ppo_update_ref as ref
from tests.gpu_common import _ordered, to_host

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -3
ALL = ref.ALL                 # a minibatch size beyond every member's rows: one minibatch per epoch


_workload = ref.native_workload


def _env(case, pop=True, stochastic=True, first=ref.FIRST, seed=ref.SEED):
    """A reset env of the case's batch under the members' nets, PPO state bound; returns (env, nets)."""
    env = _workload(first[-1])
    nets = ref.member_nets(case, len(first) - 1 if pop else 1)
    layout = ref.CASES[case][2]
    if pop:
        env.set_population(first)
        env.set_policy_network(nets["inter"], nets["intra"], stochastic=stochastic, seed=seed, intra_input=layout)
        env.set_value_network(nets["v_inter"], nets["v_intra"])
    else:
        env.set_policy_network(nets["inter"][0], nets["intra"][0], stochastic=stochastic, seed=seed, intra_input=layout)
        env.set_value_network(nets["v_inter"][0], nets["v_intra"][0])
    env.ppo_bind()
    env.reset()
    return env, nets


def _record(env, first=ref.FIRST):
    rec = env.collect(ref.T)
    torch.cuda.synchronize()
    mask = rec["mask_inter"]
    assert bool(((mask == 0).any(dim=2).any(dim=0)).all()), "every env needs an inactive slice somewhere in the record"
    assert bool((mask != 0).any()), "no live slice at all"
    return rec


def _order(rec, first, epochs, seed=3):
    from intent_radio_sched_multi_slice_amd.adapters import ppo_row_order
    return ppo_row_order(rec, first, epochs, seed)


_weights, _state, _same_state = ref.weights, ref.state, ref.same_state


def _check_against_twin(env, rec, order, case, out, weights, members, what, hp=None):
    """ref.check_against_twin with the case's one activation for both nets and its intra layout"""
    return ref.check_against_twin(rec, order, out, weights, members, what, ref.CASES[case][1], ref.CASES[case][1], ref.CASES[case][2], hp=hp)


_RUNS = {}


def _gradient_run(case):
    """lr = 0, one epoch, one minibatch of all rows, no clipping, on a stochastic record: computed once per case"""
    if ("gradient", case) not in _RUNS:
        env, _ = _env(case)
        rec = _record(env)
        G = len(ref.FIRST) - 1
        order = _order(rec, ref.FIRST, 1)
        before = _state(env, G)
        out = env.ppo_update(rec, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, order=order, grad=True, probe_logp=True)
        after = _state(env, G)
        moved = [k for k in before if k.split("/")[-1] not in "tmv" and before[k].tobytes() != after[k].tobytes()]
        worst, misses = _check_against_twin(env, rec, order, case, out, _weights(env, G), range(G), case)
        _RUNS["gradient", case] = dict(moved=moved, worst=worst, misses=misses, new=out["logp"].cpu().numpy(), old=rec["logp"].cpu().numpy(),
                                       mask=rec["mask_inter"].cpu().numpy() != 0, clip_frac=out["clip_frac"][:, :, 0].copy())
        env.close()
    return _RUNS["gradient", case]


@pytest.mark.parametrize("case", list(ref.CASES))
def test_gradient_and_old_log_probabilities_against_the_float64_twin(case):
    """dev_grad per layer tensor within 8x the float32-torch yardstick of the float64 twin; the re-evaluated logp within 1 float32 ulp
    of the recorded one (stochastic inter rows) or bit-equal (intra rows), so the clip fraction is exactly 0; and lr = 0 moved nothing.
    Measured on one MI355X: worst device error 0.21x (relu24), 0.29x (tanh40x24), 0.26x (tanh8x4) of the yardstick; every stochastic
    inter row re-evaluated to the bit as well."""
    run = _gradient_run(case)
    assert not run["moved"], run["moved"]
    new, old, mask = run["new"], run["old"], run["mask"]
    d = np.abs(_ordered(new[..., 0]) - _ordered(old[..., 0]))
    print(f"{case}: inter logp ulp distance max {d.max()}, rows off by one {int((d == 1).sum())} of {d.size}")
    assert d.max() <= 1
    assert np.array_equal(new[..., 1:][mask].view(np.int32), old[..., 1:][mask].view(np.int32)), "intra logp is not re-evaluated to the bit"
    assert np.all(run["clip_frac"] == 0.0)


@pytest.mark.parametrize("case", list(ref.CASES))
def test_statistics_against_the_float64_twin(case):
    """Policy loss, value loss, entropy, approx-KL and clip fraction of that call against the twin at 1e-6 relative or absolute.
    At unchanged weights approx-KL is the rounding residual of the recorded float32 logp (|logp| 18 .. 80 with one to four masked
    positions) and nothing else: device and twin read the same few 1e-7, a few 1e-8 apart."""
    run = _gradient_run(case)
    assert not run["misses"], run["misses"]


def test_old_log_probabilities_of_a_deterministic_collect_are_bit_equal():
    env, _ = _env("tanh40x24", stochastic=False)
    rec = _record(env)
    out = env.ppo_update(rec, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, order=_order(rec, ref.FIRST, 1), probe_logp=True)
    new, old, mask = out["logp"].cpu().numpy(), rec["logp"].cpu().numpy(), rec["mask_inter"].cpu().numpy() != 0
    assert np.array_equal(new[..., 0].view(np.int32), old[..., 0].view(np.int32))
    assert np.array_equal(new[..., 1:][mask].view(np.int32), old[..., 1:][mask].view(np.int32))
    assert np.all(out["clip_frac"][:, :, 0] == 0.0)
    env.close()


def test_advantages_as_given_and_a_kind_without_a_critic_against_the_float64_twin():
    """adv_norm None (RLlib's case: the record's advantages as they are) on a handle with no intra critic, so the intra workgroups
    train the actor alone: gradient and statistics against the twin as in the gradient test, the intra value loss exactly 0, and the
    intra rows of dev_grad behind the actor's floats untouched."""
    case, G = "tanh40x24", len(ref.FIRST) - 1
    env = _workload(ref.FIRST[-1])
    nets = ref.member_nets(case, G)
    env.set_population(ref.FIRST)
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=ref.SEED, intra_input=ref.CASES[case][2])
    env.set_value_network(nets["v_inter"])
    env.ppo_bind()
    env.reset()
    rec = _record(env)
    order = _order(rec, ref.FIRST, 1)
    roles = ("inter", "intra", "v_inter")
    out = env.ppo_update(rec, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, adv_norm=None, order=order, grad=True)
    worst, misses = _check_against_twin(env, rec, order, case, out, _weights(env, G, roles), range(G), "adv as given, no intra critic",
                                        hp=dict(clip=0.2, vf_coeff=0.5, ent_coeff=0.01, adv_norm=False))
    assert 0.0 < worst <= 8.0
    assert not misses, misses
    assert np.all(out["value_loss"][:, 1, 0] == 0.0) and np.all(out["value_loss"][:, 0, 0] > 0.0)
    # (one Adam step on that handle moves the intra actor and leaves nothing of a critic to move)
    before = _state(env, G, roles)
    env.ppo_update(rec, epochs=1, minibatch=ref.MINIBATCH, lr=1e-3, adv_norm=None, order=order)
    after = _state(env, G, roles)
    assert all(before[f"intra/{m}/w0"].tobytes() != after[f"intra/{m}/w0"].tobytes() for m in range(G))
    env.close()


@pytest.mark.parametrize("case", ["relu24", "tanh40x24"])
def test_one_adam_step_is_the_stated_float32_arithmetic_on_the_devices_own_gradient(case):
    """One minibatch with lr > 0 and clipping: the new weights equal the numpy float32 restatement of clip + Adam (include/ranenv.h's
    operation order) applied to dev_grad, within 4 float32 ulp; Adam's m and v (ppo_state) against the same restatement likewise; the
    counters read 1."""
    env, _ = _env(case)
    rec = _record(env)
    G = len(ref.FIRST) - 1
    order = _order(rec, ref.FIRST, 1)
    w0 = _weights(env, G)
    hp = dict(lr=np.array([3e-4, 1e-3, 5e-3]), grad_clip=np.array([0.5, 0.05, 0.0]), betas=(0.9, 0.999), eps=1e-8)
    out = env.ppo_update(rec, epochs=1, minibatch=ALL, order=order, grad=True, **hp)
    w1 = _weights(env, G)
    ref.check_adam_step(env, out, w0, w1, hp, G, case)
    assert any(not np.array_equal(x[0], y[0]) for x, y in zip(w0["inter"][0], w1["inter"][0])), "the weights did not move"
    env.close()


def _loop_run(case):
    """2 epochs x k minibatches of 12 in ONE call (handle a) against the same chunks one call each (handle b), the twin following every
    single call of both epochs; computed once per case: (state a, state b, worst followed gradient ratio, statistics beyond 1e-6,
    the largest clip fraction of a followed step per epoch)"""
    if ("loop", case) in _RUNS:
        return _RUNS["loop", case]
    G, E, MB = len(ref.FIRST) - 1, 2, ref.MINIBATCH
    env_a, _ = _env(case)
    env_b, _ = _env(case)
    rec_a, rec_b = _record(env_a), _record(env_b)
    for k in rec_a:
        assert torch.equal(rec_a[k], rec_b[k]), k
    order = _order(rec_a, ref.FIRST, E)
    hp = dict(lr=2e-3, clip=0.2, vf_coeff=0.5, ent_coeff=0.01, grad_clip=0.5)
    out = env_a.ppo_update(rec_a, epochs=E, minibatch=MB, order=order, **hp)
    fi, fa = order["first_inter"], order["first_intra"]
    n_chunks = [[-(-(int(f[m + 1]) - int(f[m])) // MB) for m in range(G)] for f in (fi, fa)]
    assert np.array_equal(out["minibatches"][:, 0, :], np.repeat(np.array(n_chunks[0])[:, None], E, 1))
    assert np.array_equal(out["minibatches"][:, 1, :], np.repeat(np.array(n_chunks[1])[:, None], E, 1))
    # (16 and 32 inter rows end in a short minibatch of 4 and 8, the 48 of the largest member are 4 full ones; the intra rows vary)
    assert min(n_chunks[0]) >= 2 and sum((int(fi[m + 1]) - int(fi[m])) % MB != 0 for m in range(G)) >= 2, "short tails"
    followed, misses, steps, clipped = 0.0, [], 0, [0.0] * E
    for ep in range(E):
        for i in range(max(max(n_chunks[0]), max(n_chunks[1]))):
            step = ref.chunk_order(order, G, MB, ep, i)
            # (the twin follows EVERY step of both epochs, on the REAL call's dev_grad and statistics at the weights read back in front of it)
            weights = _weights(env_b, G)
            o = env_b.ppo_update(rec_b, epochs=1, minibatch=ALL, order=step, grad=True, **hp)
            worst, miss = _check_against_twin(env_b, rec_b, step, case, o, weights, range(G), f"{case} epoch {ep} chunk {i}")
            followed, misses, steps = max(followed, worst), misses + miss, steps + 1
            clipped[ep] = max(clipped[ep], float(o["clip_frac"][:, :, 0].max()))
    print(f"{case}: {steps} followed steps, worst gradient ratio {followed:.3g}, largest clip fraction per epoch {clipped}")
    assert steps == E * max(max(n_chunks[0]), max(n_chunks[1]))
    _RUNS["loop", case] = (_state(env_a, G), _state(env_b, G), followed, misses, clipped)
    env_a.close()
    env_b.close()
    return _RUNS["loop", case]


@pytest.mark.parametrize("case", ["tanh40x24", "tanh8x4"])
def test_the_loop_inside_one_launch_equals_one_minibatch_per_launch(case):
    """One call of 2 epochs x k minibatches against 2k one-minibatch calls over the same chunks on a twin handle: weights, moments and
    counters bit for bit (a stale weight read inside the launch would show here); the gradient of each of the 2k steps, at the weights
    read back in front of it, within the gradient test's bound of the float64 twin.  Measured on one MI355X over the 24 steps:
    0.11-1.30x (tanh40x24) and 0.11-1.22x (tanh8x4) of the yardstick, the second epoch no worse than the first."""
    a, b, followed, _, _ = _loop_run(case)
    _same_state(a, b, case)
    assert 0.0 < followed <= 8.0


@pytest.mark.parametrize("case", ["tanh40x24", "tanh8x4"])
def test_followed_statistics_against_the_float64_twin(case):
    """The statistics of each of the 2k followed steps, at the weights read back in front of it, against the twin at 1e-6 -- and some
    followed step has clipped rows (a clip fraction > 0), so the kernel's min / clamp selection is held to the twin's on rows where the
    two branches differ, not only where the ratio is 1."""
    run = _loop_run(case)
    assert not run[3], run[3]
    assert max(run[4]) > 0.0, run[4]


def test_members_are_independent_and_a_plain_handle_is_a_population_of_one():
    """One call with three different (lr, clip, minibatch, epochs) equals three calls that each set epochs = 0 for the other two
    members, bit for bit; a member with epochs = 0 keeps its bytes; the same call twice on twin handles gives the same bytes; G = 1
    on a plain handle equals a 1-member population."""
    case, G = "tanh40x24", len(ref.FIRST) - 1
    hp = dict(lr=np.array([1e-3, 3e-4, 2e-3]), clip=np.array([0.1, 0.2, 0.3]), minibatch=np.array([12, 7, 32]), epochs=np.array([2, 0, 3]))
    envs = [_env(case)[0] for _ in range(3)]
    recs = [_record(e) for e in envs]
    order = _order(recs[0], ref.FIRST, 3)
    start = _state(envs[0], G)
    envs[0].ppo_update(recs[0], order=order, **hp)
    envs[1].ppo_update(recs[1], order=order, **hp)
    for m in range(G):
        only = dict(hp, epochs=np.where(np.arange(G) == m, hp["epochs"], 0))
        envs[2].ppo_update(recs[2], order=order, **only)
    a, b, c = (_state(e, G) for e in envs)
    _same_state(a, b, "the same call on twin handles")
    _same_state(a, c, "one call against one call per member")
    for k in a:
        if "/1/" in k:
            assert a[k].tobytes() == start[k].tobytes(), f"epochs = 0 moved {k}"
    assert any(a[k].tobytes() != start[k].tobytes() for k in a if "/0/w" in k) and any(a[k].tobytes() != start[k].tobytes() for k in a if "/2/w" in k)
    for e in envs:
        e.close()
    one = [0, 6]
    plain, _ = _env(case, pop=False, first=one)
    grouped, _ = _env(case, pop=True, first=one)
    rp, rg = _record(plain, one), _record(grouped, one)
    order = _order(rp, one, 2)
    sp = plain.ppo_update(rp, epochs=2, minibatch=ref.MINIBATCH, lr=1e-3, order=order)
    sg = grouped.ppo_update(rg, epochs=2, minibatch=ref.MINIBATCH, lr=1e-3, order=order)
    _same_state(_state(plain, 1), _state(grouped, 1), "plain handle against a population of one")
    for k in sp:
        assert np.array_equal(sp[k], sg[k]), k
    plain.close()
    grouped.close()


def test_the_next_collect_acts_on_the_trained_weights_and_net_weights_round_trips():
    """collect() after an update, with no rebind, records logp and vf that the float64 checks of tests/collect_ref.py accept for the
    weights read back; net_weights returns a freshly bound net exactly."""
    case, one = "tanh40x24", [0, 6]
    env, nets = _env(case, pop=False, first=one)
    for r in ref.ROLES:
        for (w, b), (w0, b0) in zip(env.net_weights(r), cr.layers_of(nets[r][0])[0]):
            assert torch.equal(w.cpu(), w0) and torch.equal(b.cpu(), b0), r
        assert env.net_activation(r) == ref.CASES[case][1]
    rec = _record(env, one)
    start = _weights(env, 1)
    env.ppo_update(rec, epochs=3, minibatch=ref.MINIBATCH, lr=3e-3, seed=5)
    trained = _weights(env, 1)
    assert not np.array_equal(start["inter"][0][0][0], trained["inter"][0][0][0])
    seq = {r: ref.as_sequential(trained[r][0], ref.CASES[case][1]) for r in ref.ROLES}
    v = env.views()
    episode, step0 = v["episode_number"].cpu().numpy().copy(), v["step_number"].cpu().numpy().copy()
    rec2 = to_host(env.collect(3))
    layout = ref.CASES[case][2]
    for t in range(3):
        r, _ = cr.check_actor_record(rec2, t, seq["inter"], seq["intra"], True, ref.SEED, episode, step0 + t, layout)
        r["vf"] = cr.check_values(rec2["vf"][t], rec2["obs_inter"][t], rec2["obs_intra"][t], rec2["mask_intra"][t], seq["v_inter"], seq["v_intra"], layout)
        print(f"slot {t}: worst error / bound after the update: {r}")
    env.close()


def test_rebinding_the_critic_restarts_the_actors_optimiser_with_the_shared_counter():
    """Actor and critic of a kind share one step counter: re-binding the critics alone zeroes the counter, the critics' moments AND
    the actors' moments (old moments under the bias correction of t = 1 would be a wrong step), and leaves the trained actors' weights."""
    case, one = "tanh40x24", [0, 6]
    env, nets = _env(case, pop=False, first=one)
    rec = _record(env, one)
    env.ppo_update(rec, epochs=1, minibatch=ref.MINIBATCH, lr=1e-3, order=_order(rec, one, 1))
    trained = _state(env, 1)
    assert all(int(trained[f"{r}/0/t"][0]) > 0 and trained[f"{r}/0/m"].any() and trained[f"{r}/0/v"].any() for r in ref.ROLES)
    env.set_value_network(nets["v_inter"][0], nets["v_intra"][0])
    after = _state(env, 1)
    for r in ref.ROLES:
        assert int(after[f"{r}/0/t"][0]) == 0 and not after[f"{r}/0/m"].any() and not after[f"{r}/0/v"].any(), r
    for k in trained:
        if k.startswith(("inter/", "intra/")) and k.split("/")[-1][0] in "wb":
            assert after[k].tobytes() == trained[k].tobytes(), f"re-binding the critics moved the actors' {k}"
    env.close()


_code = ref.refusal


def test_refusals_precede_every_device_call():
    """bf16 nets, intra nets per slice, a mixed population, the head policy, nets beyond the LDS plan, minibatch < 1 and an update
    without ranenv_ppo_bind: each returns its code with a text.  Where the state is readable round the refused call -- minibatch < 1,
    the update after an outgrown binding (weights; the optimiser state is what the binding lost), the head policy, the binding's own
    launch-length caps -- it stays byte for byte; ``force=True`` lifts the caps."""
    from intent_radio_sched_multi_slice_amd import _lib
    case, one = "tanh40x24", [0, 6]
    env, nets = _env(case, pop=False, first=one)
    rec = _record(env, one)
    order = _order(rec, one, 1)
    before = _state(env, 1)
    code, text = _code(lambda: env.ppo_update(rec, epochs=1, minibatch=0, order=order))
    assert code == E_INVALID and "minibatch" in text
    _same_state(before, _state(env, 1), "minibatch < 1")
    layout = ref.CASES[case][2]
    S, n_in = env.S, env.net_input_dims(layout)[1]
    # intra nets per slice
    env.set_policy_network(nets["inter"][0], [nets["intra"][0]] * S, stochastic=True, seed=1, intra_input=layout)
    assert _code(env.ppo_bind)[0] == E_STATE and _code(lambda: env.ppo_update(rec, epochs=1, order=order))[0] == E_STATE
    # bf16
    env.set_policy_network(nets["inter"][0], nets["intra"][0], stochastic=True, seed=1, intra_input=layout, precision="bf16")
    code, text = _code(env.ppo_bind)
    assert code == E_STATE and "bf16" in text
    assert _code(lambda: env.ppo_update(rec, epochs=1, order=order))[0] == E_STATE
    # beyond the LDS plan
    wide = ref.make_role_nets(S, env.Us, [512, 512, 512], "tanh", layout, 77)
    env.set_policy_network(wide["inter"], wide["intra"], stochastic=True, seed=1, intra_input=layout)
    env.set_value_network(wide["v_inter"], wide["v_intra"])
    code, text = _code(env.ppo_bind)
    assert code == E_STATE and "LDS" in text
    # back to the case's nets: the binding call above outgrew the bound state, so an update needs a new ranenv_ppo_bind
    env.set_policy_network(nets["inter"][0], nets["intra"][0], stochastic=True, seed=1, intra_input=layout)
    env.set_value_network(nets["v_inter"][0], nets["v_intra"][0])
    w_before = _weights(env, 1)
    code, text = _code(lambda: env.ppo_update(rec, epochs=1, order=order))
    assert code == E_STATE and "ranenv_ppo_bind" in text
    w_after = _weights(env, 1)
    for r in ref.ROLES:
        for (w0, b0), (w1, b1) in zip(w_before[r][0], w_after[r][0]):
            assert w0.tobytes() == w1.tobytes() and b0.tobytes() == b1.tobytes(), f"the update after an outgrown binding moved {r}"
    env.ppo_bind()
    env.ppo_update(rec, epochs=1, minibatch=ref.MINIBATCH, order=order)
    # the head policy
    before = _state(env, 1)
    env.set_policy(_lib.POLICY_HEAD_NETWORK)
    assert _code(lambda: env.ppo_update(rec, epochs=1, order=order))[0] == E_STATE
    env.set_policy(_lib.POLICY_NETWORK)
    _same_state(before, _state(env, 1), "the head policy")
    # the binding's own caps on the launch length: rows x epochs and optimiser steps of one member, unless forced
    from intent_radio_sched_multi_slice_amd._lib import RanEnvError
    for cap, word in (("PPO_ROW_EPOCHS_CAP", "rows x epochs"), ("PPO_STEPS_CAP", "optimiser steps")):
        setattr(env, cap, 3)            # (an instance attribute over the class's: this handle alone)
        with pytest.raises(RanEnvError, match=word):
            env.ppo_update(rec, epochs=1, minibatch=ref.MINIBATCH, order=order)
        _same_state(before, _state(env, 1), cap)
        delattr(env, cap)
    env.PPO_ROW_EPOCHS_CAP, env.PPO_STEPS_CAP = 3, 3
    env.ppo_update(rec, epochs=1, minibatch=ref.MINIBATCH, order=order, force=True)
    del env.PPO_ROW_EPOCHS_CAP, env.PPO_STEPS_CAP
    forced = _state(env, 1)
    assert forced["inter/0/w0"].tobytes() != before["inter/0/w0"].tobytes() and int(forced["inter/0/t"][0]) > int(before["inter/0/t"][0])
    # a mixed population
    env.set_population(one)
    env.set_policy_network([nets["inter"][0]], [nets["intra"][0]], stochastic=True, seed=1, intra_input=layout, mixed=True)
    env.set_value_network([nets["v_inter"][0]], [nets["v_intra"][0]], mixed=True)
    code, text = _code(env.ppo_bind)
    assert code == E_STATE and "mixed" in text
    env.close()
    other = _workload_without_bind(case, one)
    code, text = _code(lambda: other.ppo_update(rec, epochs=1, order=order))
    assert code == E_STATE and "ranenv_ppo_bind" in text
    other.close()


def _workload_without_bind(case, first):
    env = _workload(first[-1])
    nets = ref.member_nets(case, 1)
    env.set_policy_network(nets["inter"][0], nets["intra"][0], stochastic=True, seed=1, intra_input=ref.CASES[case][2])
    env.set_value_network(nets["v_inter"][0], nets["v_intra"][0])
    env.reset()
    return env
