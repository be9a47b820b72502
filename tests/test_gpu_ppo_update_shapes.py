"""The PPO update kernel (ranenv_ppo_update_kernel) across net shapes, slice counts and row tails, against its float64 twin
(adapters.ppo_update_reference) with the float32 twin as the yardstick -- what tests/test_gpu_ppo_update.py checks at one environment
shape and three narrow nets, here over ref.SHAPES: widths up to the edge of the LDS plan (162 304 bytes), both LDS strides, one to four
hidden layers, deep ReLU, actors and critics that differ in depth, width and activation, S 1 / 5 / 10 / 13 / 16, both intra layouts;
then, on the native shape, minibatches of 1, 31, 32, 33, 64 and 65 rows, list entries outside the record, the refusal one step beyond
the LDS plan, and a population of 64 members.

Every grid case: B 12, T 8, members of 2, 4 and 6 envs (16, 32 and 48 inter rows), a stochastic collect.  Tolerances are those of
tests/test_gpu_ppo_update.py: the gradient within 8x the float32-torch error (floor 1e-6 relative), statistics 1e-6, Adam 4 float32 ulp,
bit equality between schedules."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import ppo_update_ref as ref
from tests.gpu_common import _ordered, need_gpu, shaped_workload

pytestmark = pytest.mark.gpu

E_STATE = -3
ALL = ref.ALL
G = len(ref.FIRST) - 1
NATIVE = "tanh40x24"          # the nets of the tests off the grid
HP_LOOP = dict(lr=2e-3, clip=0.2, vf_coeff=0.5, ent_coeff=0.01, grad_clip=0.5)


def _order(rec, first, epochs, seed=3):
    from intent_radio_sched_multi_slice_amd.adapters import ppo_row_order
    return ppo_row_order(rec, first, epochs, seed)


def _lds_bytes(env):
    lds = C.c_int64()
    env._check(env._lib.ranenv_ppo_layout(env._h, None, C.byref(lds)), "ranenv_ppo_layout")
    return lds.value


def _shape_env(shape):
    """A reset env of the grid case's (S, Us) under the population's nets of the case's shapes, PPO state bound"""
    need_gpu()
    S, Us, layout, _, _ = ref.SHAPES[shape]
    env = shaped_workload(S, Us, ref.FIRST[-1], seed=40 + list(ref.SHAPES).index(shape)).env
    nets = ref.shape_nets(shape, G)
    env.set_population(ref.FIRST)
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=ref.SEED, intra_input=layout)
    env.set_value_network(nets["v_inter"], nets["v_intra"])
    env.ppo_bind()
    env.reset()
    return env


def _shape_record(env):
    """collect(T); for S > 1 the record holds masked and unmasked sorted positions (some row with fewer than S active slices -- position
    0 masked -- and some row with all S -- every position unmasked); for S 1 every row is active"""
    rec = env.collect(ref.T)
    torch.cuda.synchronize()
    n_act = (rec["mask_inter"] != 0).sum(dim=2)
    if env.S > 1:
        assert int(n_act.min()) < env.S and int(n_act.max()) == env.S, (int(n_act.min()), int(n_act.max()))
    else:
        assert bool((n_act == 1).all())
    return rec


def _native_env(first, case=NATIVE):
    """A reset env of the native shape (S 5, Us 5; every env on a scenario with an inactive slice) under a population of the case's nets"""
    env = ref.native_workload(first[-1])
    nets = ref.member_nets(case, len(first) - 1)
    env.set_population(first)
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=ref.SEED, intra_input=ref.CASES[case][2])
    env.set_value_network(nets["v_inter"], nets["v_intra"])
    env.ppo_bind()
    env.reset()
    return env


def _native_record(env, T=ref.T):
    rec = env.collect(T)
    torch.cuda.synchronize()
    assert bool((rec["mask_inter"] != 0).any(dim=2).all()), "an env without a live slice"
    return rec


def _twin_args(shape):
    _, _, layout, (_, aa), (_, ca) = ref.SHAPES[shape]
    return aa, ca, layout


_RUNS = {}


def _gradient_run(shape):
    """lr = 0, one epoch, one minibatch of all rows, no clipping, on a stochastic record: computed once per grid case"""
    if ("gradient", shape) not in _RUNS:
        env = _shape_env(shape)
        rec = _shape_record(env)
        order = _order(rec, ref.FIRST, 1)
        before = ref.state(env, G)
        out = env.ppo_update(rec, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, order=order, grad=True, probe_logp=True)
        after = ref.state(env, G)
        moved = [k for k in before if k.split("/")[-1] not in "tmv" and before[k].tobytes() != after[k].tobytes()]
        # (unpack_grad, inside, is told the actor's and the critic's own shapes and asserts exact zeros in dev_grad's padding)
        worst, misses = ref.check_against_twin(rec, order, out, ref.weights(env, G), range(G), f"shape {shape}", *_twin_args(shape))
        _RUNS["gradient", shape] = dict(moved=moved, worst=worst, misses=misses, new=out["logp"].cpu().numpy(), old=rec["logp"].cpu().numpy(),
                                        mask=rec["mask_inter"].cpu().numpy() != 0, clip_frac=out["clip_frac"][:, :, 0].copy(), lds=_lds_bytes(env))
        env.close()
    return _RUNS["gradient", shape]


@pytest.mark.parametrize("shape", list(ref.SHAPES))
def test_gradient_and_old_log_probabilities_against_the_float64_twin(shape):
    """dev_grad per layer tensor (each net unpacked by its own shape, padding exact zeros) within 8x the float32-torch yardstick of the
    float64 twin; the re-evaluated logp within 1 float32 ulp of the recorded one (inter rows) or bit-equal (intra rows), the clip
    fraction exactly 0; lr = 0 moved no weight.  Case A is the launch at 162 304 bytes of dynamic LDS.
    Measured on one MI355X, worst device error over the yardstick: 1.18 (A), 0.97 (B), 0.79 (C), 0.35 (D), 0.90 (E), 3.11 (F); every one of the 96 stochastic inter rows
    of each case re-evaluated to the bit as well."""
    run = _gradient_run(shape)
    assert not run["moved"], run["moved"]
    assert 0.0 < run["worst"] <= 8.0
    new, old, mask = run["new"], run["old"], run["mask"]
    d = np.abs(_ordered(new[..., 0]) - _ordered(old[..., 0]))
    print(f"shape {shape}: inter logp ulp distance max {d.max()}, rows off by one {int((d == 1).sum())} of {d.size}")
    assert d.max() <= 1
    assert np.array_equal(new[..., 1:][mask].view(np.int32), old[..., 1:][mask].view(np.int32)), "intra logp is not re-evaluated to the bit"
    assert np.all(run["clip_frac"] == 0.0)


@pytest.mark.parametrize("shape", list(ref.SHAPES))
def test_statistics_against_the_float64_twin(shape):
    """Policy loss, value loss, entropy, approx-KL and clip fraction of that call against the twin at 1e-6 relative or absolute."""
    run = _gradient_run(shape)
    assert not run["misses"], run["misses"]


@pytest.mark.parametrize("shape", list(ref.SHAPES))
def test_the_launchs_lds_bytes_are_the_headers_formula(shape):
    S, Us, layout, (aw, _), (cw, _) = ref.SHAPES[shape]
    assert _gradient_run(shape)["lds"] == ref.lds_bytes(S, Us, layout, aw, cw) <= ref.LDS_MAX
    if shape == "A":
        assert _gradient_run(shape)["lds"] == 162304


@pytest.mark.parametrize("shape", ["A", "C", "E"])
def test_one_adam_step_is_the_stated_float32_arithmetic_on_the_devices_own_gradient(shape):
    """One minibatch with per-member lr and grad_clip (the last member unclipped): new weights, m and v within 4 float32 ulp of
    ref.adam_step_f32 on the device's own dev_grad; the padding of m and v exact zeros; the counters read 1.
    Measured on one MI355X, worst ulp distance (weights, moments): 0 and 0 on all 3 568 461 (A), 167 412 (C) and 347 850 (E) weights."""
    env = _shape_env(shape)
    rec = _shape_record(env)
    order = _order(rec, ref.FIRST, 1)
    w0 = ref.weights(env, G)
    hp = dict(lr=np.array([3e-4, 1e-3, 5e-3]), grad_clip=np.array([0.5, 0.05, 0.0]), betas=(0.9, 0.999), eps=1e-8)
    out = env.ppo_update(rec, epochs=1, minibatch=ALL, order=order, grad=True, **hp)
    w1 = ref.weights(env, G)
    ref.check_adam_step(env, out, w0, w1, hp, G, f"shape {shape}")
    for r in ref.ROLES:
        assert all(not np.array_equal(x[0], y[0]) for m in range(G) for x, y in zip(w0[r][m], w1[r][m])), f"a layer of {r} did not move"
    env.close()


@pytest.mark.parametrize("shape", ["B", "E"])
def test_the_loop_inside_one_launch_equals_one_minibatch_per_launch(shape):
    """2 epochs of minibatches of 12 in ONE call against the same chunks one call each on a twin handle: weights, moments and counters bit
    for bit -- the stale-weight-read check at sizes where a row of W spans several cache lines."""
    E, MB = 2, ref.MINIBATCH
    env_a, env_b = _shape_env(shape), _shape_env(shape)
    rec_a, rec_b = _shape_record(env_a), _shape_record(env_b)
    for k in rec_a:
        assert torch.equal(rec_a[k], rec_b[k]), k
    order = _order(rec_a, ref.FIRST, E)
    start = ref.state(env_a, G)
    out = env_a.ppo_update(rec_a, epochs=E, minibatch=MB, order=order, **HP_LOOP)
    n_chunks = [[-(-(int(f[m + 1]) - int(f[m])) // MB) for m in range(G)] for f in (order["first_inter"], order["first_intra"])]
    for kind_i in range(2):
        assert np.array_equal(out["minibatches"][:, kind_i, :], np.repeat(np.array(n_chunks[kind_i])[:, None], E, 1))
    assert min(n_chunks[0]) >= 2 and sum((int(order["first_inter"][m + 1]) - int(order["first_inter"][m])) % MB != 0 for m in range(G)) >= 2, "short tails"
    for ep in range(E):
        for i in range(max(max(n_chunks[0]), max(n_chunks[1]))):
            env_b.ppo_update(rec_b, epochs=1, minibatch=ALL, order=ref.chunk_order(order, G, MB, ep, i), **HP_LOOP)
    a, b = ref.state(env_a, G), ref.state(env_b, G)
    ref.same_state(a, b, f"shape {shape}")
    assert all(a[k].tobytes() != start[k].tobytes() for k in a if k.split("/")[-1][0] == "w"), "a weight matrix did not move"
    for m in range(G):
        assert int(a[f"inter/{m}/t"][0]) == E * n_chunks[0][m] and int(a[f"intra/{m}/t"][0]) == E * n_chunks[1][m]
    env_a.close()
    env_b.close()


# ---- row tails: minibatches of 1, 31, 32, 33, 64 and 65 rows -----------------------------------------------------------------------
TAIL_FIRST = [0, 2, 4, 6, 8, 10, 12]
TAILS = [1, 31, 32, 33, 64, 65]


def _cut(order, sizes):
    """Member m's list: the first sizes[m] entries of its own shuffle, for both kinds"""
    out = {}
    for kind in ("inter", "intra"):
        f, o = order["first_" + kind], order["order_" + kind]
        assert all(int(f[m + 1]) - int(f[m]) >= n for m, n in enumerate(sizes)), (kind, f)
        out["order_" + kind] = torch.cat([o[:1, int(f[m]):int(f[m]) + n] for m, n in enumerate(sizes)], dim=1).contiguous()
        out["first_" + kind] = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return out


def _tails_run():
    """Six members of 66 inter rows (collect(33) on 2 envs each) whose lists are cut to 1, 31, 32, 33, 64 and 65 entries: the lr = 0 call
    of one minibatch against the twin, then -- on two handles in the same state -- minibatches of 32 in one call against one call per chunk"""
    if "tails" in _RUNS:
        return _RUNS["tails"]
    n = len(TAILS)
    env_a, env_b = _native_env(TAIL_FIRST), _native_env(TAIL_FIRST)
    rec_a, rec_b = _native_record(env_a, 33), _native_record(env_b, 33)
    for k in rec_a:
        assert torch.equal(rec_a[k], rec_b[k]), k
    full = _order(rec_a, TAIL_FIRST, 1)
    assert all(int(full["first_inter"][m + 1]) - int(full["first_inter"][m]) == 66 for m in range(n))
    lists = _cut(full, TAILS)
    w0 = ref.weights(env_a, n)
    probe = dict(epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, order=lists, adv_norm="minibatch")
    out = env_a.ppo_update(rec_a, grad=True, **probe)
    env_b.ppo_update(rec_b, **probe)          # (lr = 0 still moves Adam's moments and counter: both handles take the call)
    worst, misses = ref.check_against_twin(rec_a, lists, out, w0, range(n), "row tails", "tanh", "tanh", ref.CASES[NATIVE][2])
    one = ref.unpack_grad(out["grad"][0, 0].cpu().numpy(), w0["inter"][0], w0["v_inter"][0])
    mid = ref.state(env_a, n)
    ref.same_state(mid, ref.state(env_b, n), "the lr = 0 call on twin handles")
    hp = dict(HP_LOOP, adv_norm="minibatch")
    o32 = env_a.ppo_update(rec_a, epochs=1, minibatch=32, order=lists, **hp)
    for i in range(3):
        env_b.ppo_update(rec_b, epochs=1, minibatch=ALL, order=ref.chunk_order(lists, n, 32, 0, i), **hp)
    _RUNS["tails"] = dict(worst=worst, misses=misses, one_row_actor=one["actor"], one_row_policy_loss=float(out["policy_loss"][0, 0, 0]), mid=mid,
                          a=ref.state(env_a, n), b=ref.state(env_b, n), rows=o32["rows"][:, :, 0].copy(), minibatches=o32["minibatches"][:, :, 0].copy())
    env_a.close()
    env_b.close()
    return _RUNS["tails"]


def test_row_tails_gradient_and_statistics_against_the_float64_twin():
    """One minibatch of 1, 31, 32, 33, 64 and 65 rows per member under adv_norm "minibatch": gradient and statistics per member against
    the twin (``rows`` and ``minibatches`` exact, inside the comparison).  The one-row member's standardised advantage is 0: its actor
    gradient is the entropy term alone -- non-zero in the twin (asserted inside the comparison) and on the device -- and its policy loss 0.
    Measured on one MI355X, worst device error over the yardstick: 0.37."""
    run = _tails_run()
    assert 0.0 < run["worst"] <= 8.0
    assert not run["misses"], run["misses"]
    assert all(np.linalg.norm(w) > 0.0 and np.linalg.norm(b) > 0.0 for w, b in run["one_row_actor"])
    assert run["one_row_policy_loss"] == 0.0


def test_row_tails_in_minibatches_of_32_equal_one_launch_per_chunk():
    """The same lists in minibatches of 32 with lr > 0 -- tails of 1, 31, 32, 32 + 1, 32 + 32 and 32 + 32 + 1 -- in one call, against
    one call per chunk on a twin handle: weights, moments and counters bit for bit."""
    run = _tails_run()
    ref.same_state(run["a"], run["b"], "row tails, minibatches of 32")
    want = np.array([-(-n // 32) for n in TAILS])
    assert np.array_equal(run["minibatches"], np.repeat(want[:, None], 2, 1)) and np.array_equal(run["rows"], np.repeat(np.array(TAILS)[:, None], 2, 1))
    for m in range(len(TAILS)):
        assert int(run["a"][f"inter/{m}/t"][0]) == 1 + want[m] and int(run["a"][f"intra/{m}/t"][0]) == 1 + want[m]
        assert run["a"][f"inter/{m}/w0"].tobytes() != run["mid"][f"inter/{m}/w0"].tobytes()


# ---- list entries outside the record ------------------------------------------------------------------------------------------------
def test_entries_outside_the_record_count_as_rows_and_contribute_nothing():
    """include/ranenv.h: "An entry outside the record counts as a row of the minibatch and contributes nothing".  Member 2's lists with
    positions 0, 31, 32 and the last overwritten by -1, n_record, n_record + 7 and 2^31 - 1 (adv_norm None, one minibatch): a row's
    weight is 1 / entries, so gradient and statistics 0..4 are the twin's on the live entries times live / entries, ``rows`` the live
    entries.  Member 0's lists hold ONLY outside entries, under lr > 0: weights and moments keep their bytes, the counters advance by the
    one minibatch, the gradient and its norm are exactly 0, nothing is NaN.  Member 1's lists are untouched.
    Measured on one MI355X, worst device error over the yardstick: 0.38."""
    env = _native_env(ref.FIRST)
    rec = _native_record(env)
    order = _order(rec, ref.FIRST, 1)
    T, B, S = rec["mask_inter"].shape
    lists, twin, ratio = {}, {}, {}
    for kind, n_record in (("inter", T * B), ("intra", T * B * S)):
        f, o = order["first_" + kind], order["order_" + kind].clone()
        outside = torch.tensor([-1, n_record, n_record + 7, 2 ** 31 - 1], dtype=torch.int32, device=o.device)
        lo, hi = int(f[2]), int(f[3])
        assert hi - lo > 34
        o[0, [lo, lo + 31, lo + 32, hi - 1]] = outside
        o[0, int(f[0]):int(f[1])] = outside[torch.arange(int(f[1]) - int(f[0]), device=o.device) % 4]
        lists["order_" + kind], lists["first_" + kind] = o, f
        live = [o[0, int(f[m]):int(f[m + 1])] for m in range(G)]
        live = [x[(x >= 0) & (x < n_record)] for x in live]
        assert [x.numel() for x in live] == [0, int(f[2]) - int(f[1]), hi - lo - 4]
        twin["order_" + kind] = torch.cat(live)[None, :].contiguous()
        twin["first_" + kind] = np.concatenate([[0], np.cumsum([x.numel() for x in live])]).astype(np.int32)
        ratio[kind] = [x.numel() / (int(f[m + 1]) - int(f[m])) for m, x in enumerate(live)]
    before = ref.state(env, G)
    w0 = ref.weights(env, G)
    out = env.ppo_update(rec, epochs=1, minibatch=ALL, lr=np.array([1e-3, 0.0, 0.0]), grad_clip=np.array([0.5, 0.0, 0.0]), adv_norm=None, order=lists, grad=True)
    after = ref.state(env, G)
    worst, misses = ref.check_against_twin(rec, lists, out, w0, [1, 2], "entries outside the record", "tanh", "tanh", ref.CASES[NATIVE][2],
                                           hp=dict(clip=0.2, vf_coeff=0.5, ent_coeff=0.01, adv_norm=False), twin_order=twin,
                                           scale=lambda kind, m: ratio[kind][m])
    assert 0.0 < worst <= 8.0
    assert not misses, misses
    for k in before:
        if "/0/" in k:
            if k.endswith("/t"):
                assert int(after[k][0]) == int(before[k][0]) + 1, k
            else:
                assert after[k].tobytes() == before[k].tobytes(), f"a list of outside entries moved {k}"
    assert not out["grad"][0].cpu().numpy().any()
    for name in ("policy_loss", "value_loss", "entropy", "kl", "clip_frac", "grad_norm", "rows"):
        assert np.all(out[name][0, :, 0] == 0.0), (name, out[name][0, :, 0])
    assert np.all(out["minibatches"][0, :, 0] == 1)
    assert all(np.isfinite(out[name]).all() for name in out if name != "grad") and bool(torch.isfinite(out["grad"]).all())
    assert all(np.isfinite(v).all() for v in after.values())
    env.close()


# ---- the edge of the LDS plan ---------------------------------------------------------------------------------------------------------
def test_one_step_beyond_the_lds_plan_is_refused_and_moves_nothing():
    """[512, 512, 96] at S 5 needs 170 496 bytes: ranenv_ppo_bind refuses it with RANENV_E_STATE and a text that says LDS, the refused
    handle's weights keep their bytes, and another, bound and trained handle keeps its whole state.  (On the refused handle itself the
    optimiser state is not readable: ranenv_ppo_state refuses as ranenv_ppo_bind does.)  The same handle then binds case A's nets,
    the largest the plan admits, at 162 304 bytes."""
    trained = _native_env([0, 6])
    rec = _native_record(trained)
    trained.ppo_update(rec, epochs=1, minibatch=ref.MINIBATCH, lr=1e-3, order=_order(rec, [0, 6], 1))
    kept = ref.state(trained, 1)
    assert kept["inter/0/m"].any() and int(kept["inter/0/t"][0]) > 0
    env = ref.native_workload(6)
    assert ref.lds_bytes(env.S, env.Us, "obs", [512, 512, 96], [512, 512, 96]) == 170496
    wide = ref.make_role_nets(env.S, env.Us, [512, 512, 96], "tanh", "obs", 77)
    env.set_policy_network(wide["inter"], wide["intra"], stochastic=True, seed=1, intra_input="obs")
    env.set_value_network(wide["v_inter"], wide["v_intra"])
    w_before = ref.weights(env, 1)
    code, text = ref.refusal(env.ppo_bind)
    assert code == E_STATE and "LDS" in text and "170496" in text, text
    assert ref.refusal(lambda: env.ppo_state("inter"))[0] == E_STATE
    assert ref.refusal(lambda: env.ppo_update(rec, epochs=1, order=_order(rec, [0, 6], 1)))[0] == E_STATE
    w_after = ref.weights(env, 1)
    for r in ref.ROLES:
        for (w0, b0), (w1, b1) in zip(w_before[r][0], w_after[r][0]):
            assert w0.tobytes() == w1.tobytes() and b0.tobytes() == b1.tobytes(), f"the refused binding moved {r}"
    ref.same_state(kept, ref.state(trained, 1), "a bound handle beside the refused one")
    S, Us, layout, (aw, aa), (cw, ca) = ref.SHAPES["A"]
    edge = ref.make_role_nets(env.S, env.Us, aw, aa, layout, 78, cw, ca)
    env.set_policy_network(edge["inter"], edge["intra"], stochastic=True, seed=1, intra_input=layout)
    env.set_value_network(edge["v_inter"], edge["v_intra"])
    env.ppo_bind()
    assert _lds_bytes(env) == 162304
    env.close()
    trained.close()


# ---- the population limit ---------------------------------------------------------------------------------------------------------------
def test_a_population_of_64_members_trains_each_member_alone():
    """POP_MAX members of one env each (B 64, T 4, [24] relu nets), one call with 64 different lr: members 0, 31 and 63 against the twin
    for the gradient and the statistics; against a twin handle updated by three calls that set epochs = 0 for all but one of them, their
    state bit for bit; on that handle three members that no call named keep their bytes.
    Measured on one MI355X, worst device error over the yardstick: 0.92."""
    case, n, T = "relu24", 64, 4
    first = list(range(n + 1))
    checked, idle = [0, 31, 63], [1, 30, 62]
    env_a, env_b = _native_env(first, case), _native_env(first, case)
    rec_a, rec_b = _native_record(env_a, T), _native_record(env_b, T)
    for k in rec_a:
        assert torch.equal(rec_a[k], rec_b[k]), k
    order = _order(rec_a, first, 1)
    lr = np.linspace(1e-4, 5e-3, n)
    w0 = ref.weights(env_a, checked)
    start = ref.state(env_b, checked + idle)
    out = env_a.ppo_update(rec_a, epochs=1, minibatch=ALL, lr=lr, order=order, grad=True)
    act, layout = ref.CASES[case][1], ref.CASES[case][2]
    worst, misses = ref.check_against_twin(rec_a, order, out, w0, checked, "64 members", act, act, layout)
    assert 0.0 < worst <= 8.0
    assert not misses, misses
    assert np.all(out["minibatches"][:, :, 0] == 1) and np.all(out["rows"][:, 0, 0] == T)
    for m in checked:
        env_b.ppo_update(rec_b, epochs=np.where(np.arange(n) == m, 1, 0), minibatch=ALL, lr=lr, order=order)
    ref.same_state(ref.state(env_a, checked), ref.state(env_b, checked), "one call against one call per member")
    end = ref.state(env_b, checked + idle)
    for k in end:
        m = int(k.split("/")[1])
        if m in idle:
            assert end[k].tobytes() == start[k].tobytes(), f"epochs = 0 moved {k}"
        elif k.split("/")[-1][0] == "w":
            assert end[k].tobytes() != start[k].tobytes(), f"{k} did not move"
    moved = ref.state(env_a, idle)
    assert all(moved[k].tobytes() != start[k].tobytes() for k in moved if k.endswith("/w0")), "the one call left a member untrained"
    env_a.close()
    env_b.close()
