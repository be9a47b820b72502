"""The WIDE binding of the PPO update on the device (ranenv_ppo_bind_wide / ranenv_ppo_update, the kernels
ranenv_ppo_update_kernel_wide and ranenv_ppo_update_kernel_mixed_wide): bit identity with the plain binding where both plans hold;
nets beyond the plain plan -- the reference's `verybig` [512, 512, 512] -- against the float64 twin; the loop inside one launch; a mixed
population that holds such a member; the boundary between the two bindings; determinism and the next collect().

Every case: B 12, T 8 (33 for the row tails), members of 2, 4 and 6 envs, S 5 / Us 5 or the shapes of tests/ppo_update_ref.py.
Tolerances are those of tests/test_gpu_ppo_update.py: the gradient within 8x the float32-torch error (floor 1e-6 relative), statistics
1e-6, Adam 4 float32 ulp, bit equality between bindings and schedules."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import collect_ref as cr
from tests import ppo_update_ref as ref
from tests import ppo_wide_ref as wd
from tests.gpu_common import need_gpu, shaped_workload, to_host

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -3
ALL = ref.ALL
G = wd.G
HP_LOOP = dict(lr=2e-3, clip=0.2, vf_coeff=0.5, ent_coeff=0.01, grad_clip=0.5)
KINDS = (("inter", "inter", "v_inter"), ("intra", "intra", "v_intra"))
# ref.CASES' tanh40x24 and every shape of ref.SHAPES that fits both plans (tests/test_ppo_wide_cpu.py holds that list to ref.SHAPES): A is
# the plain plan's own edge [512, 512, 32], C is S 16 with 2 S = 32 outputs and no padding, D is S 1
BOTH_PLANS = ["tanh40x24"] + list(wd.BOTH_PLANS_SHAPES)


def _order(rec, first, epochs, seed=3):
    from intent_radio_sched_multi_slice_amd.adapters import ppo_row_order
    return ppo_row_order(rec, first, epochs, seed)


def _both_plans_env(case, wide, first=ref.FIRST):
    """A reset env under a population of the case's nets (they fit both plans), bound wide or plain"""
    need_gpu()
    n = len(first) - 1
    if case in ref.CASES:
        env, nets, layout = ref.native_workload(first[-1]), ref.member_nets(case, n), ref.CASES[case][2]
    else:
        S, Us, layout, _, _ = ref.SHAPES[case]
        env, nets = shaped_workload(S, Us, first[-1], seed=40 + list(ref.SHAPES).index(case)).env, ref.shape_nets(case, n)
    env.set_population(first)
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=ref.SEED, intra_input=layout)
    env.set_value_network(nets["v_inter"], nets["v_intra"])
    env.ppo_bind(wide=wide)
    env.reset()
    return env


def _twin_records(env_a, env_b, T=ref.T):
    rec_a, rec_b = env_a.collect(T), env_b.collect(T)
    torch.cuda.synchronize()
    for k in rec_a:
        assert torch.equal(rec_a[k], rec_b[k]), k
    return rec_a, rec_b


def _same_call(env_a, out_a, env_b, out_b, members, what):
    """Weights, m, v, counters, all eight statistics and dev_grad of two handles behind the same call, byte for byte"""
    ref.same_state(ref.state(env_a, members), ref.state(env_b, members), what)
    assert out_a.keys() == out_b.keys()
    for name in out_a:
        if name == "grad":
            assert torch.equal(out_a[name], out_b[name]), f"{what}: dev_grad differs"
            assert bool(out_a[name].any())
        else:
            assert np.asarray(out_a[name]).tobytes() == np.asarray(out_b[name]).tobytes(), f"{what}: statistics {name} differ"


# ---- 1. bit identity where both plans hold ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BOTH_PLANS)
def test_the_wide_binding_equals_the_plain_one_bit_for_bit_where_both_plans_hold(case):
    """Two epochs of minibatches of 12 on twin handles, one bound wide and one plain: four and five layers, a 7-wide bottleneck, odd
    widths, a critic shallower or deeper than the actor, both activations; row tails, several minibatches, the launch re-reading its
    own weights.  The wide handle reports the wide plan's LDS bytes, the plain one the plain plan's."""
    env_w, env_p = _both_plans_env(case, True), _both_plans_env(case, False)
    rec_w, rec_p = _twin_records(env_w, env_p)
    order = _order(rec_w, ref.FIRST, 2)
    start = ref.state(env_w, G)
    hp = dict(epochs=2, minibatch=ref.MINIBATCH, order=order, grad=True, **HP_LOOP)
    out_w, out_p = env_w.ppo_update(rec_w, **hp), env_p.ppo_update(rec_p, **hp)
    _same_call(env_w, out_w, env_p, out_p, G, f"{case}: wide against plain")
    end = ref.state(env_w, G)
    assert all(end[k].tobytes() != start[k].tobytes() for k in end if k.split("/")[-1][0] == "w"), "a weight matrix did not move"
    assert np.all(out_w["minibatches"][:, 0, :] >= 2)
    for kind in ("inter", "intra"):
        for m in range(G):
            assert env_w.ppo_member_layout(m, kind)["lds_bytes"] <= wd.WIDE_LDS_MAX
            assert env_w.ppo_member_layout(m, kind)["lds_bytes"] < env_p.ppo_member_layout(m, kind)["lds_bytes"] <= ref.LDS_MAX
    env_w.close()
    env_p.close()


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


def test_row_tails_and_entries_outside_the_record_equal_the_plain_binding():
    """Lists of 1, 31, 32, 33, 64 and 65 rows in minibatches of 32 under adv_norm "minibatch", then the same lists with entries outside
    the record (-1, n_record, n_record + 7, 2^31 - 1) planted at their heads and tails: wide against plain, byte for byte."""
    case, n = "tanh40x24", len(TAILS)
    env_w, env_p = _both_plans_env(case, True, TAIL_FIRST), _both_plans_env(case, False, TAIL_FIRST)
    rec_w, rec_p = _twin_records(env_w, env_p, 33)
    lists = _cut(_order(rec_w, TAIL_FIRST, 1), TAILS)
    hp = dict(epochs=1, minibatch=32, order=lists, grad=True, adv_norm="minibatch", **HP_LOOP)
    out_w, out_p = env_w.ppo_update(rec_w, **hp), env_p.ppo_update(rec_p, **hp)
    _same_call(env_w, out_w, env_p, out_p, n, "row tails: wide against plain")
    assert np.array_equal(out_w["rows"][:, :, 0], np.repeat(np.array(TAILS)[:, None], 2, 1))
    T, B, S = rec_w["mask_inter"].shape
    outside = {}
    for kind, n_record in (("inter", T * B), ("intra", T * B * S)):
        f, o = lists["first_" + kind], lists["order_" + kind].clone()
        bad = torch.tensor([-1, n_record, n_record + 7, 2 ** 31 - 1], dtype=torch.int32, device=o.device)
        for m in range(1, n):            # (member 0's one row stays; the others lose their first and, from 33 rows on, their 33rd and last entry)
            lo, hi = int(f[m]), int(f[m + 1])
            o[0, lo] = bad[m % 4]
            if hi - lo > 32:
                o[0, lo + 32], o[0, hi - 1] = bad[(m + 1) % 4], bad[(m + 2) % 4]
        outside["order_" + kind], outside["first_" + kind] = o, f
    hp = dict(hp, order=outside, adv_norm=None)
    out_w, out_p = env_w.ppo_update(rec_w, **hp), env_p.ppo_update(rec_p, **hp)
    _same_call(env_w, out_w, env_p, out_p, n, "entries outside the record: wide against plain")
    assert np.all(out_w["rows"][1:, :, 0] < np.array(TAILS)[1:, None]) and np.all(out_w["rows"][1:, :, 0] > 0)
    assert all(np.isfinite(np.asarray(out_w[k])).all() for k in out_w if k != "grad") and bool(torch.isfinite(out_w["grad"]).all())
    env_w.close()
    env_p.close()


# ---- 2. beyond the plain plan ---------------------------------------------------------------------------------------------------------------
def _beyond_env(case, stochastic=True):
    """A reset env of the native shape under a population of the BEYOND case's nets, bound wide"""
    env = ref.native_workload(wd.FIRST[-1])
    nets = wd.beyond_nets(case)
    env.set_population(wd.FIRST)
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=stochastic, seed=ref.SEED, intra_input=wd.BEYOND[case][2])
    env.set_value_network(nets["v_inter"], nets["v_intra"])
    env.ppo_bind(wide=True)
    env.reset()
    return env


def _on_device(env, d):
    return {k: (v.to(env.device) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


@pytest.mark.parametrize("case", list(wd.BEYOND))
def test_nets_beyond_the_plain_plan_against_the_float64_twin(case):
    """[512, 512, 512] tanh, [512, 512, 96] relu and [512, 512, 512, 512] tanh (`deepest`: the largest net the acting path accepts, five
    layers of parked rows) actors and critics, inter and intra, members of 2 / 4 / 6 envs.  One minibatch of
    all rows at lr 0: dev_grad per layer tensor (padding exact zeros) within 8x the float32-torch yardstick of the float64 twin and
    the five statistics within 1e-6; then one Adam step within 4 float32 ulp of ref.adam_step_f32 on the device's own gradient, the
    padding of m and v exact zeros, the counters reading 1.  The launch's LDS bytes are the restated wide formula.
    Measured on one MI355X, worst device error over the yardstick: 1.72 (verybig), 0.93 (past_limit), 1.77 (deepest); Adam 0 ulp on
    all 6 544 941 / 3 980 685 / 9 696 813 weights and on their moments."""
    widths, act, layout = wd.BEYOND[case]
    env = _beyond_env(case)
    rec, order = _on_device(env, wd.beyond_record(case)), _on_device(env, wd.order(wd.beyond_record(case), 1))
    out = env.ppo_update(rec, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, order=order, grad=True)
    weights = ref.weights(env, G)
    worst, misses = ref.check_against_twin(rec, order, out, weights, range(G), case, act, act, layout)
    assert 0.0 < worst <= 8.0
    assert not misses, misses
    assert np.all((out["clip_frac"][:, :, 0] > 0.0) & (out["clip_frac"][:, :, 0] < 1.0)), "rows on both sides of the clip"
    for kind, dims in wd.kind_dims(widths, layout).items():
        for m in range(G):
            assert env.ppo_member_layout(m, kind)["lds_bytes"] == wd.wide_lds_bytes(*dims) <= wd.WIDE_LDS_MAX
    env.ppo_bind(wide=True)            # (lr 0 moved no weight, but it took an optimiser step: moments and counters start again)
    hp = dict(lr=np.array([3e-4, 1e-3, 5e-3]), grad_clip=np.array([0.5, 0.05, 0.0]), betas=(0.9, 0.999), eps=1e-8)
    out = env.ppo_update(rec, epochs=1, minibatch=ALL, order=order, grad=True, **hp)
    w1 = ref.weights(env, G)
    ref.check_adam_step(env, out, weights, w1, hp, G, case)
    for r in ref.ROLES:
        assert all(not np.array_equal(x[0], y[0]) for m in range(G) for x, y in zip(weights[r][m], w1[r][m])), f"a layer of {r} did not move"
    env.close()


# ---- 3. the loop inside one launch ----------------------------------------------------------------------------------------------------------
def test_the_loop_inside_one_launch_equals_one_minibatch_per_launch_on_verybig():
    """2 epochs of minibatches of 12 in ONE call against the same chunks one call each on a twin handle: weights, moments and counters
    bit for bit -- a stale read of the weights, or of rows parked by an earlier tile or net, would show here."""
    case, E, MB = "verybig", 2, wd.MINIBATCH
    env_a, env_b = _beyond_env(case), _beyond_env(case)
    rec_a, rec_b = _on_device(env_a, wd.beyond_record(case)), _on_device(env_b, wd.beyond_record(case))
    order = _on_device(env_a, wd.order(wd.beyond_record(case), E))
    start = ref.state(env_a, G)
    out = env_a.ppo_update(rec_a, epochs=E, minibatch=MB, order=order, **HP_LOOP)
    n_chunks = [[-(-(int(f[m + 1]) - int(f[m])) // MB) for m in range(G)] for f in (order["first_inter"], order["first_intra"])]
    for kind_i in range(2):
        assert np.array_equal(out["minibatches"][:, kind_i, :], np.repeat(np.array(n_chunks[kind_i])[:, None], E, 1))
    assert min(n_chunks[0]) >= 2
    for ep in range(E):
        for i in range(max(max(n_chunks[0]), max(n_chunks[1]))):
            env_b.ppo_update(rec_b, epochs=1, minibatch=ALL, order=ref.chunk_order(order, G, MB, ep, i), **HP_LOOP)
    a, b = ref.state(env_a, G), ref.state(env_b, G)
    ref.same_state(a, b, "verybig: one call against one call per chunk")
    assert all(a[k].tobytes() != start[k].tobytes() for k in a if k.split("/")[-1][0] == "w"), "a weight matrix did not move"
    for m in range(G):
        assert int(a[f"inter/{m}/t"][0]) == E * n_chunks[0][m] and int(a[f"intra/{m}/t"][0]) == E * n_chunks[1][m]
    env_a.close()
    env_b.close()


# ---- 4. mixed wide ------------------------------------------------------------------------------------------------------------------------------
def _bind_nets(env, nets, mixed):
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=ref.SEED, intra_input=wd.MIXED_LAYOUT, mixed=mixed)
    env.set_value_network(nets["v_inter"], nets["v_intra"], mixed=mixed)


def _population_env(nets, mixed, wide):
    env = ref.native_workload(wd.FIRST[-1])
    env.set_population(wd.FIRST)
    _bind_nets(env, nets, mixed)
    env.ppo_bind(mixed=mixed, wide=wide)
    env.reset()
    return env


def _same_member(a, out_a, b, out_b, m, what, layouts=True):
    """Member m of two handles after the same call: weights, m, v, t, the statistics rows and the dev_grad block byte for byte; the
    block is compared up to actor + critic floats, the rest of handle ``a``'s is exact zeros"""
    ref.same_state(ref.state(a, [m]), ref.state(b, [m]), what)
    for name in out_a:
        if name != "grad":
            assert out_a[name][m].tobytes() == out_b[name][m].tobytes(), f"{what}: statistics {name} of member {m} differ"
    ga, gb = out_a["grad"][m].cpu().numpy(), out_b["grad"][m].cpu().numpy()
    for kind_i, (kind, _, _) in enumerate(KINDS):
        lay, lay_b = a.ppo_member_layout(m, kind), b.ppo_member_layout(m, kind)
        assert (lay == lay_b) if layouts else (lay["actor"], lay["critic"]) == (lay_b["actor"], lay_b["critic"]), (what, kind)
        n = lay["actor"] + lay["critic"]
        assert 0 < n <= ga.shape[1] and n <= gb.shape[1]
        assert ga[kind_i, :n].tobytes() == gb[kind_i, :n].tobytes(), f"{what}: dev_grad of member {m}, {kind}, differs"
        assert ga[kind_i, :n].any(), f"{what}: dev_grad of member {m}, {kind}, is all zeros"
        assert not ga[kind_i, n:].any(), f"{what}: dev_grad of member {m}, {kind}, is written behind its {n} floats"


MIXED_HP = dict(epochs=2, minibatch=wd.MINIBATCH, lr=np.array([1e-3, 3e-4, 2e-3]), grad_clip=np.array([0.5, 0.05, 0.0]))


def test_a_mixed_wide_population_with_a_verybig_member():
    """Members [64, 64], [512, 512, 512] and [256, 256, 256] under ppo_bind(mixed=True, wide=True), two epochs of minibatches of 12:
    member m's weights, moments, counter, statistics and gradient are bit for bit those of a uniform wide population of m's shape on
    the same rows, and members 0 and 2 -- the two that fit the plain plan -- equal the plain mixed binding's."""
    env = _population_env(wd.mixed_nets(), True, True)
    rec, order = _on_device(env, wd.mixed_record()), _on_device(env, wd.order(wd.mixed_record(), 2))
    out = env.ppo_update(rec, order=order, grad=True, **MIXED_HP)
    for m in range(G):
        twin = _population_env(wd.twin_nets(m), False, True)
        out_t = twin.ppo_update(_on_device(twin, wd.mixed_record()), order=order, grad=True, **MIXED_HP)
        _same_member(env, out, twin, out_t, m, f"mixed wide member {m} against its uniform wide twin")
        twin.close()
    lay = [env.ppo_member_layout(i, k) for i in range(G) for k in ("inter", "intra")]
    assert out["grad"].shape[2] == max(x["actor"] + x["critic"] for x in lay)
    for (w, _), i in zip(wd.MIXED, range(G)):
        for kind, dims in wd.kind_dims(w, wd.MIXED_LAYOUT).items():
            assert env.ppo_member_layout(i, kind)["lds_bytes"] == wd.wide_lds_bytes(*dims)
    # the plain mixed binding of a population whose member 1 fits the plain plan: members 0 and 2 see the same rows
    small = [wd.MIXED[0], ([24], "relu"), wd.MIXED[2]]
    plain = _population_env(wd.mixed_nets(small), True, False)
    out_p = plain.ppo_update(_on_device(plain, wd.mixed_record()), order=order, grad=True, **MIXED_HP)
    for m in (0, 2):
        _same_member(plain, out_p, env, out, m, f"member {m}: the plain mixed binding against the wide one", layouts=False)
    plain.close()
    env.close()


def _sequentials(env, m):
    return {r: ref.as_sequential([(w.cpu(), b.cpu()) for w, b in env.net_weights(r, m)], env.net_activation(r, m)) for r in ref.ROLES}


def test_rebinding_members_across_the_two_plans_under_a_mixed_wide_binding():
    """PBT's copy across architectures under the wide binding: the [512] x 3 member into the [64, 64] member's place and the [64, 64]
    winner into the [512] x 3 member's -- moments zero over the extent's used floats, counter 0, the other members' bytes kept, and
    one more update of the re-bound member equals a fresh uniform wide twin of that shape.  A re-bind that parks more rows than the
    bind allocated, or that is larger than the extent, is refused and moves nothing."""
    env = _population_env(wd.mixed_nets(), True, True)
    rec, order = _on_device(env, wd.mixed_record()), _on_device(env, wd.order(wd.mixed_record(), 1))
    env.ppo_update(rec, epochs=1, minibatch=wd.MINIBATCH, lr=1e-3, order=order)
    before = ref.state(env, G)
    assert all(before[f"{r}/{m}/m"].any() and int(before[f"{r}/{m}/t"][0]) > 0 for r in ref.ROLES for m in range(G))
    # the refusals first: every byte stays
    grown = ref.make_role_nets(wd.S, wd.US, wd.OUTGROWS_SCRATCH, "tanh", wd.MIXED_LAYOUT, 91)
    code, text = ref.refusal(lambda: env.set_population_member(0, inter=grown["inter"]))
    assert code == E_STATE and "member 0" in text and "park" in text, text
    huge = ref.make_role_nets(wd.S, wd.US, wd.OUTGROWS_EXTENT, "tanh", wd.MIXED_LAYOUT, 92)
    code, text = ref.refusal(lambda: env.set_population_member(0, inter=huge["inter"]))
    assert code == E_INVALID and "extent" in text, text
    ref.same_state(before, ref.state(env, G), "refused re-binds")
    # member 1 ([512] x 3) into member 0's place, then the old member 0 ([64, 64]) into member 1's
    big, small = _sequentials(env, 1), _sequentials(env, 0)
    hidden = {(r, m): env.population_net(r, m)["hidden"] for r in ref.ROLES for m in range(G)}
    assert hidden["inter", 1] == wd.MIXED[1][0] and hidden["inter", 0] == wd.MIXED[0][0]
    env.set_population_member(0, **big)
    env.set_population_member(1, **small)
    after = ref.state(env, G)
    for dst, src in ((0, 1), (1, 0)):
        for r in ref.ROLES:
            assert env.population_net(r, dst)["hidden"] == hidden[r, src]
            assert not after[f"{r}/{dst}/m"].any() and not after[f"{r}/{dst}/v"].any() and int(after[f"{r}/{dst}/t"][0]) == 0, (r, dst)
            n_layers = len([k for k in after if k.startswith(f"{r}/{dst}/w")])
            assert n_layers == len([k for k in before if k.startswith(f"{r}/{src}/w")])
            for i in range(n_layers):
                assert after[f"{r}/{dst}/w{i}"].tobytes() == before[f"{r}/{src}/w{i}"].tobytes() and after[f"{r}/{dst}/b{i}"].tobytes() == before[f"{r}/{src}/b{i}"].tobytes()
    for k in before:
        if "/2/" in k:
            assert before[k].tobytes() == after[k].tobytes(), f"re-binding members 0 and 1 moved {k}"
    for dst, shape in ((0, 1), (1, 0)):
        twin = _population_env(wd.twin_nets(shape), False, True)
        twin.set_population_member(dst, **(big if dst == 0 else small))
        twin.ppo_bind(wide=True)
        hp = dict(epochs=np.where(np.arange(G) == dst, 1, 0), minibatch=wd.MINIBATCH, lr=2e-3, order=order, grad=True)
        out, out_t = env.ppo_update(rec, **hp), twin.ppo_update(_on_device(twin, wd.mixed_record()), **hp)
        _same_member(env, out, twin, out_t, dst, f"member {dst} in member {shape}'s shape")
        twin.close()
    env.close()


# ---- 5. the boundary ----------------------------------------------------------------------------------------------------------------------------
def test_the_boundary_between_the_plain_and_the_wide_binding():
    """ppo_bind() still refuses [512] x 3; the wide entries keep their counterparts' refusals in their words -- uniform against mixed,
    bf16, nets per slice, the head policy -- and the handle's weights keep their bytes; wide and head exclude each other in the binding;
    a plain ppo_bind() behind a wide one gives the state of a fresh plain binding."""
    from intent_radio_sched_multi_slice_amd import _lib
    env = ref.native_workload(wd.FIRST[-1])
    layout = wd.BEYOND["verybig"][2]
    big = wd.beyond_nets("verybig")
    one = {r: big[r][0] for r in ref.ROLES}
    env.set_policy_network(one["inter"], one["intra"], stochastic=True, seed=1, intra_input=layout)
    env.set_value_network(one["v_inter"], one["v_intra"])
    w_before = ref.weights(env, 1)
    code, text = ref.refusal(env.ppo_bind)
    assert code == E_STATE and "LDS" in text and "219648" in text, text
    with pytest.raises(ValueError):
        env.ppo_bind(head=True, wide=True)
    # a plain handle is no mixed population
    code, text = ref.refusal(lambda: env.ppo_bind(mixed=True, wide=True))
    assert code == E_STATE and "ranenv_ppo_bind_mixed trains a mixed population" in text, text
    # intra nets per slice
    env.set_policy_network(one["inter"], [one["intra"]] * env.S, stochastic=True, seed=1, intra_input=layout)
    code, text = ref.refusal(lambda: env.ppo_bind(wide=True))
    assert code == E_STATE and "per slice" in text, text
    # bf16
    env.set_policy_network(one["inter"], one["intra"], stochastic=True, seed=1, intra_input=layout, precision="bf16")
    code, text = ref.refusal(lambda: env.ppo_bind(wide=True))
    assert code == E_STATE and "bf16" in text, text
    env.set_policy_network(one["inter"], one["intra"], stochastic=True, seed=1, intra_input=layout)
    w_after = ref.weights(env, 1)
    for r in ref.ROLES:
        for (w0, b0), (w1, b1) in zip(w_before[r][0], w_after[r][0]):
            assert w0.tobytes() == w1.tobytes() and b0.tobytes() == b1.tobytes(), f"a refused binding moved {r}"
    # the head policy: the plain entry's words
    env.set_policy(_lib.POLICY_HEAD_NETWORK)
    code, plain_text = ref.refusal(env.ppo_bind)
    code_w, text_w = ref.refusal(lambda: env.ppo_bind(wide=True))
    assert code == code_w == E_STATE and "RANENV_POLICY_HEAD_NETWORK" in text_w
    assert text_w.split(": ", 1)[1] == plain_text.split(": ", 1)[1]
    env.set_policy(_lib.POLICY_NETWORK)
    # a uniform population under the mixed wide entry, a mixed one under the uniform wide entry
    env.set_population(wd.FIRST)
    env.set_policy_network(big["inter"], big["intra"], stochastic=True, seed=1, intra_input=layout)
    env.set_value_network(big["v_inter"], big["v_intra"])
    code, text = ref.refusal(lambda: env.ppo_bind(mixed=True, wide=True))
    assert code == E_STATE and "no bound role is mixed" in text, text
    env.ppo_bind(wide=True)
    mixed = wd.mixed_nets()
    _bind_nets(env, mixed, True)
    code, text = ref.refusal(lambda: env.ppo_bind(wide=True))
    assert code == E_STATE and "does not train a mixed population: use ranenv_ppo_bind_mixed" in text, text
    rec = _on_device(env, wd.mixed_record())
    order = _on_device(env, wd.order(wd.mixed_record(), 1))
    assert ref.refusal(lambda: env.ppo_update(rec, epochs=1, order=order))[0] == E_STATE      # (the uniform wide binding of a moment ago)
    env.close()
    # a plain bind behind a wide one: the state of a fresh plain binding
    case = "tanh40x24"
    env_a, env_b = _both_plans_env(case, True), _both_plans_env(case, False)
    rec_a, rec_b = _twin_records(env_a, env_b)
    order = _order(rec_a, ref.FIRST, 1)
    env_a.ppo_update(rec_a, epochs=1, minibatch=ref.MINIBATCH, lr=0.0, order=order)      # (moves moments and counters, no weight)
    assert int(ref.state(env_a, [0])["inter/0/t"][0]) > 0
    env_a.ppo_bind()
    ref.same_state(ref.state(env_a, G), ref.state(env_b, G), "a plain bind behind a wide one")
    assert env_a.ppo_member_layout(0, "inter") == env_b.ppo_member_layout(0, "inter")
    hp = dict(epochs=1, minibatch=ref.MINIBATCH, order=order, grad=True, **HP_LOOP)
    _same_call(env_a, env_a.ppo_update(rec_a, **hp), env_b, env_b.ppo_update(rec_b, **hp), G, "the plain binding behind a wide one")
    env_a.close()
    env_b.close()


# ---- 6. determinism and acting ------------------------------------------------------------------------------------------------------------------
def test_the_same_wide_call_gives_the_same_bytes_and_the_next_collect_acts_on_the_trained_verybig_nets():
    """Twin handles under [512] x 3 nets, a deterministic collect(8): the re-evaluated logp (probe_logp) equals the recorded one to the
    bit at unchanged weights, as in the plain path; the same training call gives the same bytes on both; and a second collect, with no
    rebind, records what the float64 checks of tests/collect_ref.py accept for the weights read back, member by member."""
    case = "verybig"
    layout = wd.BEYOND[case][2]
    env_a, env_b = _beyond_env(case, stochastic=False), _beyond_env(case, stochastic=False)
    rec_a, rec_b = _twin_records(env_a, env_b)
    order = _order(rec_a, wd.FIRST, 2)
    probe = env_a.ppo_update(rec_a, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, order=order, probe_logp=True)
    env_b.ppo_update(rec_b, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, order=order)
    new, old, mask = probe["logp"].cpu().numpy(), rec_a["logp"].cpu().numpy(), rec_a["mask_inter"].cpu().numpy() != 0
    assert np.array_equal(new[..., 0].view(np.int32), old[..., 0].view(np.int32))
    assert np.array_equal(new[..., 1:][mask].view(np.int32), old[..., 1:][mask].view(np.int32))
    assert np.all(probe["clip_frac"][:, :, 0] == 0.0)
    start = ref.state(env_a, G)
    hp = dict(epochs=2, minibatch=wd.MINIBATCH, lr=3e-3, order=order, grad=True)
    _same_call(env_a, env_a.ppo_update(rec_a, **hp), env_b, env_b.ppo_update(rec_b, **hp), G, "the same wide call on twin handles")
    trained = ref.state(env_a, G)
    assert all(trained[k].tobytes() != start[k].tobytes() for k in trained if k.split("/")[-1][0] == "w")
    v = env_a.views()
    episode, step0 = v["episode_number"].cpu().numpy().copy(), v["step_number"].cpu().numpy().copy()
    rec2 = to_host(env_a.collect(3))
    for m, sl in enumerate(env_a.population_slices()):
        seq = _sequentials(env_a, m)
        mine = {k: x[:, sl] for k, x in rec2.items()}
        for t in range(3):
            r, _ = cr.check_actor_record(mine, t, seq["inter"], seq["intra"], False, ref.SEED, episode[sl], step0[sl] + t, layout)
            r["vf"] = cr.check_values(mine["vf"][t], mine["obs_inter"][t], mine["obs_intra"][t], mine["mask_intra"][t], seq["v_inter"], seq["v_intra"], layout)
            print(f"member {m} slot {t}: worst error / bound after the wide update: {r}")
    env_a.close()
    env_b.close()
