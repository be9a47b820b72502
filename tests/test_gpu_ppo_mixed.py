"""The PPO update of MIXED populations on the device (ranenv_ppo_bind_mixed / ranenv_ppo_update, the kernel
ranenv_ppo_update_kernel_mixed): every member against the uniform population of its own shape that the repository already tests, bit
for bit; against the float64 twin per member; the loop inside one launch; re-binding a member into another shape; the next collect();
the refusals; 64 members.  The cases, the nets and the record are tests/ppo_mixed_ref.py's: S 5 / Us 5, B 12, T 8, members of 16, 32
and 48 inter rows, minibatch 12."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import collect_ref as cr
from tests import ppo_mixed_ref as mx
from tests import ppo_update_ref as ref
from tests.gpu_common import to_host

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -3
ALL = ref.ALL
G3 = len(mx.FIRST) - 1
KINDS = (("inter", "inter", "v_inter"), ("intra", "intra", "v_intra"))


def _bind(env, nets, case, mixed, stochastic=True):
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=stochastic, seed=ref.SEED, intra_input=mx.layout(case), mixed=mixed)
    env.set_value_network(nets["v_inter"], nets["v_intra"], mixed=mixed)


def _mixed_env(case, first=mx.FIRST, G=None, stochastic=True):
    """A reset env under the case's mixed population, PPO state bound"""
    env = ref.native_workload(first[-1])
    env.set_population(first)
    _bind(env, mx.mixed_nets(case, G), case, True, stochastic)
    env.ppo_bind(mixed=True)
    env.reset()
    return env


def _twin_env(case, m, first=mx.FIRST, G=None):
    """... under the UNIFORM population of member m's shape with m's weights at position m, bound by the plain ranenv_ppo_bind"""
    env = ref.native_workload(first[-1])
    env.set_population(first)
    _bind(env, mx.twin_nets(case, m, G), case, False)
    env.ppo_bind()
    env.reset()
    return env


def _on_device(env, d):
    return {k: (v.to(env.device) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def _record(env, case, first=mx.FIRST, G=None):
    return _on_device(env, mx.record(case, first, G))


def _order(env, case, epochs, first=mx.FIRST, G=None):
    return _on_device(env, mx.order(case, epochs, first, G))


def _same_member(a, out_a, b, out_b, m, what):
    """Member m of handle ``a`` (mixed) and of handle ``b`` (its twin) after the same call: weights, m, v, t, the statistics rows and the
    dev_grad block byte for byte; the block is compared up to actor + critic floats, the rest of the mixed handle's is exact zeros"""
    ref.same_state(ref.state(a, [m]), ref.state(b, [m]), what)
    for name in out_a:
        if name != "grad":
            assert out_a[name][m].tobytes() == out_b[name][m].tobytes(), f"{what}: statistics {name} of member {m} differ"
    ga, gb = out_a["grad"][m].cpu().numpy(), out_b["grad"][m].cpu().numpy()
    for kind_i, (kind, _, _) in enumerate(KINDS):
        lay = a.ppo_member_layout(m, kind)
        assert lay == b.ppo_member_layout(m, kind), (what, kind)
        n = lay["actor"] + lay["critic"]
        assert 0 < n <= ga.shape[1] and n <= gb.shape[1]
        assert ga[kind_i, :n].tobytes() == gb[kind_i, :n].tobytes(), f"{what}: dev_grad of member {m}, {kind}, differs"
        assert ga[kind_i, :n].any(), f"{what}: dev_grad of member {m}, {kind}, is all zeros"
        assert not ga[kind_i, n:].any(), f"{what}: dev_grad of member {m}, {kind}, is written behind its {n} floats"


LOOP_HP = dict(epochs=2, minibatch=mx.MINIBATCH, lr=np.array([1e-3, 3e-4, 2e-3]), grad_clip=np.array([0.5, 0.05, 0.0]))
_RUNS = {}


def _mixed_run(case):
    """The case's mixed handle behind ONE call of two epochs x minibatches of 12 with per-member lr / grad_clip: (env, out, order)"""
    if case not in _RUNS:
        env = _mixed_env(case)
        order = _order(env, case, 2)
        before = ref.state(env, G3)
        out = env.ppo_update(_record(env, case), order=order, grad=True, **LOOP_HP)
        after = ref.state(env, G3)
        for m in range(G3):
            assert any(before[k].tobytes() != after[k].tobytes() for k in before if k.startswith(f"inter/{m}/w")), f"member {m} did not move"
        _RUNS[case] = (env, out, order)
    return _RUNS[case]


@pytest.mark.parametrize("m", range(G3))
@pytest.mark.parametrize("case", list(mx.CASES))
def test_a_member_equals_the_uniform_population_of_its_own_shape_bit_for_bit(case, m):
    env, out, order = _mixed_run(case)
    twin = _twin_env(case, m)
    out_t = twin.ppo_update(_record(twin, case), order=order, grad=True, **LOOP_HP)
    _same_member(env, out, twin, out_t, m, f"{case} member {m}")
    # (the launch's figures: the largest member's)
    lay = [env.ppo_member_layout(i, k) for i in range(G3) for k in ("inter", "intra")]
    assert out["grad"].shape[2] == max(x["actor"] + x["critic"] for x in lay)
    twin.close()


@pytest.mark.parametrize("case", list(mx.CASES))
def test_gradient_statistics_and_one_adam_step_against_the_twins_per_member(case):
    """One minibatch of all rows at lr 0: dev_grad per layer tensor within 8x the float32-torch yardstick of the float64 twin (floor
    1e-6) and the five statistics within 1e-6, member by member under the member's own activations (ref.check_against_twin's figures);
    then one Adam step within 4 float32 ulp of ref.adam_step_f32 on the device's own gradient, the counters reading 1.
    Measured on one MI355X: worst gradient tensor 0.19 / 0.84 / 0.31 (base) and 1.20 / 0.46 / 1.58 (edge) of the yardstick per member;
    Adam 0 ulp on all 16 629 / 1 228 751 weights and on their moments."""
    env = _mixed_env(case)
    rec, order = _record(env, case), _order(env, case, 1)
    out = env.ppo_update(rec, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, order=order, grad=True)
    weights = ref.weights(env, G3)
    misses = []
    for m, (_, aa, _, ca) in enumerate(mx.shapes(case)):
        worst, miss = ref.check_against_twin(rec, order, out, weights, [m], f"{case} member {m}", aa, ca, mx.layout(case))
        assert 0.0 < worst <= 8.0
        misses += miss
    assert not misses, misses
    assert np.all((out["clip_frac"][:, :, 0] > 0.0) & (out["clip_frac"][:, :, 0] < 1.0)), "rows on both sides of the clip"
    env.ppo_bind(mixed=True)            # (lr 0 moved no weight, but it took an optimiser step: moments and counters start again)
    hp = dict(lr=np.array([3e-4, 1e-3, 5e-3]), grad_clip=np.array([0.5, 0.05, 0.0]), betas=(0.9, 0.999), eps=1e-8)
    out = env.ppo_update(rec, epochs=1, minibatch=ALL, order=order, grad=True, **hp)
    ref.check_adam_step(env, out, weights, ref.weights(env, G3), hp, G3, case)
    env.close()


def test_the_loop_inside_one_launch_equals_one_minibatch_per_launch():
    """Two epochs x k minibatches in ONE call against one call per chunk on a twin mixed handle: weights, moments, counters bit for bit"""
    case = "base"
    env_a, _, order = _mixed_run(case)
    env_b = _mixed_env(case)
    rec = _record(env_b, case)
    n_chunks = max(-(-(int(f[m + 1]) - int(f[m])) // mx.MINIBATCH) for f in (order["first_inter"], order["first_intra"]) for m in range(G3))
    assert n_chunks >= 4
    hp = dict(LOOP_HP, epochs=1, minibatch=ALL)
    for ep in range(2):
        for i in range(n_chunks):
            env_b.ppo_update(rec, order=ref.chunk_order(order, G3, mx.MINIBATCH, ep, i), **hp)
    ref.same_state(ref.state(env_a, G3), ref.state(env_b, G3), "one call against one call per chunk")
    env_b.close()


def _extent_view(env, role, m, name):
    """Adam's ``name`` ("m" / "v") of member m's WHOLE extent of ``role``, beyond the floats its net uses now"""
    from intent_radio_sched_multi_slice_amd.batched_env import _DevArray
    st, extent = env.ppo_state(role, m), env.population_net(role, m)["extent"]
    assert st[name].numel() == env.population_net(role, m)["used"] <= extent
    return torch.as_tensor(_DevArray(st[name].data_ptr(), (extent,), "f4", env), device=env.device).cpu().numpy()


def test_rebinding_a_member_into_another_shape_restarts_its_optimiser_over_the_whole_extent():
    """PBT's copy across architectures: member 0's trained nets into member 1.  Member 1's moments read zero over its whole extent and
    its counter 0; members 0 and 2 keep every byte; one more update of member 1 equals a fresh uniform twin of that shape, bit for bit."""
    case = "base"
    env = _mixed_env(case)
    rec, order = _record(env, case), _order(env, case, 1)
    env.ppo_update(rec, epochs=1, minibatch=mx.MINIBATCH, lr=1e-3, order=order)
    before = ref.state(env, G3)
    assert all(before[f"{r}/1/m"].any() and before[f"{r}/1/v"].any() and int(before[f"{r}/1/t"][0]) > 0 for r in ref.ROLES)
    tails = {r: _extent_view(env, r, 1, "v") for r in ref.ROLES}
    src = {r: ref.as_sequential([(w.cpu(), b.cpu()) for w, b in env.net_weights(r, 0)], env.net_activation(r, 0)) for r in ref.ROLES}
    used0 = {r: env.population_net(r, 0)["used"] for r in ref.ROLES}
    # (member 1's old shape used more floats than member 0's: moments of the old shape lie behind the new one's end)
    assert any(tails[r][used0[r]:].any() for r in ref.ROLES)
    env.set_population_member(1, **src)
    after = ref.state(env, G3)
    for r in ref.ROLES:
        assert env.population_net(r, 1)["hidden"] == env.population_net(r, 0)["hidden"] and env.net_activation(r, 1) == env.net_activation(r, 0)
        assert not _extent_view(env, r, 1, "m").any() and not _extent_view(env, r, 1, "v").any(), f"{r}: stale moments in member 1's extent"
        assert int(after[f"{r}/1/t"][0]) == 0
        for i in range(len(src[r]) // 2 + 1):
            assert after[f"{r}/1/w{i}"].tobytes() == before[f"{r}/0/w{i}"].tobytes() and after[f"{r}/1/b{i}"].tobytes() == before[f"{r}/0/b{i}"].tobytes()
    for k in before:
        if "/0/" in k or "/2/" in k:
            assert before[k].tobytes() == after[k].tobytes(), f"re-binding member 1 moved {k}"
    twin = _twin_env(case, 0)
    twin.set_population_member(1, **src)
    twin.ppo_bind()
    hp = dict(epochs=np.array([0, 1, 0]), minibatch=mx.MINIBATCH, lr=2e-3, order=order, grad=True)
    out, out_t = env.ppo_update(rec, **hp), twin.ppo_update(_record(twin, case), **hp)
    _same_member(env, out, twin, out_t, 1, "member 1 in member 0's shape")
    twin.close()
    env.close()


def test_a_rebind_beyond_the_lds_plan_is_refused_and_moves_nothing():
    """A shape that fits member 1's extent (tests/test_ppo_mixed_cpu.py) and needs 171 008 bytes of LDS: RANENV_E_STATE naming the
    member, and weights, moments and counters of every member keep their bytes; the binding goes on working."""
    case = "edge"
    env = _mixed_env(case)
    rec, order = _record(env, case), _order(env, case, 1)
    env.ppo_update(rec, epochs=1, minibatch=mx.MINIBATCH, lr=1e-3, order=order)
    before = ref.state(env, G3)
    shape = env.population_net("inter", 1)
    wide = ref.make_inter_net(mx.S, mx.BEYOND[0], mx.BEYOND[1], 99)
    code, text = ref.refusal(lambda: env.set_population_member(1, inter=wide))
    assert code == E_STATE and "member 1" in text and "LDS" in text and "171008" in text, text
    ref.same_state(before, ref.state(env, G3), "a refused re-bind")
    assert env.population_net("inter", 1) == shape
    env.ppo_update(rec, epochs=1, minibatch=mx.MINIBATCH, lr=1e-3, order=order)
    assert ref.state(env, [1])["inter/1/w0"].tobytes() != before["inter/1/w0"].tobytes()
    env.close()


def test_the_next_collect_acts_on_every_members_trained_net():
    """collect(8) with a (gamma, lambda) pair per member -> ppo_update -> net_weights per member; a second, deterministic collect
    records what the float64 checks of tests/collect_ref.py accept for the exported nets, member by member; a member with epochs = 0
    keeps every byte, the others' weights moved."""
    case = "base"
    env = _mixed_env(case, stochastic=False)
    rec = env.collect(mx.T, gamma=[0.99, 0.9, 0.95], lam=[0.95, 0.9, 1.0])
    torch.cuda.synchronize()
    before = ref.state(env, G3)
    epochs = np.array([2, 0, 1])
    env.ppo_update(rec, epochs=epochs, minibatch=mx.MINIBATCH, lr=3e-3, seed=5)
    after = ref.state(env, G3)
    for m in range(G3):
        moved = [k for k in before if f"/{m}/" in k and before[k].tobytes() != after[k].tobytes()]
        if epochs[m] == 0:
            assert not moved, moved
        else:
            assert all(any(k.startswith(f"{r}/{m}/w") for k in moved) for r in ref.ROLES), (m, moved)
    v = env.views()
    episode, step0 = v["episode_number"].cpu().numpy().copy(), v["step_number"].cpu().numpy().copy()
    rec2 = to_host(env.collect(3))
    for m, sl in enumerate(env.population_slices()):
        seq = {r: ref.as_sequential([(w.cpu(), b.cpu()) for w, b in env.net_weights(r, m)], env.net_activation(r, m)) for r in ref.ROLES}
        mine = {k: x[:, sl] for k, x in rec2.items()}
        for t in range(3):
            r, _ = cr.check_actor_record(mine, t, seq["inter"], seq["intra"], False, ref.SEED, episode[sl], step0[sl] + t, mx.layout(case))
            r["vf"] = cr.check_values(mine["vf"][t], mine["obs_inter"][t], mine["obs_intra"][t], mine["mask_intra"][t], seq["v_inter"], seq["v_intra"], mx.layout(case))
            print(f"member {m} slot {t}: worst error / bound after the update: {r}")
    env.close()


def test_refusals_of_the_mixed_binding():
    """Plain ppo_bind on a mixed population; ppo_bind(mixed=True) on a uniform population and on a plain handle; a member beyond the LDS
    plan, named; bf16 members; intra nets per slice: RANENV_E_STATE each."""
    case = "base"
    env = ref.native_workload(mx.FIRST[-1])
    nets = mx.mixed_nets(case)
    one = {r: nets[r][0] for r in ref.ROLES}
    # a plain handle, and intra nets per slice
    env.set_policy_network(one["inter"], one["intra"], stochastic=True, seed=1, intra_input=mx.layout(case))
    env.set_value_network(one["v_inter"], one["v_intra"])
    code, text = ref.refusal(lambda: env.ppo_bind(mixed=True))
    assert code == E_STATE and "mixed" in text
    env.set_policy_network(one["inter"], [one["intra"]] * env.S, stochastic=True, seed=1, intra_input=mx.layout(case))
    code, text = ref.refusal(lambda: env.ppo_bind(mixed=True))
    assert code == E_STATE and "per slice" in text
    env.set_policy_network(one["inter"], one["intra"], stochastic=True, seed=1, intra_input=mx.layout(case))
    # a uniform population
    env.set_population(mx.FIRST)
    _bind(env, mx.twin_nets(case, 1), case, False)
    assert ref.refusal(lambda: env.ppo_bind(mixed=True))[0] == E_STATE
    env.ppo_bind()
    # the mixed population: the plain entry refuses, and an update under the uniform binding of a moment ago does too
    _bind(env, nets, case, True)
    code, text = ref.refusal(env.ppo_bind)
    assert code == E_STATE and "mixed" in text and "ranenv_ppo_bind_mixed" in text
    rec = _record(env, case)
    assert ref.refusal(lambda: env.ppo_update(rec, epochs=1, order=_order(env, case, 1)))[0] == E_STATE
    # a member beyond the plan
    wide = ref.make_role_nets(mx.S, mx.US, [512, 512, 512], "tanh", mx.layout(case), 77)
    big = {r: nets[r][:2] + [wide[r]] for r in ref.ROLES}
    _bind(env, big, case, True)
    code, text = ref.refusal(lambda: env.ppo_bind(mixed=True))
    assert code == E_STATE and "member 2" in text and "LDS" in text, text
    # bf16 members
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=1, intra_input=mx.layout(case), mixed=True, precision="bf16")
    env.set_value_network(nets["v_inter"], nets["v_intra"], mixed=True)
    code, text = ref.refusal(lambda: env.ppo_bind(mixed=True))
    assert code == E_STATE and "bf16" in text
    # ... and the case's own nets bind
    _bind(env, nets, case, True)
    env.ppo_bind(mixed=True)
    assert env.ppo_member_layout(2, "intra")["lds_bytes"] <= ref.LDS_MAX
    env.close()


def test_sixty_four_members_of_one_env_each():
    """Shapes cycling through the base case's three; members 0, 31 and 63 against their uniform twins, bit for bit"""
    case, G = "base", 64
    first = list(range(G + 1))
    env = _mixed_env(case, first, G)
    order = _order(env, case, 2, first, G)
    hp = dict(epochs=2, minibatch=5, lr=np.linspace(3e-4, 3e-3, G), grad_clip=0.5, order=order, grad=True)
    out = env.ppo_update(_record(env, case, first, G), **hp)
    assert np.all(out["minibatches"][:, 0, :] == 2) and np.all(out["rows"][:, 0, :] == mx.T)
    for m in (0, 31, 63):
        twin = _twin_env(case, m, first, G)
        out_t = twin.ppo_update(_record(twin, case, first, G), **hp)
        _same_member(env, out, twin, out_t, m, f"64 members, member {m}")
        twin.close()
    env.close()
