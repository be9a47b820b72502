"""The row lists on the device (ranenv_ppo_row_count / ranenv_ppo_row_order; the kernels of ranenv_rows.hip: count, scan, compact,
shuffle) against the numpy twin ``adapters.ppo_row_order_reference``, byte for byte, on the cases of tests/ppo_row_order_ref.py --
tests/test_ppo_row_order_cpu.py holds the twin to the plain restatement and shows that each planted slip fails this comparison on
these cases.  The handle is the native workload of tests/test_gpu_ppo_spread.py (B 12, S 5 / Us 5); the entries read nothing but
the mask, so most cases pass synthetic ``mask_inter`` tensors and need no rollout.  The compaction's chunk is
``ppo_row_order_ref.CHUNK`` = 2048 cells of one unit: that module's docstring says which lengths stand at its boundaries.

Then the refusals, and end to end on a real ``collect(8)`` record: ``order="device"`` under the plain, the spread, the per-slice
and the head binding leaves the state a twin handle reaches on the twin's lists."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import ppo_bindings_shapes_ref as bs
from tests import ppo_head_ref as hd
from tests import ppo_row_order_ref as rr
from tests import ppo_spread_ref as sp
from tests import ppo_update_ref as ref
from tests.gpu_common import need_gpu, shaped_workload

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -3
B, S = rr.B, rr.S
HP = dict(lr=2e-3, clip=0.2, vf_coeff=0.5, ent_coeff=0.01, grad_clip=0.5)


@pytest.fixture(scope="module")
def env():
    need_gpu()
    from intent_radio_sched_multi_slice_amd.adapters import ppo_row_order_reference      # noqa: F401  (fails here without the feature)
    e = ref.native_workload(B)
    assert (e.B, e.S) == (B, S)
    yield e
    e.close()


def _twin(mask, first, epochs, seed, **kw):
    from intent_radio_sched_multi_slice_amd.adapters import ppo_row_order_reference
    return ppo_row_order_reference(mask, first, epochs, seed, **kw)


def _rec(env, mask):
    return {"mask_inter": torch.from_numpy(mask).to(env.device)}


def _populate(env, pop):
    env.set_population(None if pop == "one" else rr.POPULATIONS[pop])


@pytest.mark.parametrize("case", rr.cases(), ids=lambda c: c[0])
def test_device_lists_equal_the_twins_byte_for_byte(env, case):
    """Tables equal, lists byte for byte; the same call a second time gives the same bytes"""
    name, T, kind, pop, per_slice, epochs, seed = case
    _populate(env, pop)
    mask = rr.make_mask(kind, T)
    got = env.ppo_row_order(_rec(env, mask), epochs, seed, per_slice=per_slice)
    want = _twin(mask, rr.POPULATIONS[pop], epochs, seed, per_slice=per_slice)
    assert rr.same(got, want) is None, (name, rr.same(got, want))
    if kind == "zeros":
        assert got["order_intra"].shape == (epochs, 0) and not got["first_intra"].any()
    if kind == "last_cell":
        assert got["order_intra"].cpu().tolist() == [[T * B * S - 1]] * epochs
    if kind == "dead_slice" and per_slice:
        assert got["first_intra"][2] == got["first_intra"][3] and got["first_intra"][1] == T * B
    again = env.ppo_row_order(_rec(env, mask), epochs, seed, per_slice=per_slice)
    assert rr.same(again, want) is None, name
    _populate(env, "one")


def test_inter_only_and_the_head_list(env):
    """No mask: the inter kind alone, for a record that has none; the head list is the one-member inter list; the seed's high word
    matters"""
    _populate(env, "three")
    for T in (1, 8):
        rec = {"logp": torch.zeros((T, B, S + 1), device=env.device)}
        for seed in rr.SEEDS:
            got = env.ppo_row_order(rec, 3, seed, intra=False)
            assert got["order_intra"] is None and got["first_intra"] is None
            assert rr.same(got, _twin((T, B, S), rr.POPULATIONS["three"], 3, seed, intra=False)) is None
    with pytest.raises(Exception):
        env.ppo_head_row_order(rec, 1)
    _populate(env, "one")
    rec = {"logp": torch.zeros((8, B), device=env.device)}
    lists = {seed: env.ppo_head_row_order(rec, 3, seed) for seed in rr.SEEDS + (5,)}
    for seed, o in lists.items():
        want = _twin((8, B, S), [0, B], 3, seed, intra=False)["order_inter"]
        assert o.dtype == torch.int32 and o.cpu().numpy().tobytes() == want.tobytes()
        assert torch.equal(o, env.ppo_row_order(_rec(env, rr.make_mask("bernoulli", 8)), 3, seed)["order_inter"])
    assert not torch.equal(lists[5], lists[2 ** 33 + 5])


def test_a_members_cells_beyond_one_chunk():
    """A wider batch: members of 2045, 2050 and 50 cells per TTI -- three cells short of a chunk, two past it, and a small one --
    under the members' grouping, and runs of 2487 rows under the slices'"""
    need_gpu()
    big = rr.BIG
    e = shaped_workload(big["S"], 5, big["B"], seed=71).env
    mask = rr.make_mask("bernoulli", big["T"], big["B"], big["S"], seed=3)
    mask[1, 408, :] = 1
    mask[1, 409, :] = 1
    for first, per_slice in ((big["first_env"], False), ([0, big["B"]], False), ([0, big["B"]], True)):
        e.set_population(first if len(first) > 2 else None)
        got = e.ppo_row_order(_rec(e, mask), 2, 11, per_slice=per_slice)
        assert rr.same(got, _twin(mask, first, 2, 11, per_slice=per_slice)) is None, (first, per_slice)
    e.close()


def test_refusals_change_nothing(env):
    """ranenv_ppo_row_order without a matching count, the slices' grouping on a population, sizes out of range: refused with the
    documented code, and the caller's buffers keep their bytes"""
    lib, h = env._lib, env._h
    T, epochs = 8, 2
    mask = torch.from_numpy(rr.make_mask("bernoulli", T)).to(env.device)
    other = mask.clone()
    fi, fa = (C.c_int32 * 65)(*([-7] * 65)), (C.c_int32 * 65)(*([-7] * 65))
    inter = torch.full((epochs, T * B), -7, dtype=torch.int32, device=env.device)
    intra = torch.full((epochs, T * B * S), -7, dtype=torch.int32, device=env.device)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    stream = env._stream()

    def untouched():
        torch.cuda.synchronize()
        return bool((inter == -7).all()) and bool((intra == -7).all()) and list(fi) == [-7] * 65 and list(fa) == [-7] * 65

    _populate(env, "one")
    fresh = ref.native_workload(B)               # a handle that has counted nothing
    assert fresh._lib.ranenv_ppo_row_order(fresh._h, T, p(mask), 0, epochs, 0, p(inter), p(intra), stream) == E_STATE
    fresh.close()
    assert untouched()
    assert lib.ranenv_ppo_row_count(h, 0, p(mask), 0, fi, fa, stream) == E_INVALID
    assert lib.ranenv_ppo_row_count(h, T, p(mask), 2, fi, fa, stream) == E_INVALID
    assert lib.ranenv_ppo_row_count(h, 2 ** 31 // (B * S) + 1, p(mask), 0, fi, fa, stream) == E_INVALID
    _populate(env, "three")
    assert lib.ranenv_ppo_row_count(h, T, p(mask), 1, fi, fa, stream) == E_INVALID
    assert lib.ranenv_ppo_row_order(h, T, p(mask), 1, epochs, 0, p(inter), p(intra), stream) == E_INVALID
    _populate(env, "one")
    assert untouched()
    # a count, then orders that do not match it
    f2, f3 = (C.c_int32 * 65)(), (C.c_int32 * 65)()
    assert lib.ranenv_ppo_row_count(h, T, p(mask), 0, f2, f3, stream) == 0
    assert lib.ranenv_ppo_row_order(h, T - 1, p(mask), 0, epochs, 0, p(inter), p(intra), stream) == E_STATE
    assert lib.ranenv_ppo_row_order(h, T, p(other), 0, epochs, 0, p(inter), p(intra), stream) == E_STATE
    assert lib.ranenv_ppo_row_order(h, T, p(mask), 1, epochs, 0, p(inter), p(intra), stream) == E_STATE
    assert lib.ranenv_ppo_row_order(h, T, p(mask), 0, 0, 0, p(inter), p(intra), stream) == E_INVALID
    _populate(env, "three")
    assert lib.ranenv_ppo_row_order(h, T, p(mask), 0, epochs, 0, p(inter), p(intra), stream) == E_STATE
    _populate(env, "one")
    assert untouched()
    assert lib.ranenv_ppo_row_count(h, T, None, 0, f2, None, stream) == 0
    assert lib.ranenv_ppo_row_order(h, T, None, 0, epochs, 0, p(inter), p(intra), stream) == E_STATE
    assert untouched()
    # ... and the one that does
    assert lib.ranenv_ppo_row_count(h, T, p(mask), 0, f2, f3, stream) == 0
    assert lib.ranenv_ppo_row_order(h, T, p(mask), 0, epochs, 0, p(inter), p(intra), stream) == 0
    torch.cuda.synchronize()
    want = _twin(mask, [0, B], epochs, 0)
    n = int(want["first_intra"][1])
    assert list(f2[:2]) == [0, T * B] and list(f3[:2]) == [0, n]
    assert inter.cpu().numpy().tobytes() == want["order_inter"].tobytes()
    flat = intra.reshape(-1).cpu().numpy()
    assert flat[:epochs * n].tobytes() == want["order_intra"].tobytes() and (flat[epochs * n:] == -7).all()
    with pytest.raises(ValueError):
        env.ppo_update({}, order="torch")


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _agent(case="relu24", **bind):
    env = ref.native_workload(B)
    nets, layout = sp.one_agent_nets(case), ref.CASES[case][2]
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=ref.SEED, intra_input=layout)
    env.set_value_network(nets["v_inter"], nets["v_intra"])
    env.ppo_bind(**bind)
    env.reset()
    return env


def _same_out(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        if name == "grad":
            assert torch.equal(a[name], b[name]) and bool(a[name].any()), f"{what}: dev_grad"
        else:
            assert np.asarray(a[name]).tobytes() == np.asarray(b[name]).tobytes(), f"{what}: statistics {name}"


def _as_tensors(twin, env):
    return {k: (torch.from_numpy(v).to(env.device) if k.startswith("order_") and v is not None else v) for k, v in twin.items()}


@pytest.mark.parametrize("bind", [{}, dict(spread=True, slabs=3)], ids=["plain", "spread3"])
def test_update_on_device_lists_equals_update_on_the_twins_lists(bind):
    """ppo_update(rec, order="device", seed=s) on a real collect(8) record leaves weights, moments, counters, statistics and dev_grad
    byte-equal to ppo_update(rec, order=<the twin's lists>) on a twin handle; the next collect() runs"""
    seed = 2 ** 33 + 5
    env_a, env_b = _agent(**bind), _agent(**bind)
    rec_a, rec_b = env_a.collect(8), env_b.collect(8)
    torch.cuda.synchronize()
    for k in rec_a:
        assert torch.equal(rec_a[k], rec_b[k]), k
    lists = _as_tensors(_twin(rec_b["mask_inter"], [0, B], 2, seed), env_b)
    assert 130 < int(lists["first_intra"][1]) < 8 * B * S
    out_a = env_a.ppo_update(rec_a, epochs=2, minibatch=ref.MINIBATCH, order="device", seed=seed, grad=True, **HP)
    out_b = env_b.ppo_update(rec_b, epochs=2, minibatch=ref.MINIBATCH, order=lists, grad=True, **HP)
    _same_out(out_a, out_b, str(bind))
    ref.same_state(ref.state(env_a, 1), ref.state(env_b, 1), str(bind))
    assert int(env_a.ppo_state("inter")["t"].cpu()[0]) == 2 * 8
    nxt_a, nxt_b = env_a.collect(8), env_b.collect(8)
    torch.cuda.synchronize()
    assert torch.equal(nxt_a["action_inter"], nxt_b["action_inter"]) and bool(torch.isfinite(nxt_a["logp"]).all())
    env_a.close()
    env_b.close()


def test_per_slice_update_on_device_lists():
    """The same for ppo_update_per_slice, whose intra lists are grouped by slice"""
    seed, case = 7, "relu24"

    def make():
        env = shaped_workload(3, 4, 6, seed=71).env
        widths, act, layout = ref.CASES[case]
        per = [ref.make_role_nets(3, 4, widths, act, layout, 4100 + 10 * s) for s in range(3)]
        env.set_policy_network(per[0]["inter"], [p["intra"] for p in per], stochastic=True, seed=ref.SEED, intra_input=layout)
        env.set_value_network(per[0]["v_inter"], [p["v_intra"] for p in per])
        env.ppo_bind(per_slice=True)
        env.reset()
        return env
    need_gpu()
    env_a, env_b = make(), make()
    rec_a, rec_b = env_a.collect(8), env_b.collect(8)
    torch.cuda.synchronize()
    for k in rec_a:
        assert torch.equal(rec_a[k], rec_b[k]), k
    lists = _as_tensors(_twin(rec_b["mask_inter"], [0, 6], 2, seed, per_slice=True), env_b)
    assert len(lists["first_intra"]) == 4 and int(lists["first_intra"][-1]) > 12
    out_a = env_a.ppo_update_per_slice(rec_a, epochs=2, minibatch=12, order="device", seed=seed, grad=True, **HP)
    out_b = env_b.ppo_update_per_slice(rec_b, epochs=2, minibatch=12, order=lists, grad=True, **HP)
    _same_out(out_a, out_b, "per slice")
    for s in (None, 0, 1, 2):
        ref.same_state(bs.slice_state(env_a, s), bs.slice_state(env_b, s), f"per slice, slice {s}")
    env_a.collect(8)
    torch.cuda.synchronize()
    env_a.close()
    env_b.close()


def test_head_update_on_device_lists():
    """... and for ppo_update_head with ppo_head_row_order's list"""
    need_gpu()
    seed, case = 2 ** 33 + 5, "base"
    (env_a, _), (env_b, _) = hd.make_env(case), hd.make_env(case)
    rec_a, rec_b = hd.with_noise(hd.collect(env_a, case)), hd.with_noise(hd.collect(env_b, case))
    for k in rec_a:
        assert torch.equal(rec_a[k], rec_b[k]), k
    T = int(rec_b["logp"].shape[0])
    want = torch.from_numpy(_twin((T, hd.B, env_b.S), [0, hd.B], 2, seed, intra=False)["order_inter"]).to(env_b.device)
    assert torch.equal(env_a.ppo_head_row_order(rec_a, 2, seed), want)
    hp = dict(epochs=2, minibatch=hd.MINIBATCH, lr=3e-4, grad_clip=0.5, clip=0.2, vf_coeff=0.5, ent_coeff=0.01, grad=True)
    out_a = env_a.ppo_update_head(rec_a, order="device", seed=seed, **hp)
    out_b = env_b.ppo_update_head(rec_b, order=want, **hp)
    _same_out(out_a, out_b, "head")
    ref.same_state(hd.head_state(env_a), hd.head_state(env_b), "head")
    env_a.collect_head(8)
    torch.cuda.synchronize()
    env_a.close()
    env_b.close()
