"""One handle passing through the PPO bindings of the IBSched nets in turn.  The handle keeps ONE record of its binding (plain, mixed,
wide, per slice) and every later call reads the geometry -- units, workgroups, counter and parked-row numbering -- from it, so what a
switch puts at risk is state of the binding just left surviving into the next: counters numbered [1 + S] read as [members][2], a
parked-rows share cut for another workgroup count, moments of the former nets.  Each walk trains one minibatch under the first binding,
switches, trains one under the second and holds weights, moments, counters, statistics and last gradient, byte for byte, against a
fresh handle given the same nets and the second binding alone; after a switch between the member and the per-slice geometry the
update call of the binding just left is RANENV_E_STATE and moves no byte.  Every refused call here is an ordinary error return.

Shapes, nets and row lists are tests/test_gpu_ppo_per_slice.py's (B 6, T 8, S 3, Us 4, case tanh40x24, explicit shares of 20 / 40 /
all live rows), the record collected once."""
from __future__ import annotations

import pytest
import torch

from tests import ppo_update_ref as ref
from tests.test_gpu_ppo_per_slice import E_STATE, HP, S, STAT_NAMES, T, _nets, _order, _plain_state, _share, _slice_state, _workload

pytestmark = pytest.mark.gpu

CASE = "tanh40x24"
ACT, LAYOUT = ref.CASES[CASE][1], ref.CASES[CASE][2]
_SHARED = {}


def _setup():
    """(the nets as (W, b) layers: "inter" / "v_inter" one net, "intra" / "v_intra" S, the record, its row lists), computed once"""
    if not _SHARED:
        nets = _nets(CASE)
        layers = {"inter": ref.layers_of(nets["inter"]), "v_inter": ref.layers_of(nets["v_inter"]),
                  "intra": [ref.layers_of(n) for n in nets["intra"]], "v_intra": [ref.layers_of(n) for n in nets["v_intra"]]}
        env = _handle(layers, per_slice=True)
        rec = env.collect(T)
        torch.cuda.synchronize()
        _SHARED.update(nets=layers, rec=rec, order=_order(rec, 1)[0])
        env.close()
    return _SHARED["nets"], _SHARED["rec"], _SHARED["order"]


def _set_nets(env, nets):
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=ref.SEED, intra_input=LAYOUT, activation=ACT)
    env.set_value_network(nets["v_inter"], nets["v_intra"], activation=ACT)


def _handle(nets, **bind):
    """A fresh, reset handle under ``nets`` with ``ppo_bind(**bind)`` alone"""
    env = _workload()
    _set_nets(env, nets)
    env.ppo_bind(**bind)
    env.reset()
    return env


def _shared_pair(nets, s, inter=None):
    """Slice s's intra pair as the one shared pair, beside the inter pair of ``nets`` or the one given"""
    return {"inter": (inter or nets)["inter"], "v_inter": (inter or nets)["v_inter"], "intra": nets["intra"][s], "v_intra": nets["v_intra"][s]}


def _inter_now(env):
    return {"inter": env.net_weights("inter"), "v_inter": env.net_weights("v_inter")}


def _train(env, per_slice, s=0):
    """One minibatch per policy on the shared record: the per-slice call, or the plain one on the inter rows and slice s's share"""
    _, rec, order = _setup()
    if per_slice:
        return env.ppo_update_per_slice(rec, epochs=1, minibatch=ref.ALL, order=order, grad=True, **HP)
    return env.ppo_update(rec, epochs=1, minibatch=ref.ALL, order=_share(order, s), grad=True, **HP)


def _state(env, per_slice):
    """Every trainable byte with its moments and counters, on the host"""
    if not per_slice:
        return {**_plain_state(env, 0), **_plain_state(env, 1)}
    out = dict(_slice_state(env, None))
    for s in range(S):
        out.update({f"slice{s}/{k}": v for k, v in _slice_state(env, s).items()})
    return out


def _same(env, out, fresh, out_fresh, per_slice, what):
    ref.same_state(_state(env, per_slice), _state(fresh, per_slice), what)
    for n in STAT_NAMES:
        assert out[n].tobytes() == out_fresh[n].tobytes(), f"{what}: {n}"
    assert out["grad"].cpu().numpy().tobytes() == out_fresh["grad"].cpu().numpy().tobytes(), f"{what}: last gradient"
    assert out["minibatches"].max() == 1 and out["rows"].min() > 0, f"{what}: one minibatch of every policy"


def _refused_and_kept(env, call, per_slice, what):
    before = _state(env, per_slice)
    code, text = ref.refusal(call)
    assert code == E_STATE and len(text) > 20, (what, code, text)
    ref.same_state(_state(env, per_slice), before, what)
    return text


def test_per_slice_wide_then_plain():
    nets, rec, order = _setup()
    env = _handle(nets, per_slice=True, wide=True)
    _train(env, True)
    assert all(int(env.ppo_state("intra", slice=s)["t"][0]) == 1 for s in range(S)) and int(env.ppo_state("inter", slice=0)["t"][0]) == 1
    second = _shared_pair(nets, 1, inter=_inter_now(env))
    _set_nets(env, second)
    env.ppo_bind()
    text = _refused_and_kept(env, lambda: env.ppo_update_per_slice(rec, epochs=1, order=order), False, "the per-slice update after the switch to plain")
    assert "per-slice" in text
    out = _train(env, False, s=1)
    fresh = _handle(second)
    _same(env, out, fresh, _train(fresh, False, s=1), False, "per slice + wide, then plain")
    assert int(env.ppo_state("intra")["t"][0]) == 1 and int(env.ppo_state("inter")["t"][0]) == 1
    env.close()
    fresh.close()


def test_plain_then_per_slice():
    nets, rec, order = _setup()
    env = _handle(_shared_pair(nets, 1))
    _train(env, False, s=1)
    second = {**nets, **_inter_now(env)}
    _set_nets(env, second)
    env.ppo_bind(per_slice=True)
    text = _refused_and_kept(env, lambda: env.ppo_update(rec, epochs=1, order=_share(order, 1)), True, "the plain update after the switch to per slice")
    assert "per slice" in text
    out = _train(env, True)
    fresh = _handle(second, per_slice=True)
    _same(env, out, fresh, _train(fresh, True), True, "plain, then per slice")
    assert all(int(env.ppo_state("intra", slice=s)["t"][0]) == 1 for s in range(S))
    env.close()
    fresh.close()


def test_plain_wide_plain_and_wide_again_on_the_kept_parked_rows():
    """plain -> wide -> plain -> wide on one handle: the second wide bind finds the parked rows of the first allocated and reuses them.
    (Both bindings train through ``ppo_update``: there is no call of the binding just left to refuse.)"""
    nets, _, _ = _setup()
    env = _handle(_shared_pair(nets, 0))
    _train(env, False)
    for step, bind in enumerate(({"wide": True}, {}, {"wide": True})):
        now = {**_inter_now(env), "intra": env.net_weights("intra"), "v_intra": env.net_weights("v_intra")}
        env.ppo_bind(**bind)
        out = _train(env, False)
        fresh = _handle(now, **bind)
        _same(env, out, fresh, _train(fresh, False), False, f"step {step}: ppo_bind({bind})")
        fresh.close()
    env.close()
