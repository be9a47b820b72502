"""The PPO update of non-shared intra policies on the device (ranenv_ppo_bind_slices / ranenv_ppo_update_slices, the kernels
ranenv_ppo_update_kernel_slices and _slices_wide): one launch of 1 + S workgroups, slice s's actor / critic pair trained on slice s's
rows alone.  Held bit for bit against the existing kernel -- a handle bound to ONE shared intra pair (slice s's nets) under the plain
``ppo_bind()`` and given slice s's share of the row list --, against the float64 twin ``adapters.ppo_update_reference`` through the
comparisons of tests/ppo_update_ref.py at its tolerances, and in its mapping, its empty slices, its wide twin, the next collect(), the
re-binding rules and the refusals.

The shape is the smallest with every hazard: B 6, T 8, S 3, Us 4, nets of ``ppo_update_ref.CASES`` (widths off the 32 grid, both intra
input layouts), S DISTINCT nets per slice, minibatch 12.  The row lists are explicit: one slice keeps 20 rows (a partial tile; 12 + 8),
the slice with the most live rows keeps 40 (a tile and a quarter; 12 + 12 + 12 + 4), the third keeps all its live rows -- or, in the
empty-slice case, none."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import ppo_bindings_shapes_ref as bs
from tests import ppo_update_ref as ref
from tests.gpu_common import need_gpu, shaped_workload, to_host

pytestmark = pytest.mark.gpu

E_STATE = -3
S, US, B, T, MB = 3, 4, 6, 8, 12
SMALL, BIG = 20, 40
ALL = ref.ALL
HP = dict(lr=2e-3, clip=0.2, vf_coeff=0.5, ent_coeff=0.01, grad_clip=0.5)
STAT_NAMES = bs.STAT_NAMES


def _nets(case, seed=4100):
    """The inter pair and S distinct intra pairs of the case's shape: {"inter", "v_inter": net, "intra", "v_intra": [S nets]}"""
    widths, act, layout = ref.CASES[case]
    per = [ref.make_role_nets(S, US, widths, act, layout, seed + 10 * s) for s in range(S)]
    return {"inter": per[0]["inter"], "v_inter": per[0]["v_inter"], "intra": [p["intra"] for p in per], "v_intra": [p["v_intra"] for p in per]}


def _workload():
    need_gpu()
    return shaped_workload(S, US, B, seed=71).env


def _env(case, nets=None, **bind):
    """A reset env under the non-shared nets, bound with ``ppo_bind(per_slice=True, **bind)``"""
    env, nets = _workload(), _nets(case) if nets is None else nets
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=ref.SEED, intra_input=ref.CASES[case][2])
    env.set_value_network(nets["v_inter"], nets["v_intra"])
    env.ppo_bind(per_slice=True, **bind)
    env.reset()
    return env


def _shared_env(case, nets, s):
    """A reset env under ONE shared intra pair, slice s's nets, bound with the plain ``ppo_bind()``"""
    env = _workload()
    env.set_policy_network(nets["inter"], nets["intra"][s], stochastic=True, seed=ref.SEED, intra_input=ref.CASES[case][2])
    env.set_value_network(nets["v_inter"], nets["v_intra"][s])
    env.ppo_bind()
    env.reset()
    return env


def _order(rec, epochs, empty=None, seed=3):
    """Explicit row lists with the docstring's shares (bs.slice_order); returns (order, the slices' shares [S]).  Asserts the counts."""
    return bs.slice_order(rec, epochs, MB, SMALL, BIG, empty, seed)


_share, _host, _slice_state, _plain_state, _row = bs.share, bs.host, bs.slice_state, bs.plain_state, bs.wg_row


_RUNS = {}


def _run(case, empty=None, **bind):
    """2 epochs x minibatches of 12 on a stochastic record under the per-slice binding, computed once:
    (record on the device, order, shares, out, state per slice, the inter pair's state)"""
    key = (case, empty, tuple(sorted(bind.items())))
    if key not in _RUNS:
        env = _env(case, **bind)
        rec = env.collect(T)
        torch.cuda.synchronize()
        order, counts = _order(rec, 2, empty)
        start = [_slice_state(env, s) for s in range(S)]
        out = env.ppo_update_per_slice(rec, epochs=2, minibatch=MB, order=order, grad=True, **HP)
        _RUNS[key] = dict(rec=rec, order=order, counts=counts, out=out, start=start, slices=[_slice_state(env, s) for s in range(S)], inter=_slice_state(env, None))
        env.close()
    return _RUNS[key]


@pytest.mark.parametrize("case", list(ref.CASES))
def test_every_slice_bit_for_bit_against_the_plain_kernel_on_one_shared_pair(case):
    """Slice s's weights, moments, counter, statistics and last gradient equal, byte for byte, those of a handle bound to the shared pair
    (net s) under ``ppo_bind()`` and updated on the same record with an intra list of slice s's share; the inter pair equals that
    handle's inter pair."""
    run, nets = _run(case), _nets(case)
    assert run["counts"].count(SMALL) >= 1 and run["counts"].count(BIG) >= 1 and min(run["counts"]) > 0
    for s in range(S):
        shared = _shared_env(case, nets, s)
        o = shared.ppo_update(run["rec"], epochs=2, minibatch=MB, order=_share(run["order"], s), grad=True, **HP)
        ref.same_state(run["slices"][s], _plain_state(shared, 1), f"{case} slice {s}")
        stats, grad = _row(run["out"], 1 + s)
        assert stats.tobytes() == np.stack([o[n][0, 1] for n in STAT_NAMES], axis=-1).tobytes(), f"{case} slice {s}: statistics"
        assert grad.tobytes() == o["grad"][0, 1].cpu().numpy().tobytes(), f"{case} slice {s}: last gradient"
        assert int(run["slices"][s]["intra/t"][0]) == 2 * -(-run["counts"][s] // MB)
        if s == 0:
            ref.same_state(run["inter"], _plain_state(shared, 0), f"{case} inter pair")
            stats, grad = _row(run["out"], 0)
            assert stats.tobytes() == np.stack([o[n][0, 0] for n in STAT_NAMES], axis=-1).tobytes(), f"{case}: inter statistics"
            assert grad.tobytes() == o["grad"][0, 0].cpu().numpy().tobytes(), f"{case}: inter gradient"
        shared.close()
    assert all(run["slices"][s][k].tobytes() != run["start"][s][k].tobytes() for s in range(S) for k in ("intra/w0", "v_intra/w0")), "a slice did not train"


_SliceView = bs.SliceView


@pytest.mark.parametrize("case", list(ref.CASES))
def test_gradient_statistics_and_adam_step_of_every_slice_against_the_float64_twin(case):
    """ref.check_against_twin (gradient per layer tensor within 8x the float32-torch yardstick of the float64 twin, the statistics at
    1e-6) on an lr = 0 call of one minibatch per policy, the twin called per slice with kind "intra", slice s's nets and slice s's share;
    then ref.check_adam_step (weights and moments within 4 float32 ulp of the stated arithmetic on the device's own gradient) on the
    first real step from zero moments."""
    env = _env(case)
    rec = env.collect(T)
    torch.cuda.synchronize()
    order, counts = _order(rec, 1)
    act, layout = ref.CASES[case][1], ref.CASES[case][2]
    out = env.ppo_update_per_slice(rec, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, order=order, grad=True)
    views = [_SliceView(env, s) for s in range(S)]
    w0 = [v.weights() for v in views]
    misses = []
    for s, v in enumerate(views):
        worst, miss = ref.check_against_twin(rec, _share(order, s), v.out(out), w0[s], [0], f"{case} slice {s}", act, act, layout)
        assert 0.0 < worst <= 8.0
        misses += miss
        assert out["rows"][1 + s, 0] == counts[s]
    assert not misses, misses
    hp = dict(lr=[1e-3], grad_clip=[0.5], betas=(0.9, 0.999), eps=1e-8)
    env.ppo_bind(per_slice=True)           # (the lr = 0 call moved moments and counters: the later bind replaces the earlier one and zeroes them)
    out = env.ppo_update_per_slice(rec, epochs=1, minibatch=ALL, lr=1e-3, grad_clip=0.5, order=order, grad=True)
    for s, v in enumerate(views):
        ref.check_adam_step(v, v.out(out), w0[s], v.weights(), hp, 1, f"{case} slice {s}")
    env.close()


def test_the_probe_returns_the_records_own_log_probabilities_for_every_live_cell():
    """lr = 0, one epoch, all live rows, probe_logp: every live cell's re-evaluated logp is the recorded one -- intra cells to the bit,
    inter cells within 1 float32 ulp, the probe tolerance of tests/test_gpu_ppo_update.py.  The S nets are distinct: a slice -> net shift
    would re-evaluate slice s's rows with another net."""
    from tests.gpu_common import _ordered
    case = "tanh40x24"
    env = _env(case)
    rec = env.collect(T)
    out = env.ppo_update_per_slice(rec, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, seed=9, probe_logp=True)
    new, old, mask = out["logp"].cpu().numpy(), rec["logp"].cpu().numpy(), rec["mask_inter"].cpu().numpy() != 0
    assert mask.any(axis=(0, 1)).all(), "a slice without a live cell"
    assert np.array_equal(new[..., 1:][mask].view(np.int32), old[..., 1:][mask].view(np.int32)), "intra logp is not re-evaluated to the bit"
    assert np.abs(_ordered(new[..., 0]) - _ordered(old[..., 0])).max() <= 1
    assert np.array_equal(out["rows"][1:, 0], mask.sum(axis=(0, 1)))
    # (the shift made visible: slice 0's rows under slice 1's net do not give the recorded logp)
    shifted = _shared_env(case, _nets(case), 1)
    o = shifted.ppo_update(rec, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, seed=9, probe_logp=True)
    other = o["logp"].cpu().numpy()
    assert not np.array_equal(other[..., 1][mask[..., 0]].view(np.int32), old[..., 1][mask[..., 0]].view(np.int32))
    env.close()
    shifted.close()


@pytest.mark.parametrize("empty", [0, 1, 2])
def test_an_empty_slice_keeps_its_bytes_and_leaves_the_others_alone(empty):
    """A slice whose share is empty: weights, moments and counter keep their bytes, its statistics rows are zero; the other slices and
    the inter pair equal, byte for byte, the run with that slice present."""
    case = "tanh40x24"
    full, run = _run(case), _run(case, empty=empty)
    assert run["counts"][empty] == 0 and [c for s, c in enumerate(run["counts"]) if s != empty] == [c for s, c in enumerate(full["counts"]) if s != empty]
    ref.same_state(run["slices"][empty], run["start"][empty], f"empty slice {empty}")
    assert int(run["slices"][empty]["intra/t"][0]) == 0
    stats, grad = _row(run["out"], 1 + empty)
    assert not stats.any() and not grad.any()
    ref.same_state(run["inter"], full["inter"], "the inter pair beside an empty slice")
    for s in range(S):
        if s != empty:
            ref.same_state(run["slices"][s], full["slices"][s], f"slice {s} beside the empty slice {empty}")
            assert _row(run["out"], 1 + s)[0].tobytes() == _row(full["out"], 1 + s)[0].tobytes()


@pytest.mark.parametrize("case", list(ref.CASES))
def test_the_wide_binding_gives_the_plain_per_slice_bytes(case):
    plain, wide = _run(case), _run(case, wide=True)
    ref.same_state(plain["inter"], wide["inter"], f"{case} inter")
    for s in range(S):
        ref.same_state(plain["slices"][s], wide["slices"][s], f"{case} slice {s}")
    for wg in range(1 + S):
        a, b = _row(plain["out"], wg), _row(wide["out"], wg)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), f"{case} workgroup {wg}"


def test_the_next_collect_acts_on_the_trained_nets_and_a_fresh_handle_agrees():
    """After the update, with no rebind, collect() acts on the trained nets: a fresh handle bound to what ``net_weights(role, slice=s)``
    returns records the same actions, log-probabilities and values bit for bit; before the update ``net_weights`` returns the bound nets."""
    from intent_radio_sched_multi_slice_amd.batched_env import packed_net_floats
    case = "tanh40x24"
    act, layout = ref.CASES[case][1], ref.CASES[case][2]
    env, nets = _env(case), _nets(case)
    for s in range(S):
        for r in ("intra", "v_intra"):
            for (w, b), (w0, b0) in zip(env.net_weights(r, slice=s), ref.layers_of(nets[r][s])):
                assert torch.equal(w.cpu(), w0) and torch.equal(b.cpu(), b0), (r, s)
            assert env.net_activation(r, slice=s) == act
        lay = env.ppo_member_layout(s, "intra")          # (what unpacks row 1 + s of "grad")
        assert (lay["actor"], lay["critic"]) == tuple(packed_net_floats(ref.layers_of(nets[r][s])) for r in ("intra", "v_intra"))
    rec = env.collect(T)
    env.ppo_update_per_slice(rec, epochs=2, minibatch=MB, seed=5, **HP)
    trained = {"inter": env.net_weights("inter"), "v_inter": env.net_weights("v_inter"),
               "intra": [env.net_weights("intra", slice=s) for s in range(S)], "v_intra": [env.net_weights("v_intra", slice=s) for s in range(S)]}
    assert all(not torch.equal(trained["intra"][s][0][0].cpu(), ref.layers_of(nets["intra"][s])[0][0]) for s in range(S))
    fresh = _env(case)                     # (a second handle walks the same T TTIs under the same untrained nets ...)
    rec_f = fresh.collect(T)
    for k in rec:
        assert torch.equal(rec[k], rec_f[k]), k
    fresh.set_policy_network(trained["inter"], trained["intra"], stochastic=True, seed=ref.SEED, intra_input=layout, activation=act)
    fresh.set_value_network(trained["v_inter"], trained["v_intra"], activation=act)      # (... and is then bound to what was read back)
    a, b = to_host(env.collect(3)), to_host(fresh.collect(3))
    for k in a:
        assert torch.equal(torch.as_tensor(a[k]), torch.as_tensor(b[k])), k
    env.close()
    fresh.close()


def test_rebinding_and_refusals():
    """A rebind of the per-slice actors restarts the S counters and the moments of both nets of every slice and leaves the inter pair's;
    a shared intra critic beside per-slice actors, a population, bf16 nets and an update after leaving the per-slice form are
    RANENV_E_STATE with a text, and the weights keep their bytes across every refused call; ``ppo_bind()`` without ``per_slice``
    still refuses nets per slice."""
    case = "tanh40x24"
    act, layout = ref.CASES[case][1], ref.CASES[case][2]
    env, nets = _env(case), _nets(case)
    rec = env.collect(T)
    order, _ = _order(rec, 1)
    env.ppo_update_per_slice(rec, epochs=1, minibatch=MB, order=order, **HP)
    trained, inter = [_slice_state(env, s) for s in range(S)], _slice_state(env, None)
    assert all(int(x["intra/t"][0]) > 0 and x["intra/m"].any() and x["v_intra/v"].any() for x in trained) and int(inter["inter/t"][0]) > 0
    _, in_intra = env.net_input_dims(layout)
    from intent_radio_sched_multi_slice_amd.batched_env import NET_INPUTS
    env._set_net_list("intra_policy_nets", "ranenv_set_intra_policy_networks", env._net_list(nets["intra"], None, in_intra, 3, NET_INPUTS[layout]))
    after = [_slice_state(env, s) for s in range(S)]
    for s in range(S):
        for r in ("intra", "v_intra"):
            assert int(after[s][f"{r}/t"][0]) == 0 and not after[s][f"{r}/m"].any() and not after[s][f"{r}/v"].any(), (r, s)
        for k in trained[s]:
            if k.startswith("v_intra/") and k.split("/")[1][0] in "wb":
                assert after[s][k].tobytes() == trained[s][k].tobytes(), f"re-binding the actors moved the critics' {k}"
    ref.same_state(_slice_state(env, None), inter, "the inter pair across a rebind of the per-slice actors")

    def kept(fn, what):
        before = [_slice_state(env, s) for s in range(S)]
        code, text = ref.refusal(fn)
        assert code == E_STATE and len(text) > 20, (what, code, text)
        for s in range(S):
            ref.same_state(_slice_state(env, s), before[s], what)
        return text

    kept(env.ppo_bind, "ppo_bind() without per_slice")
    assert "per slice" in kept(lambda: env.ppo_update(rec, epochs=1, order=_share(order, 0)), "ppo_update under the per-slice binding")
    # a shared intra critic beside the per-slice actors
    env.set_value_network(nets["v_inter"], nets["v_intra"][0])
    assert "no one owner" in ref.refusal(lambda: env.ppo_bind(per_slice=True))[1]
    assert ref.refusal(lambda: env.ppo_update_per_slice(rec, epochs=1, order=order))[0] == E_STATE
    env.set_value_network(nets["v_inter"], nets["v_intra"])
    env.ppo_bind(per_slice=True)
    env.ppo_update_per_slice(rec, epochs=1, minibatch=MB, order=order, **HP)
    # leaving the per-slice form: one shared intra actor
    env.set_policy_network(nets["inter"], nets["intra"][0], stochastic=True, seed=ref.SEED, intra_input=layout)
    code, text = ref.refusal(lambda: env.ppo_update_per_slice(rec, epochs=1, order=order))
    assert code == E_STATE and "bind again" in text
    assert "no one owner" in ref.refusal(lambda: env.ppo_bind(per_slice=True))[1]
    env.close()
    # bf16 nets
    env = _workload()
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=ref.SEED, intra_input=layout, precision="bf16")
    env.set_value_network(nets["v_inter"], nets["v_intra"], precision="bf16")
    code, text = ref.refusal(lambda: env.ppo_bind(per_slice=True))
    assert code == E_STATE and "bf16" in text
    env.close()
    # a population
    env = _workload()
    env.set_population([0, 2, B])
    env.set_policy_network([nets["inter"]] * 2, [nets["intra"][0]] * 2, stochastic=True, seed=ref.SEED, intra_input=layout)
    env.set_value_network([nets["v_inter"]] * 2, [nets["v_intra"][0]] * 2)
    code, text = ref.refusal(lambda: env.ppo_bind(per_slice=True))
    assert code == E_STATE and "population" in text
    with pytest.raises(ValueError):
        env.ppo_bind(per_slice=True, mixed=True)
    env.close()
