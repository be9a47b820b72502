"""The bf16 spread PPO binding without a GPU (ranenv_ppo_bind_spread_bfloat / ranenv_ppo_spread_bfloat_bytes; include/ranenv.h "bf16 nets
over the chip"): the two new exports in the header, the ctypes table and the built library; the size function against the LDS rule and
the byte formula restated in tests/ppo_bf16_ref.py; the twin ``adapters.ppo_update_reference(..., precision="bf16")`` -- its forward
against ``_mlp_forward``, its gradient against a plain numpy restatement of contract steps 1-3, its acting copy behind Adam steps --;
the exact nets of family (a) with the conditions that make them exact; and, per gradient tensor of the random nets, the distance e_bf
between bf16 and f32 training with what each planted slip moves against the quarter of it that caps the GPU comparison."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from intent_radio_sched_multi_slice_amd import _lib
from intent_radio_sched_multi_slice_amd import adapters as ad
from intent_radio_sched_multi_slice_amd import batched_env as be
from tests import ppo_bf16_ref as bf
from tests import ppo_spread_ref as sp
from tests import ppo_update_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = {"ranenv_ppo_bind_spread_bfloat": 3, "ranenv_ppo_spread_bfloat_bytes": 5}
E_INVALID = -1
CASES = ["relu24", "tanh40x24"]


def test_header_binding_and_library_agree_on_the_new_exports():
    hdr = open(os.path.join(REPO, "include", "ranenv.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name, n_args in NEW_EXPORTS.items():
        proto = re.search(r"^int " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
        assert proto, f"{name} is not declared in include/ranenv.h"
        assert len(proto.group(1).split(",")) == n_args, name
        assert name in _lib.EXPORTS and len(_lib.FUNCTIONS[name][1]) == n_args and hasattr(lib, name), name
    assert re.search(r"^#define RANENV_ABI_VERSION 10\b", hdr, re.M), "added entries leave the ABI version at 10"


def test_the_size_function_against_the_restated_rule():
    """The SHAPES grid of tests/ppo_update_ref.py, [512] x 3 and [512] x 4: LDS and device bytes; the issue's three figures; what the
    function refuses, by code and message"""
    pairs = []
    for S, Us, layout, (aw, _), (cw, _) in ref.SHAPES.values():
        pairs += list(bf.kind_dims(S, Us, layout, aw, cw).values())
    pairs += list(bf.kind_dims(5, 5, "obs", [512] * 3, [512] * 3).values()) + list(bf.kind_dims(16, 16, "mask_obs", [512] * 4, [512] * 4).values())
    for actor, critic in pairs:
        for slabs in (1, 64, 256):
            got = be.ppo_spread_bf16_bytes(actor, critic, slabs)
            assert got == {"lds": bf.pair_lds_bytes(actor, critic), "device": bf.device_bytes(actor, critic, slabs)}, (actor, critic, slabs)
        assert be.ppo_spread_bf16_bytes(actor, None, 3) == {"lds": bf.pair_lds_bytes(actor), "device": bf.device_bytes(actor, None, 3)}
    verybig = ([50, 512, 512, 512, 10], [50, 512, 512, 512, 1])
    assert be.ppo_spread_bf16_bytes(*verybig)["lds"] == 119296 < bf.LDS_MAX < be.ppo_lds_bytes(*verybig)      # (the f32 rows need the wide plan)
    deep = ([160] + [512] * 4 + [32], [160] + [512] * 4 + [1])
    assert be.ppo_spread_bf16_bytes(*deep)["lds"] == 159232 <= bf.LDS_MAX
    n_in = ref.intra_width(100, "mask_obs")
    assert be.ppo_spread_bf16_bytes([n_in] + [512] * 4 + [3], [n_in] + [512] * 4 + [1])["lds"] > bf.LDS_MAX      # (beyond the plan by size)
    # ... but no handle has such an input: ranenv_create takes S <= 16 and Us <= 16, a net four hidden layers of at most 512, so the
    # largest pair a handle can bind is `deep` above (the intra input at Us 16 under mask_obs is 57 -> 64, narrower than 160): every
    # pair that can be bound fits the bf16 plan, and the bind's refusal by size is a guard no handle reaches today.
    assert max(bf.pair_lds_bytes(*pair) for pair in bf.kind_dims(16, 16, "mask_obs", [512] * 4, [512] * 4).values()) == 159232
    assert be.ppo_spread_bf16_bytes(*verybig, 64)["device"] - be.ppo_spread_bf16_bytes(*verybig, 1)["device"] == 63 * 4 * sum(sp.packed_floats(d) for d in verybig)
    lib, lds, dev = _lib.load(), C.c_int64(-7), C.c_int64(-7)
    actor = _lib.Mlp()
    actor.n_hidden, actor.dims[0], actor.dims[1], actor.dims[2] = 1, 50, 64, 10
    assert lib.ranenv_ppo_spread_bfloat_bytes(None, None, 4, C.byref(lds), C.byref(dev)) == E_INVALID and lds.value == dev.value == -7
    assert lib.ranenv_ppo_spread_bfloat_bytes(C.byref(actor), None, 4, None, None) == E_INVALID and b"null argument" in lib.ranenv_last_error(None)
    assert lib.ranenv_ppo_spread_bfloat_bytes(C.byref(actor), None, 0, C.byref(lds), None) == E_INVALID and b"slabs 0 (1..256)" in lib.ranenv_last_error(None)
    assert lib.ranenv_ppo_spread_bfloat_bytes(C.byref(actor), None, 257, None, C.byref(dev)) == E_INVALID and dev.value == -7
    actor.dims[1] = 513
    assert lib.ranenv_ppo_spread_bfloat_bytes(C.byref(actor), None, 4, C.byref(lds), None) == E_INVALID and b"hidden width 513" in lib.ranenv_last_error(None)
    actor.dims[1] = 64
    assert lib.ranenv_ppo_spread_bfloat_bytes(C.byref(actor), None, 4, C.byref(lds), None) == 0 and lds.value == bf.pair_lds_bytes([50, 64, 10])
    assert lib.ranenv_ppo_bind_spread_bfloat(None, 0, None) == E_INVALID and b"slabs 0 (1..256)" in lib.ranenv_last_error(None)
    assert lib.ranenv_ppo_bind_spread_bfloat(None, 64, None) == E_INVALID and b"null handle" in lib.ranenv_last_error(None)


def test_ppo_bind_bf16_needs_spread_and_excludes_the_other_bindings():
    env = object.__new__(be.BatchedRanEnv)      # (refused before the handle is touched: no GPU needed)
    with pytest.raises(ValueError) as e:
        env.ppo_bind(bf16=True)
    assert "bf16 needs spread" in str(e.value)
    for other in ("wide", "mixed", "per_slice", "head"):
        with pytest.raises(ValueError) as e:
            env.ppo_bind(spread=True, slabs=8, bf16=True, **{other: True})
        assert "bf16 and " + other in str(e.value)


# ---- the twin ---------------------------------------------------------------------------------------------------------------------------
def _case(case, seed=4100):
    """(the four nets of ONE agent as host (W, b) lists, activation, intra layout) of a ref.CASES shape"""
    nets = sp.one_agent_nets(case, seed)
    return {r: [(w.numpy(), b.numpy()) for w, b in ref.layers_of(nets[r])] for r in ref.ROLES}, ref.CASES[case][1], ref.CASES[case][2]


@pytest.mark.parametrize("case", CASES)
def test_the_twins_forward_is_the_acting_contracts_bit_for_bit(case):
    nets, act, _ = _case(case)
    x = torch.rand((70, nets["inter"][0][0].shape[1]), generator=torch.Generator().manual_seed(3))
    layers = ref.as_torch(nets["inter"])
    got = ad._mlp_forward_bf16_trained(x, layers, act)
    want = ad._mlp_forward(x, layers, act, precision="bf16")
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert not torch.equal(want, ad._mlp_forward(x, layers, act))          # (the rounding does change the outputs)


@pytest.mark.parametrize("case", CASES)
def test_the_twins_gradient_against_the_numpy_restatement(case):
    """Contract steps 1-3 in plain numpy against torch autograd through the twin's functions, float64, relative 1e-12 per tensor: with a
    random dL/d(output) on all four nets, and for the critic through ``ppo_update_reference`` itself, whose G is 2 vf (V - vtarg) / rows"""
    nets, act, layout = _case(case)
    rng = np.random.default_rng(11)
    for r in ref.ROLES:
        layers = [(torch.as_tensor(w, dtype=torch.float64).requires_grad_(True), torch.as_tensor(b, dtype=torch.float64).requires_grad_(True)) for w, b in nets[r]]
        x = rng.random((45, nets[r][0][0].shape[1])).astype(np.float32)
        G = rng.standard_normal((45, nets[r][-1][0].shape[0])) * 0.01
        out = ad._mlp_forward_bf16_trained(torch.as_tensor(x, dtype=torch.float64), layers, act)
        assert np.array_equal(out.detach().numpy(), bf.contract_forward(x, nets[r], act)[0])
        got = torch.autograd.grad((out * torch.as_tensor(G)).sum(), [p for wb in layers for p in wb])
        stats = {}
        want = bf.contract_backward(x, nets[r], act, G, stats=stats)
        assert stats["d_changed"] > 16 and stats["hidden_changed"] > 16
        for li, (gw, gb) in enumerate(want):
            assert bf.rel_l2(got[2 * li].numpy(), gw) <= 1e-12 and bf.rel_l2(got[2 * li + 1].numpy(), gb) <= 1e-12, (r, li)
    rec = ref.synthetic_record(B=12, seed=5, layout=layout)
    order = ad.ppo_row_order(rec, [0, 12], 1, 3)
    n = int(order["first_inter"][1])
    res = bf.twin_grads(rec, "inter", nets["inter"], nets["v_inter"], order["order_inter"], 0, n, act, layout)
    rows = ad.ppo_rows(rec, "inter", order["order_inter"][0, :n], layout)
    x, vtarg = rows["x"].numpy().astype(np.float32), rows["vtarg"].numpy()
    v = bf.contract_forward(x, nets["v_inter"], act)[0][:, 0]
    want = bf.contract_backward(x, nets["v_inter"], act, (2.0 * 0.5 * (v - vtarg) / n)[:, None])
    for (gw, gb), (ww, wb) in zip(res["grad"]["critic"], want):
        assert bf.rel_l2(gw.numpy(), ww) <= 1e-12 and bf.rel_l2(gb.numpy(), wb) <= 1e-12


def test_the_twins_acting_copy_is_bf16_of_its_masters_behind_every_step():
    """Three epochs of minibatches of 40 at lr 3e-3: the masters move off the bf16 grid, the acting copy is their rounding, and the
    default precision is today's path -- the same bytes with and without the new argument"""
    nets, act, layout = _case("tanh40x24")
    rec = ref.synthetic_record(B=12, seed=5, layout=layout)
    order = ad.ppo_row_order(rec, [0, 12], 3, 3)
    n = int(order["first_inter"][1])
    args = dict(rec=rec, kind="inter", actor=ref.as_torch(nets["inter"]), critic=ref.as_torch(nets["v_inter"]), order=order["order_inter"], lo=0, hi=n,
                epochs=3, minibatch=40, lr=3e-3, act_actor=act, act_critic=act, layout=layout)
    for dtype in (torch.float64, torch.float32):
        res = ad.ppo_update_reference(dtype=dtype, precision="bf16", **args)
        for net in ("actor", "critic"):
            for (w, b), (wq, bq) in zip(res[net], res["acting"][net]):
                assert w.dtype == dtype and torch.equal(wq, ad.bf16_round(w).to(dtype)) and torch.equal(bq, b)
                assert not torch.equal(wq, w)
    a, b = ad.ppo_update_reference(**args), ad.ppo_update_reference(precision="f32", **args)
    assert "acting" not in a and all(torch.equal(x, y) for net in ("actor", "critic") for p, q in zip(a[net], b[net]) for x, y in zip(p, q))
    assert np.array_equal(a["stats"], b["stats"])
    with pytest.raises(ValueError):
        ad.ppo_update_reference(precision="fp8", **args)


# ---- the exact nets ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", list(bf.EXACT_ARCHS))
def test_exact_nets_of_family_a_meet_their_conditions(arch):
    """``policy_bf16_ref.exact_net`` critics at seed 900 on 0 / 1 rows with targets V - j 2^-9, lists of exactly 32 and 64 entries:
    every rounding point a no-op, every sum of absolute products below 2^24 units, and the float32 numpy gradient -- another summation
    order and precision -- equal to the float64 one bit for bit"""
    rng = np.random.default_rng(bf.EXACT_SEED)
    for n_in in (50, 24):                        # the inter input at S 5; the intra input at Us 5 under mask_obs
        layers = bf.exact_critic(n_in, arch)
        for rows in (32, 64):
            x = rng.integers(0, 2, (rows, n_in)).astype(np.float32)
            v = bf.contract_forward(x, layers, "relu")[0][:, 0]
            vtarg, j = bf.exact_targets(v, rng)
            assert np.array_equal(v - vtarg.astype(np.float64), j * 2.0 ** -9) and len(set(j.tolist())) > 3
            worst = bf.exact_conditions(x, layers, vtarg, rows)
            assert worst < 2.0 ** 24 / 1000, worst          # (a few thousand units: far below the 2^24 limit)
            grads, vl, _ = bf.exact_critic_grad(x, layers, vtarg, rows)
            assert vl == float((j * 2.0 ** -9) ** 2 @ np.ones(rows) / rows)
            for l, (gw, gb) in enumerate(grads):
                assert gw.any() and np.array_equal(gw.astype(np.float32).astype(np.float64), gw) and np.array_equal(gb.astype(np.float32).astype(np.float64), gb), l
            # a float32 evaluation in another order: per 32-row tile, reversed rows, tiles added last to first
            for l, (gw, gb) in enumerate(grads):
                acc = np.zeros_like(gw, dtype=np.float32)
                for t0 in range(rows - 32, -1, -32):
                    part = bf.exact_critic_grad(x[t0:t0 + 32][::-1], layers, vtarg[t0:t0 + 32][::-1], rows)[0][l][0]
                    acc = acc + part.astype(np.float32)
                assert np.array_equal(acc.astype(np.float64), gw), l


@pytest.mark.parametrize("arch", bf.EXACT_B_ARCHS)
def test_exact_nets_of_family_b_meet_their_conditions(arch):
    """Critics whose roundings are not no-ops but exactly decided (``ppo_bf16_ref.exact_critic_b``: first-layer weights +-1..32 with
    12-20 nonzeros per row, deeper weights +-1..4 with 6, targets V - j 2^-9 with j in -48..48) on sparse 0 / 1 rows, lists of 32 and 64
    entries: every sum of absolute products below 2^24 units, at least 16 hidden and 16 D values changed by the rounding, a
    truncated D, an unrounded D and a Wt swapped in k each flip a bit of some dW -- and the three slips that are identities on a
    one-step relu gradient from freshly seeded masters flip none (``exact_conditions``) --, and a float32 evaluation tile by tile in
    another order equal to the float64 gradient bit for bit.  ``[512] x 3`` is not in this family: its D values stay within 8 bits."""
    rng = np.random.default_rng(bf.EXACT_SEED + 1)
    for n_in, seed in ((50, bf.EXACT_SEED), (24, bf.EXACT_SEED + 3)):
        layers = bf.exact_critic_b(n_in, arch, seed)
        for rows in (32, 64):
            x = (rng.random((rows, n_in)) < bf.EXACT_B_DENSITY).astype(np.float32)
            v = bf.contract_forward(x, layers, "relu")[0][:, 0]
            vtarg, j = bf.exact_targets(v, rng, 48)
            assert np.array_equal(v - vtarg.astype(np.float64), j * 2.0 ** -9) and np.abs(j).max() > 40
            bf.exact_conditions(x, layers, vtarg, rows, "b")
            grads = bf.exact_critic_grad(x, layers, vtarg, rows)[0]
            for l, (gw, gb) in enumerate(grads):
                assert gw.any() and np.array_equal(gw.astype(np.float32).astype(np.float64), gw), l
                acc = np.zeros_like(gw, dtype=np.float32)
                for t0 in range(rows - 32, -1, -32):
                    acc = acc + bf.exact_critic_grad(x[t0:t0 + 32][::-1], layers, vtarg[t0:t0 + 32][::-1], rows)[0][l][0].astype(np.float32)
                assert np.array_equal(acc.astype(np.float64), gw), l


# ---- the random-net tier: e_bf and what the slips move ------------------------------------------------------------------------------------
def _second_step(rec, kind, nets, order, n, act, layout, slip=None, precision="bf16"):
    """The gradient of a SECOND one-minibatch step behind a first at lr 1e-2 (the stale-copy slip shows from the second step on)"""
    a, c = ("inter", "v_inter") if kind == "inter" else ("intra", "v_intra")
    return ad.ppo_update_reference(rec=rec, kind=kind, actor=ref.as_torch(nets[a]), critic=ref.as_torch(nets[c]), order=order, lo=0, hi=n, epochs=2,
                                   minibatch=ref.ALL, lr=1e-2, grad_clip=0.0, act_actor=act, act_critic=act, layout=layout, precision=precision, slip=slip)


@pytest.mark.parametrize("case", CASES)
def test_every_planted_slip_moves_a_gradient_tensor_beyond_the_gpu_cap(case):
    """Per list and gradient tensor e_bf = the relative L2 distance between the bf16 twin and the same net's f32 twin, both float64;
    the GPU comparison's cap is a quarter of it, on lists of 1 / 31 / 32 / 33 / 64 / 65 / all rows, right behind the bind and behind an
    Adam step.  Every slip of the contract, applied to the twin behind an Adam step (on the bf16 grid of freshly seeded masters the
    product on the master and the stale copy are no slips yet), must move some tensor of some list beyond that tensor's cap: a
    device that makes the slip cannot pass the GPU test.  Not every tensor, and not every list: the output layer's dW sees no hidden
    act' or Wt, and over all rows the weights' rounding, a bias that does not average out, is most of e_bf -- on the all-rows list
    alone trunc / unrounded D / master-backward moved relu24's intra tensors by 0.3 to 0.4 of the cap only.  ONE pair is no slip at
    all: relu's act' = (a > 0) is the same for the rounded and the unrounded value (rounding to nearest keeps the sign and never
    reaches zero from a normal number), so there the twin must not move."""
    nets, act, layout = _case(case)
    rec = ref.synthetic_record(B=12, seed=5, layout=layout)
    order = ad.ppo_row_order(rec, [0, 12], 2, 3)
    for kind in ("inter", "intra"):
        best = {slip: 0.0 for slip in bf.SLIPS}
        for n in (1, 31, 32, 33, 64, 65, int(order["first_" + kind][1])):
            o = torch.cat([order["order_" + kind][:1, :n]] * 2)          # (both steps on the same rows)
            good, f32 = _second_step(rec, kind, nets, o, n, act, layout), _second_step(rec, kind, nets, o, n, act, layout, precision="f32")
            g, f = bf.grad_tensors(good), bf.grad_tensors(f32)
            e_bf = {k: bf.rel_l2(g[k], f[k]) for k in g}
            assert n == 1 or min(e_bf.values()) > 1e-4, e_bf          # (bf16 training is measurably not f32 training on every tensor)
            for slip in bf.SLIPS:
                s = bf.grad_tensors(_second_step(rec, kind, nets, o, n, act, layout, slip))
                best[slip] = max([best[slip]] + [bf.rel_l2(s[k], g[k]) / (0.25 * e_bf[k]) for k in g if e_bf[k] > 0.0])
        print(f"{case} {kind}: largest move / cap per slip: " + ", ".join(f"{k} {v:.3g}" for k, v in best.items()))
        for slip, moved in best.items():
            if slip == "bf16_act_unrounded" and act == "relu":
                assert moved == 0.0
            else:
                assert moved > 1.0, (kind, slip, moved)
