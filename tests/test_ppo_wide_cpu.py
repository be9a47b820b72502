"""The wide binding of the PPO update, on the CPU: the two new entries of the C ABI and their binding, the library's wide plan
(ranenv_ppo_wide_bytes) against the header's two formulas restated in tests/ppo_wide_ref.py, the reference's `verybig` on both sides
of the two plans, the shapes the GPU file's re-binds rely on, and the health of the float64 twin on the nets tests/test_gpu_ppo_wide.py
trains."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import ppo_update_ref as ref
from tests import ppo_wide_ref as wd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = {"ranenv_ppo_bind_wide": 3, "ranenv_ppo_wide_bytes": 4}
E_INVALID = -1
VERYBIG = [512, 512, 512]


def _mlp(dims):
    from intent_radio_sched_multi_slice_amd import _lib
    mlp = _lib.Mlp()
    mlp.n_hidden = len(dims) - 2
    for i, d in enumerate(dims[:6]):
        mlp.dims[i] = d
    return mlp


def test_the_c_abi_declares_the_new_entries_and_the_binding_matches():
    from intent_radio_sched_multi_slice_amd import _lib
    header = open(os.path.join(REPO, "include", "ranenv.h")).read()
    lib = _lib.load()
    for name, n_args in NEW_EXPORTS.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == n_args, name
        assert name in _lib.EXPORTS and len(_lib.FUNCTIONS[name][1]) == n_args and hasattr(lib, name), name
    assert "#define RANENV_ABI_VERSION 10" in header and _lib.ABI_VERSION == 10 and lib.ranenv_abi_version() == 10
    assert lib.ranenv_ppo_bind_wide(None, 0, None) == E_INVALID and b"null handle" in lib.ranenv_last_error(None)
    assert lib.ranenv_ppo_bind_wide(None, 2, None) == E_INVALID and b"mixed 2" in lib.ranenv_last_error(None)
    lds, park = C.c_int64(-7), C.c_int64(-7)
    assert lib.ranenv_ppo_wide_bytes(None, None, C.byref(lds), C.byref(park)) == E_INVALID and lds.value == park.value == -7
    actor = _mlp([50, 64, 10])
    assert lib.ranenv_ppo_wide_bytes(C.byref(actor), None, None, None) == E_INVALID
    # either output alone
    assert lib.ranenv_ppo_wide_bytes(C.byref(actor), None, C.byref(lds), None) == 0 and lds.value == wd.wide_lds_bytes([50, 64, 10])
    assert lib.ranenv_ppo_wide_bytes(C.byref(actor), None, None, C.byref(park)) == 0 and park.value == wd.wide_scratch_floats([50, 64, 10])
    for bad in ([30, 6], [30, 1, 2, 3, 4, 5, 6], [30, 513, 6], [30, 0, 6], [0, 32, 6]):
        lds.value = -7
        bad_mlp = _mlp(bad)
        assert lib.ranenv_ppo_wide_bytes(C.byref(bad_mlp), None, C.byref(lds), C.byref(park)) == E_INVALID and lds.value == -7, bad


def test_the_librarys_wide_plan_is_the_headers_two_formulas():
    """ranenv_ppo_wide_bytes (through ppo_lds_bytes(wide=True) and ppo_wide_scratch_floats) against the restated formulas on 200 seeded
    shapes: S 1..16, both intra layouts, 1..4 hidden layers of widths 1..512, actor and critic drawn apart, both kinds; without a
    critic it is the actor's alone; every one within 136 192 bytes."""
    from intent_radio_sched_multi_slice_amd.batched_env import ppo_lds_bytes, ppo_wide_scratch_floats
    rng = np.random.default_rng(2025)
    seen_layouts, top = set(), 0
    for _ in range(200):
        S_, Us = int(rng.integers(1, 17)), int(rng.integers(1, 17))
        layout = ("obs", "mask_obs")[int(rng.integers(0, 2))]
        seen_layouts.add(layout)
        hidden = [[int(rng.integers(1, 513)) for _ in range(int(rng.integers(1, 5)))] for _ in range(2)]
        for n_in, n_out in ((10 * S_, 2 * S_), (ref.intra_width(Us, layout), 3)):
            actor, critic = [n_in] + hidden[0] + [n_out], [n_in] + hidden[1] + [1]
            assert ppo_lds_bytes(actor, critic, wide=True) == wd.wide_lds_bytes(actor, critic) <= wd.WIDE_LDS_MAX, (actor, critic)
            assert ppo_lds_bytes(actor, None, wide=True) == wd.wide_lds_bytes(actor), actor
            assert ppo_wide_scratch_floats(actor, critic) == wd.wide_scratch_floats(actor, critic), (actor, critic)
            assert ppo_wide_scratch_floats(actor) == wd.wide_scratch_floats(actor), actor
            top = max(top, wd.wide_lds_bytes(actor, critic))
            # (the plain flag still gives the plain plan)
            assert ppo_lds_bytes(actor, critic) == ppo_lds_bytes(actor, critic, wide=False) == max(4096 + 128 * sum(ref.net_ld(w) for w in wd.padded(d)) for d in (actor, critic))
    assert seen_layouts == {"obs", "mask_obs"} and top > ref.LDS_MAX // 2
    # the largest net the acting path accepts sits AT the bound
    assert ppo_lds_bytes([160, 512, 512, 512, 512, 32], None, wide=True) == wd.WIDE_LDS_MAX < ref.LDS_MAX


@pytest.mark.parametrize("S_", [5, 10])
def test_verybig_is_beyond_the_plain_plan_and_inside_the_wide_one(S_):
    from intent_radio_sched_multi_slice_amd.batched_env import ppo_lds_bytes, ppo_wide_scratch_floats
    for layout in ("obs", "mask_obs"):
        for actor, critic in wd.kind_dims(VERYBIG, layout, S_, 100 if S_ == 10 else 5).values():
            assert ppo_lds_bytes(actor, critic) > ref.LDS_MAX
            assert ppo_lds_bytes(actor, critic, wide=True) <= wd.WIDE_LDS_MAX
            assert ppo_wide_scratch_floats(actor, critic) == 32 * (ref.net_ld(ref.pad32(actor[0])) + 3 * 516)
    if S_ == 5:
        assert ppo_lds_bytes([50] + VERYBIG + [10], [50] + VERYBIG + [1]) == 219648
        assert ppo_lds_bytes([50] + VERYBIG + [10], [50] + VERYBIG + [1], wide=True) == 136192


def test_the_shapes_the_gpu_file_relies_on():
    """The GPU file's other nets: `past_limit` is the 170 496 bytes one step past the plain plan; members 0 and 2 of the mixed
    population fit the plain plan and member 1 does not; the re-bind that must be refused for its parked rows fits every extent and
    the wide LDS plan, and the one that must be refused for its size does not fit the extent."""
    from intent_radio_sched_multi_slice_amd.batched_env import packed_net_floats, ppo_lds_bytes, ppo_wide_scratch_floats
    widths, _, layout = wd.BEYOND["past_limit"]
    assert ref.lds_bytes(wd.S, wd.US, layout, widths, widths) == 170496 > ref.LDS_MAX
    fits = [all(ppo_lds_bytes(a, c) <= ref.LDS_MAX for a, c in wd.kind_dims(w, wd.MIXED_LAYOUT).values()) for w, _ in wd.MIXED]
    assert fits == [True, False, True]
    allocated = max(ppo_wide_scratch_floats(a, c) for w, _ in wd.MIXED for a, c in wd.kind_dims(w, wd.MIXED_LAYOUT).values())
    extent = max(packed_net_floats(wd.kind_dims(w, wd.MIXED_LAYOUT)["inter"][0]) for w, _ in wd.MIXED)
    grown = wd.kind_dims(wd.OUTGROWS_SCRATCH, wd.MIXED_LAYOUT)["inter"]
    assert packed_net_floats(grown[0]) <= extent and ppo_lds_bytes(grown[0], None, wide=True) <= wd.WIDE_LDS_MAX
    assert ppo_wide_scratch_floats(grown[0], None) > allocated
    assert packed_net_floats(wd.kind_dims(wd.OUTGROWS_EXTENT, wd.MIXED_LAYOUT)["inter"][0]) > extent


def test_the_bit_identity_list_is_every_shape_that_fits_both_plans():
    """wd.BOTH_PLANS_SHAPES is every entry of ref.SHAPES whose nets fit the plain plan (the wide plan holds every net); A sits at that
    plan's own edge, 162 304 of 163 840 bytes.  `deepest` is the largest net the acting path accepts: it sits AT the wide plan's bound,
    parks four slabs of 516 floats a row behind the input's, and lies far beyond the plain plan."""
    from intent_radio_sched_multi_slice_amd.batched_env import ppo_lds_bytes, ppo_wide_scratch_floats
    fits = []
    for name, (S_, Us, layout, (aw, _), (cw, _)) in ref.SHAPES.items():
        if ref.lds_bytes(S_, Us, layout, aw, cw) <= ref.LDS_MAX:
            fits.append(name)
    assert tuple(fits) == tuple(wd.BOTH_PLANS_SHAPES) == tuple(ref.SHAPES)
    S_, Us, layout, (aw, _), (cw, _) = ref.SHAPES["A"]
    assert ref.lds_bytes(S_, Us, layout, aw, cw) == 162304
    widths, _, layout = wd.BEYOND["deepest"]
    assert widths == [512] * 4
    for actor, critic in wd.kind_dims(widths, layout).values():
        assert ppo_lds_bytes(actor, critic) > ref.LDS_MAX
        assert ppo_lds_bytes(actor, critic, wide=True) == wd.WIDE_LDS_MAX
        assert ppo_wide_scratch_floats(actor, critic) == 32 * (ref.net_ld(ref.pad32(actor[0])) + 4 * 516)


def _twin_is_healthy(rec, nets, acts, layout, what):
    from intent_radio_sched_multi_slice_amd import adapters as ad
    o = wd.order(rec, 1)
    assert bool((rec["mask_inter"] == 0).any()) and bool((rec["mask_inter"] != 0).any())
    for kind, (a, c) in (("inter", ("inter", "v_inter")), ("intra", ("intra", "v_intra"))):
        f = o["first_" + kind]
        for m in range(wd.G):
            args = dict(epochs=1, minibatch=ref.ALL, lr=0.0, grad_clip=0.0, act_actor=acts[m], act_critic=acts[m], layout=layout, clip=0.2, vf_coeff=0.5,
                        ent_coeff=0.01, adv_norm=True)
            t64 = ad.ppo_update_reference(rec, kind, ref.layers_of(nets[a][m]), ref.layers_of(nets[c][m]), o["order_" + kind], int(f[m]), int(f[m + 1]),
                                          dtype=torch.float64, **args)
            for net in ("actor", "critic"):
                for li, pair in enumerate(t64["grad"][net]):
                    for name, x in zip("Wb", pair):
                        assert float(x.norm()) > 0.0, (what, kind, m, net, li, name)
            assert 0.0 < t64["stats"][0, 4] < 1.0, (what, kind, m, "clip fraction", t64["stats"][0, 4])


@pytest.mark.parametrize("case", list(wd.BEYOND))
def test_the_twin_is_healthy_on_the_nets_beyond_the_plain_plan(case):
    """For every member and kind, with the nets, the seed and the record the GPU file uses: no gradient tensor of the float64 twin is
    zero, and the record holds clipped and unclipped rows."""
    _twin_is_healthy(wd.beyond_record(case), wd.beyond_nets(case), [wd.BEYOND[case][1]] * wd.G, wd.BEYOND[case][2], case)


def test_the_twin_is_healthy_on_the_mixed_population():
    _twin_is_healthy(wd.mixed_record(), wd.mixed_nets(), [a for _, a in wd.MIXED], wd.MIXED_LAYOUT, "mixed")
