"""The PPO update of mixed populations, on the CPU: the three new entries of the C ABI and their binding, the library's LDS rule
(ranenv_ppo_lds_bytes) against the header's formula, the health of the float64 twin on the cases tests/test_gpu_ppo_mixed.py runs, and
planted slips of the kind a per-member kernel can make -- each leaves the bound the GPU file puts on the gradient (8x the float32
yardstick), so that bound bites on these cases."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import ppo_mixed_ref as mx
from tests import ppo_update_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = {"ranenv_ppo_bind_mixed": 2, "ranenv_ppo_member_layout": 6, "ranenv_ppo_lds_bytes": 3}
E_INVALID = -1
# the reference's net_arch choices (agents/ray_agent.py): the four a device-trained population can hold, and the one it cannot
TRAINABLE = {"small": [64, 64], "medium": [256, 256], "big": [400, 300], "deep": [256, 256, 256]}
VERYBIG = [512, 512, 512]


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
    assert lib.ranenv_ppo_bind_mixed(None, None) == E_INVALID and b"null handle" in lib.ranenv_last_error(None)
    assert lib.ranenv_ppo_member_layout(None, 0, 0, None, None, None) == E_INVALID
    out = C.c_int64(-7)
    assert lib.ranenv_ppo_lds_bytes(None, None, C.byref(out)) == E_INVALID and out.value == -7


def _lds(actor_dims, critic_dims):
    from intent_radio_sched_multi_slice_amd.batched_env import ppo_lds_bytes
    return ppo_lds_bytes(actor_dims, critic_dims)


def _formula(dims):
    return 4096 + 128 * sum(ref.net_ld(ref.pad32(w)) for w in dims)


def test_the_librarys_lds_rule_is_the_headers_formula():
    """ranenv_ppo_lds_bytes against ref.lds_bytes' formula on 200 seeded shapes, depths 1..4, widths 1..512, actor and critic drawn
    apart; without a critic it is the actor's alone; malformed nets are RANENV_E_INVALID."""
    rng = np.random.default_rng(2024)
    for _ in range(200):
        dims = [[int(rng.integers(1, 513)) for _ in range(int(rng.integers(1, 5)) + 2)] for _ in range(2)]
        assert _lds(dims[0], dims[1]) == max(_formula(dims[0]), _formula(dims[1])), dims
        assert _lds(dims[0], None) == _formula(dims[0]), dims
    # ... and with ref.lds_bytes itself, which takes both kinds of one (S, Us, layout): the larger of the two kinds' pairs
    for S_, Us, layout, (aw, _), (cw, _) in ref.SHAPES.values():
        n_in = ref.intra_width(Us, layout)
        got = max(_lds([10 * S_] + aw + [2 * S_], [10 * S_] + cw + [1]), _lds([n_in] + aw + [3], [n_in] + cw + [1]))
        assert got == ref.lds_bytes(S_, Us, layout, aw, cw)
    from intent_radio_sched_multi_slice_amd import _lib
    lib, out = _lib.load(), C.c_int64(-7)
    for bad in ([30, 6], [30, 1, 2, 3, 4, 5, 6], [30, 513, 6], [30, 0, 6], [0, 32, 6]):
        mlp = _lib.Mlp()
        mlp.n_hidden = len(bad) - 2
        for i, d in enumerate(bad[:6]):
            mlp.dims[i] = d
        assert lib.ranenv_ppo_lds_bytes(C.byref(mlp), None, C.byref(out)) == E_INVALID and out.value == -7, bad


def test_the_four_trainable_reference_architectures_fit_the_plan_and_verybig_does_not():
    S_, Us = 10, 100
    for layout in ("obs", "mask_obs"):
        n_in = ref.intra_width(Us, layout)
        for name, w in TRAINABLE.items():
            assert _lds([10 * S_] + w + [2 * S_], [10 * S_] + w + [1]) <= ref.LDS_MAX, name
            assert _lds([n_in] + w + [3], [n_in] + w + [1]) <= ref.LDS_MAX, name
            assert ref.lds_bytes(S_, Us, layout, w, w) <= ref.LDS_MAX
        assert _lds([10 * S_] + VERYBIG + [2 * S_], [10 * S_] + VERYBIG + [1]) > ref.LDS_MAX
        assert _lds([n_in] + VERYBIG + [3], None) > ref.LDS_MAX
    # the GPU file's shapes: every member of both cases inside, the edge case's owner AT the edge, the re-bind's shape beyond
    for case in mx.CASES:
        for aw, _, cw, _ in mx.shapes(case):
            assert ref.lds_bytes(mx.S, mx.US, mx.layout(case), aw, cw) <= ref.LDS_MAX
    assert _lds([10 * mx.S] + mx.CASES["edge"][1][0][0] + [2 * mx.S], None) == 162304
    assert _lds([10 * mx.S] + mx.BEYOND[0] + [2 * mx.S], None) == 171008 > ref.LDS_MAX
    assert ref.net_ld(ref.pad32(33)) % 64 != 0 and ref.net_ld(160) % 64 != 0


def test_the_beyond_shape_fits_the_edge_cases_extent():
    """The re-bind that the GPU file expects refused for its LDS need is not refused for its size first"""
    from intent_radio_sched_multi_slice_amd.batched_env import packed_net_floats
    extent = max(packed_net_floats([10 * mx.S] + aw + [2 * mx.S]) for aw, _, _, _ in mx.shapes("edge"))
    assert packed_net_floats([10 * mx.S] + mx.BEYOND[0] + [2 * mx.S]) <= extent


@pytest.mark.parametrize("case", list(mx.CASES))
def test_the_twin_is_healthy_on_the_gpu_cases(case):
    """For every member and kind, with the nets and the record the GPU file uses: no gradient tensor of the float64 twin is zero, the
    float32 yardstick is finite, and the record holds masked and unmasked positions and clipped and unclipped rows."""
    rec = mx.record(case)
    mask = rec["mask_inter"]
    assert bool((mask == 0).any()) and bool((mask != 0).any())
    assert bool((rec["mask_intra"] == 0).any()) and bool((rec["mask_intra"] != 0).any())
    for kind in ("inter", "intra"):
        for m in range(len(mx.FIRST) - 1):
            t64, t32 = mx.twin_gradient(case, kind, m), mx.twin_gradient(case, kind, m, torch.float32)
            for net in ("actor", "critic"):
                for li, (g64, g32) in enumerate(zip(t64["grad"][net], t32["grad"][net])):
                    for name, x64, x32 in zip("Wb", g64, g32):
                        assert float(x64.norm()) > 0.0, (case, kind, m, net, li, name)
                        assert bool(torch.isfinite(x32).all()), (case, kind, m, net, li, name)
            assert 0.0 < t64["stats"][0, 4] < 1.0, (case, kind, m, "clip fraction", t64["stats"][0, 4])
            assert max(mx.ratios(t64["grad"], t32["grad"], t32["grad"]).values()) <= 1.0 + 1e-9


def _np_grad(t):
    return {net: [(w.numpy(), b.numpy()) for w, b in t["grad"][net]] for net in ("actor", "critic")}


def test_planted_slips_between_members_leave_the_gpu_bound():
    """Evaluated with the twin alone, on the base case: member m under member m + 1's activation; member 1's first hidden width cut
    to member 0's; member m's critic gradient read at member 0's actor-floats offset.  Each differs from the true twin by more than
    the GPU test's bound, 8x the float32 yardstick, in some tensor."""
    case, G = "base", len(mx.FIRST) - 1
    sh = mx.shapes(case)
    nets = mx.mixed_nets(case)
    for kind, (a, c) in (("inter", ("inter", "v_inter")), ("intra", ("intra", "v_intra"))):
        true = {m: (mx.twin_gradient(case, kind, m), mx.twin_gradient(case, kind, m, torch.float32)) for m in range(G)}
        # 1. the neighbour's activation (where it is another one)
        differ = [m for m in range(G) if sh[m][1] != sh[(m + 1) % G][1]]
        assert len(differ) >= 2
        for m in differ:
            other = sh[(m + 1) % G]
            wrong = mx.twin_gradient(case, kind, m, acts=(other[1], other[3]))
            r = max(mx.ratios(true[m][0]["grad"], true[m][1]["grad"], wrong["grad"]).values())
            print(f"{kind} member {m} under member {(m + 1) % G}'s activation: {r:.3g} x the yardstick")
            assert r > 8.0
        # 2. member 1's hidden width 40 cut to member 0's 24: the units beyond take no part, their gradient is zero
        m, keep = 1, sh[0][0][0]
        assert sh[m][0][0] > keep
        layers = ref.layers_of(nets[a][m])
        cut = [(layers[0][0][:keep], layers[0][1][:keep]), (layers[1][0][:, :keep], layers[1][1])] + layers[2:]
        wrong = _np_grad(mx.twin_gradient(case, kind, m, nets=(cut, ref.layers_of(nets[c][m]))))
        full = _np_grad(true[m][0])
        (w0, b0), (w1, b1) = wrong["actor"][0], wrong["actor"][1]
        W0, B0, W1 = np.zeros_like(full["actor"][0][0]), np.zeros_like(full["actor"][0][1]), np.zeros_like(full["actor"][1][0])
        W0[:keep], B0[:keep], W1[:, :keep] = w0, b0, w1
        wrong["actor"][0], wrong["actor"][1] = (W0, B0), (W1, b1)
        r = mx.ratios(true[m][0]["grad"], true[m][1]["grad"], wrong)
        print(f"{kind} member {m} at member 0's hidden width: {max(r.values()):.3g} x the yardstick")
        assert r["actor", 0, "W"] > 8.0 and r["actor", 1, "W"] > 8.0
        # 3. the critic's gradient read behind member 0's actor floats in place of the member's own
        for m in (1, 2):
            g = _np_grad(true[m][0])
            flat = mx.pack_grad(g["actor"], g["critic"])
            mine, theirs = mx.packed_floats(g["actor"]), mx.packed_floats(_np_grad(true[0][0])["actor"])
            assert mine != theirs
            right = mx.unpack_at(flat, g["critic"], mine)
            for (w, b), (x, y) in zip(right, g["critic"]):
                assert np.array_equal(w, x) and np.array_equal(b, y)
            wrong = {"actor": g["actor"], "critic": mx.unpack_at(flat, g["critic"], theirs)}
            r = mx.ratios(true[m][0]["grad"], true[m][1]["grad"], wrong)
            worst = max(v for k, v in r.items() if k[0] == "critic")
            print(f"{kind} member {m}'s critic gradient at member 0's offset: {worst:.3g} x the yardstick")
            assert worst > 8.0
