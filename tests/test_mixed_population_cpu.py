"""Mixed populations without a device: ``BatchedRanEnv``'s handling of ``mixed=True`` lists and of per-member gamma / lambda on a stub
without a library, the packed-size rule of the library (ranenv_packed_net_floats) against its restatement in
tests/mixed_population_ref.py, the new exports, and the planted slips that the twin of the GPU tests must show."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import mixed_population_ref as mx
from tests import population_ref as pop

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1357_9BDF_2468_ACE0
E_INVALID = -1
NEW_EXPORTS = ("ranenv_set_population_policy_mixed", "ranenv_set_population_value_mixed", "ranenv_get_population_net", "ranenv_packed_net_floats",
               "ranenv_set_population_gae", "ranenv_gae_population")


@pytest.fixture(scope="module")
def lib():
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.csrc import build
    build.build()
    return _lib.load()


class _Reached(Exception):
    """The binding call was reached: every check in front of it passed"""


def _stub(first=mx.FIRST, reach=False):
    """BatchedRanEnv's list handling without a handle (the pattern of tests/test_population_cpu.py): S 3 / Us 4 on the CPU, no library
    -- a call that reached one would raise AttributeError, not ValueError.  ``reach``: the step that hands the checked lists to the
    library raises ``_Reached`` with the entry's name instead."""
    from intent_radio_sched_multi_slice_amd.batched_env import BatchedRanEnv
    env = object.__new__(BatchedRanEnv)
    env.S, env.Us, env.W, env.B, env.device = 3, 4, 17, first[-1], torch.device("cpu")
    env._population, env._intra_layout, env._keep, env._h, env._lib = np.asarray(first, dtype=np.int32), 0, {}, None, None
    env._recorder, env._gae_per_member = None, False
    if reach:
        def reached(call, key, G, lists, *args):
            assert G == len(first) - 1 and all(x is None or len(x[0]) == G for x in lists)
            raise _Reached(call)
        env._set_population_nets = reached
    return env


# ---- the stub ----------------------------------------------------------------------------------------------------------------------
def test_mixed_lists_pass_the_checks_and_reach_the_mixed_entries():
    from tests.gpu_common import make_inter_net, make_net
    inters, intras, v_inters, v_intras = mx.make_nets("mixed", 5)
    env = _stub(reach=True)
    with pytest.raises(_Reached, match="ranenv_set_population_policy_mixed"):
        env.set_policy_network(inters, intras, mixed=True)
    with pytest.raises(_Reached, match="ranenv_set_population_policy_mixed"):
        env.set_policy_network(inters, None, mixed=True)
    with pytest.raises(_Reached, match="ranenv_set_population_value_mixed"):
        env.set_value_network(v_inters, v_intras, mixed=True)
    w_inters, w_intras, _, _ = mx.make_nets("wide", 5)               # tanh and relu members in one list
    with pytest.raises(_Reached, match="ranenv_set_population_policy_mixed"):
        env.set_policy_network(w_inters, w_intras, mixed=True)
    # equal shapes through the mixed path are fine too; without the flag the uniform entry is reached
    same = mx.make_nets("mixed", 5, members=[1, 1, 1])
    with pytest.raises(_Reached, match="ranenv_set_population_policy_mixed"):
        env.set_policy_network(same[0], same[1], mixed=True)
    with pytest.raises(_Reached, match="ranenv_set_population_policy$"):
        env.set_policy_network(same[0], same[1])
    # what still raises, before any library call
    env = _stub()
    with pytest.raises(ValueError, match="one per member is 3"):
        env.set_policy_network(inters[:2], intras[:2], mixed=True)
    with pytest.raises(ValueError, match="one per member is 3"):
        env.set_value_network(v_inters, v_intras + v_intras[:1], mixed=True)
    with pytest.raises(ValueError, match="input width"):
        env.set_policy_network(inters[:2] + [make_net([31, 24, 6], "tanh", 1)], intras, mixed=True)
    with pytest.raises(ValueError, match="output width"):
        env.set_policy_network(inters[:2] + [make_net([30, 24, 5], "tanh", 1)], intras, mixed=True)
    with pytest.raises(ValueError, match="input width"):
        env.set_policy_network(inters, intras[:2] + [make_net([21, 24, 3], "tanh", 1)], mixed=True)       # the other layout's width
    with pytest.raises(ValueError, match="output width"):
        env.set_value_network(v_inters, v_intras[:2] + [make_net([17, 24, 3], "tanh", 1)], mixed=True)
    with pytest.raises(ValueError, match="another input layout"):
        env.set_value_network(v_inters, v_intras[:2] + [make_net([21, 24, 1], "tanh", 1)], mixed=True)    # mask_obs beside obs critics
    with pytest.raises(ValueError, match="precision"):
        env.set_policy_network(inters, intras, precision="fp8", mixed=True)
    with pytest.raises(ValueError, match="hidden layers"):
        env.set_policy_network(inters[:2] + [make_inter_net(3, [8] * 5, "tanh", 1)], intras, mixed=True)
    with pytest.raises(ValueError, match="one per member"):
        env.set_policy_network(inters[0], intras[0], mixed=True)     # one net is no population
    with pytest.raises(ValueError, match="a list of nets, one per member"):
        env.set_policy_network(inters, intras[0], mixed=True)
    # mixed=False is as it was
    with pytest.raises(ValueError, match="differs from net 0"):
        env.set_policy_network(inters, intras)
    with pytest.raises(ValueError, match="differs from net 0"):
        env.set_policy_network(same[0], intras, mixed=False)
    with pytest.raises(ValueError, match="differs from net 0"):
        env.set_value_network(v_inters, None)
    env._population = None
    with pytest.raises(ValueError, match="no population set"):
        env.set_policy_network(inters, intras, mixed=True)
    with pytest.raises(ValueError, match="no population set"):
        env.set_value_network(v_inters, v_intras, mixed=True)


def test_gamma_and_lambda_sequences_are_checked_before_any_library_call():
    env = _stub()
    assert env._gae_pairs(0.99, 0.95) is None
    g, l = env._gae_pairs(mx.GAMMA, 0.9)
    assert g.tolist() == mx.GAMMA and l.tolist() == [0.9] * 3 and g.dtype == l.dtype == np.float64
    g, l = env._gae_pairs(0.5, np.asarray(mx.LAM, dtype=np.float32))
    assert g.tolist() == [0.5] * 3 and np.allclose(l, mx.LAM, rtol=1e-7)
    r, v, d = torch.zeros(2, 70, 4, dtype=torch.float64), torch.zeros(3, 70, 4), torch.zeros(2, 70, dtype=torch.uint8)
    for bad in ([0.9, 0.9], [0.9] * 4, []):
        with pytest.raises(ValueError, match="one per member is 3"):
            env.collect(2, gamma=bad)
        with pytest.raises(ValueError, match="one per member is 3"):
            env.collect(2, lam=bad)
        with pytest.raises(ValueError, match="one per member is 3"):
            env.gae(r, v, d, gamma=mx.GAMMA, lam=bad)
    env._population = None
    with pytest.raises(ValueError, match="no population set"):
        env.collect(2, gamma=mx.GAMMA, lam=mx.LAM)
    with pytest.raises(ValueError, match="no population set"):
        env.gae(r, v, d, lam=mx.LAM)
    with pytest.raises(ValueError, match="no population set"):
        env.population_net("inter", 0)
    env = _stub()
    with pytest.raises(ValueError, match="role must be"):
        env.population_net("actor", 0)
    with pytest.raises(ValueError, match="outside the population"):
        env.population_net("inter", 3)


# ---- the size rule -----------------------------------------------------------------------------------------------------------------
def _floats(lib, dims, prec):
    out = C.c_int64(-7)
    rc = lib.ranenv_packed_net_floats(len(dims) - 2, (C.c_int32 * 6)(*dims), prec, C.byref(out))
    return rc, out.value


def test_the_librarys_packed_size_is_the_restatements(lib):
    from intent_radio_sched_multi_slice_amd.batched_env import packed_net_floats
    rng = np.random.default_rng(77)
    seen = set()
    for _ in range(200):
        n_hidden = int(rng.integers(1, 5))
        dims = [int(rng.choice([17, 21, 30, 50, 160]))] + [int(x) for x in rng.choice([1, 24, 31, 32, 33, 64, 96, 300, 400, 511, 512], n_hidden)] + \
               [int(rng.choice([1, 3, 6, 10]))]
        for prec, bf in ((0, False), (1, True)):
            assert _floats(lib, dims, prec) == (0, mx.packed_floats(dims, bf)), (dims, prec)
            assert packed_net_floats(dims, "bf16" if bf else "f32") == mx.packed_floats(dims, bf)
        seen.add(n_hidden)
    assert seen == {1, 2, 3, 4}
    assert _floats(lib, [30, 24, 6], 0) == (0, 32 * 32 + 32 + 32 * 32 + 32) and _floats(lib, [30, 24, 6], 1) == (0, 32 * 16 + 32 + 32 * 16 + 32)
    # the extent of the GPU tests' actors is member 2's -- every member's shape fits every member -- and a [512] net does not fit it
    sizes = [mx.packed_floats([30] + h + [6]) for h in mx.SETS["mixed"][0]]
    assert max(sizes) == sizes[2] > sizes[1] > sizes[0]
    assert packed_net_floats(mx.make_nets("mixed", 1)[0][2]) == sizes[2] < mx.packed_floats([30, 512, 6])
    # argument errors
    out = C.c_int64(-7)
    for bad in ([30, 6], [30, 8, 8, 8, 8, 8, 6]):                   # depth 0 and 5
        assert lib.ranenv_packed_net_floats(len(bad) - 2, (C.c_int32 * 8)(*bad), 0, C.byref(out)) == E_INVALID and out.value == -7
    for bad in ([30, 0, 6], [30, 513, 6], [30, 32, 513, 6], [30, 32, -1, 6], [0, 32, 6], [30, 32, 0]):
        assert _floats(lib, bad, 0) == (E_INVALID, -7), bad
    assert _floats(lib, [30, 32, 6], 2)[0] == E_INVALID
    assert lib.ranenv_packed_net_floats(1, None, 0, C.byref(out)) == E_INVALID and lib.ranenv_packed_net_floats(1, (C.c_int32 * 3)(30, 32, 6), 0, None) == E_INVALID
    with pytest.raises(ValueError):
        packed_net_floats([30, 6])
    with pytest.raises(ValueError):
        packed_net_floats([30, 32, 6], "fp8")


# ---- the exports -------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_new_exports(lib):
    from intent_radio_sched_multi_slice_amd import _lib
    header = open(os.path.join(REPO, "include", "ranenv.h")).read()
    declared = set(re.findall(r"^int (ranenv_[a-z_]+)\s*\(", header, flags=re.M))
    for name in NEW_EXPORTS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
        proto = re.search(r"^int " + name + r"\(([^)]*)\)", header, flags=re.M).group(1)
        assert len(_lib.FUNCTIONS[name][1]) == len(proto.split(",")), name
    assert [len(_lib.FUNCTIONS[n][1]) for n in NEW_EXPORTS] == [7, 5, 8, 4, 4, 12]
    assert lib.ranenv_abi_version() == _lib.ABI_VERSION == 10 and "#define RANENV_ABI_VERSION 10" in header
    # the calls that need a handle refuse a null one
    assert lib.ranenv_set_population_gae(None, 3, None, None) == E_INVALID and lib.ranenv_get_population_net(None, 0, 0, None, None, None, None, None) == E_INVALID


# ---- planted slips -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin():
    """Per (set, stochastic): snapshot, nets, the float64 reference -- computed once, shared, left unchanged"""
    out = {}
    for k, name in enumerate(mx.SETS):
        snap = pop.synthetic_snapshot(mx.CASE, 80 + k)
        nets = mx.make_nets(name, 3000)
        for st in (False, True):
            out[name, st] = (snap, nets, mx.policy_ref(snap, nets[0], nets[1], mx.FIRST, st, SEED))
    return out


@pytest.mark.parametrize("slip", ["next", "truncate"])
@pytest.mark.parametrize("stochastic", [False, True])
@pytest.mark.parametrize("name", list(mx.SETS))
def test_a_shifted_table_or_a_truncated_member_moves_the_twin_beyond_the_bound(twin, name, stochastic, slip):
    """The GPU tests hold the device against this twin within the float64 bounds (check_actions) and against one-net handles bit for
    bit: every env whose net the slip changes leaves both bars, the others stay, and the slipped twin's own actions, handed to
    check_actions as a device's, are refused."""
    from tests import policy_ref as pr
    snap, nets, ref = twin[name, stochastic]
    wrong = mx.policy_ref(snap, nets[0], nets[1], mx.FIRST, stochastic, SEED, slip=slip)
    moved = np.ones(70, dtype=bool)
    if slip == "truncate":
        moved[:mx.FIRST[1]] = False                                   # member 0 is its own width
    assert moved.sum() == (70 if slip == "next" else 65)
    assert np.allclose(wrong.out[~moved], ref.out[~moved], rtol=0, atol=1e-12) and np.allclose(wrong.logits[~moved], ref.logits[~moved], rtol=0, atol=1e-12)
    for b in np.flatnonzero(moved):
        assert np.any(np.abs(wrong.out[b] - ref.out[b]) > ref.out_t[b] + wrong.out_t[b]), (slip, b)
        assert np.any(np.abs(wrong.logits[b] - ref.logits[b]) > ref.logit_bound[b] + wrong.logit_bound[b]), (slip, b)
    with pytest.raises(AssertionError, match="outside the bound|intra choices differ"):
        pr.check_actions(ref, wrong.scores, wrong.intra, min_safe=0.9)
    assert pr.check_actions(ref, ref.scores, ref.intra, min_safe=0.9) >= 0.9 * 70 * mx.S


@pytest.mark.parametrize("ends", [False, True])
def test_the_neighbours_gamma_and_lambda_move_every_members_advantages(ends):
    """The GPU comparison is bit for bit: under the neighbouring member's pair every member's adv and vtarg move by far more than a
    float32 rounding, with and without an episode end inside the T steps; the per-member pass is adapters.gae of the slice."""
    from intent_radio_sched_multi_slice_amd.adapters import gae
    rng = np.random.default_rng(9)
    T, B, Cn = 3, 70, mx.S + 1
    reward, vf = rng.standard_normal((T, B, Cn)), rng.standard_normal((T + 1, B, Cn)).astype(np.float32)
    done = np.zeros((T, B), dtype=np.uint8)
    if ends:
        done[1] = 1
    adv, vtarg = mx.gae_ref(reward, vf, done, mx.FIRST, mx.GAMMA, mx.LAM)
    w_adv, w_vtarg = mx.gae_ref(reward, vf, done, mx.FIRST, mx.GAMMA, mx.LAM, slip="next")
    for m in range(mx.G):
        sl = slice(mx.FIRST[m], mx.FIRST[m + 1])
        a, v = gae(reward[:, sl], vf[:, sl], done[:, sl], mx.GAMMA[m], mx.LAM[m])
        assert np.array_equal(adv[:, sl], a) and np.array_equal(vtarg[:, sl], v)
        for got, want in ((w_adv[:, sl], a), (w_vtarg[:, sl], v)):
            moved = np.abs(got.astype(np.float64) - want) > 1e-4 * (1.0 + np.abs(want))
            assert moved.any(axis=(0, 2)).all(), m                   # every env of the member shows
    one = gae(reward, vf, done, 0.99, 0.95)
    same = mx.gae_ref(reward, vf, done, mx.FIRST, [0.99] * 3, [0.95] * 3)
    assert np.array_equal(one[0], same[0]) and np.array_equal(one[1], same[1])
