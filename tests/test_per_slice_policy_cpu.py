"""Non-shared intra policies without a device: the float32 restatement (``adapters.ibsched_policy_actions`` with a list of S nets)
against the float64 twin of tests/per_slice_policy_ref.py on the shapes and nets the GPU tests use, three planted slips of the
slice -> net mapping that ``check_actions`` must catch, the checkpoint reader ``rllib_per_slice_layers``, and the two new exports."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import per_slice_policy_ref as ps
from tests import policy_ref as pr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1357_9BDF_2468_ACE0
MODES = [False, True]


def _restatement(snap, inter, intras, stochastic, layout):
    from intent_radio_sched_multi_slice_amd import adapters
    B = snap["obs_inter"].shape[0]
    return adapters.ibsched_policy_actions(snap["obs_inter"], snap["mask_inter"], inter, snap["obs_intra"], snap["mask_intra"], intras,
                                           stochastic=stochastic, seed=SEED, intra_input=layout, env_ids=np.arange(B),
                                           episode=snap["episode_number"], step=snap["step_number"])


@pytest.fixture(scope="module")
def twins():
    """Per (case, stochastic): snapshot, nets, the float64 reference -- computed once, shared, left unchanged."""
    out = {}
    for k, case in enumerate(ps.CASES):
        snap = ps.synthetic_snapshot(case, 40 + k)
        inter, intras, _, _ = ps.make_nets(*ps.TWIN_NETS[k])
        for st in MODES:
            out[k, st] = (snap, inter, intras, ps.policy_ref(snap, inter, intras, st, SEED, case[5]))
    return out


@pytest.mark.parametrize("stochastic", MODES)
@pytest.mark.parametrize("k", range(len(ps.CASES)), ids=ps.CASE_IDS)
def test_restatement_with_a_net_per_slice_is_within_the_twins_bounds(twins, k, stochastic):
    snap, inter, intras, ref = twins[k, stochastic]
    S, Us, B = ps.CASES[k][:3]
    assert ref.intra_safe.mean() >= 0.9, ref.intra_safe.mean()          # (check_actions' own cap, for the GPU file's nets and shapes)
    scores, intra = _restatement(snap, inter, intras, stochastic, ps.CASES[k][5])
    assert intra.shape == (B, S) and intra.dtype == torch.uint8
    assert pr.check_actions(ref, scores, intra, min_safe=0.9) >= 0.9 * B * S
    # the nets differ: the shared restatement under net 0 alone is another policy
    _, shared = _restatement(snap, inter, intras[0], stochastic, ps.CASES[k][5])
    assert torch.equal(shared[:, 0], intra[:, 0]) and not torch.equal(shared[:, 1:], intra[:, 1:])


def test_the_twin_decides_nine_rows_in_ten_for_every_net_the_gpu_tests_check():
    for n, (case, seed) in enumerate(ps.TWIN_NETS):
        inter, intras, _, _ = ps.make_nets(case, seed)
        for st in MODES:
            for draw in range(2):
                ref = ps.policy_ref(ps.synthetic_snapshot(case, 1000 + 10 * n + draw), inter, intras, st, SEED, case[5])
                assert ref.intra_safe.mean() >= 0.9, (case, st, ref.intra_safe.mean())


@pytest.mark.parametrize("slip", list(ps.SLIPS))
@pytest.mark.parametrize("stochastic", MODES)
@pytest.mark.parametrize("k", range(len(ps.CASES)), ids=ps.CASE_IDS)
def test_a_slipped_slice_to_net_mapping_is_caught(twins, k, stochastic, slip):
    snap, inter, intras, ref = twins[k, stochastic]
    S = ps.CASES[k][0]
    wrong = [intras[ps.SLIPS[slip](s, S)] for s in range(S)]
    scores, intra = _restatement(snap, inter, wrong, stochastic, ps.CASES[k][5])
    moved = [s for s in range(S) if ps.SLIPS[slip](s, S) != s]
    changed = ref.intra_safe[:, moved] & (intra.numpy()[:, moved] != ref.intra[:, moved])
    print(f"{ps.CASE_IDS[k]} {slip} stochastic={stochastic}: {changed.sum() / ref.intra_safe[:, moved].sum():.1%} of the decidable moved rows change")
    with pytest.raises(AssertionError, match="intra choices differ"):
        pr.check_actions(ref, scores, intra, min_safe=0.9)


def test_list_of_another_length_and_a_single_layer_list():
    from intent_radio_sched_multi_slice_amd.batched_env import per_slice_nets
    case = ps.CASES[0]
    snap = ps.synthetic_snapshot(case, 1)
    inter, intras, _, _ = ps.make_nets(case, 7)
    with pytest.raises(ValueError, match="one per slice"):
        _restatement(snap, inter, intras[:2], False, case[5])
    layers, _ = ps.layers_of(intras[0])
    assert per_slice_nets(layers) is None and per_slice_nets(intras[0]) is None and per_slice_nets(None) is None      # one net
    assert len(per_slice_nets(intras)) == 3 and len(per_slice_nets([layers] * 3)) == 3 and len(per_slice_nets(tuple(intras))) == 3
    a, b = _restatement(snap, inter, layers, False, case[5]), _restatement(snap, inter, [layers] * 3, False, case[5])
    assert torch.equal(a[1], b[1])


def test_one_net_or_a_list_of_nets_is_told_by_where_the_layer_pairs_sit():
    """per_slice_nets goes by the (W, b) pairs' place, not by the containers' types: a single net whose matrices are nested Python
    lists (policy_net_layers takes that form) is one net; a list of nets of two layers each -- entries of length 2, like a pair -- and
    a list of nets in nested lists are lists of nets."""
    from intent_radio_sched_multi_slice_amd.batched_env import per_slice_nets, policy_net_layers
    case = ps.CASES[0]
    snap = ps.synthetic_snapshot(case, 2)
    inter, intras, _, _ = ps.make_nets(case, 8)
    layers = [ps.layers_of(net)[0] for net in intras]
    assert all(len(net) == 2 for net in layers)                          # ([32]: two Linear layers)
    nested = [[[w.tolist(), b.tolist()] for w, b in net] for net in layers]
    arrays = [[(w.numpy(), b.numpy()) for w, b in net] for net in layers]
    for one in (nested[0], arrays[0], tuple(layers[0])):
        assert per_slice_nets(one) is None
        assert torch.equal(policy_net_layers(one)[0][0][0], layers[0][0][0])
    for many in (nested, arrays, layers, [tuple(net) for net in layers]):
        assert len(per_slice_nets(many)) == 3
    want = _restatement(snap, inter, intras, False, case[5])
    for many in (nested, arrays):
        assert torch.equal(_restatement(snap, inter, many, False, case[5])[1], want[1])
    assert torch.equal(_restatement(snap, inter, nested[0], False, case[5])[1], _restatement(snap, inter, intras[0], False, case[5])[1])


def _rllib_state(S, Us, widths, seed):
    """{policy_id: state dict} as a non-shared IBSched trainer's get_weights() (key names: adapters.rllib_fcnet_layers)"""
    rng = np.random.default_rng(seed)
    dims = [2 * Us + 9] + list(widths)
    out = {}
    for name in ["inter_slice_sched"] + [f"intra_slice_sched_{s}" for s in range(S)]:
        sd = {}
        for branch, head, n_out in (("_hidden_layers", "_logits", 3), ("_value_branch_separate", "_value_branch", 1)):
            for i in range(len(widths)):
                sd[f"internal_model.{branch}.{i}._model.0.weight"] = rng.standard_normal((dims[i + 1], dims[i])).astype(np.float32)
                sd[f"internal_model.{branch}.{i}._model.0.bias"] = rng.standard_normal(dims[i + 1]).astype(np.float32)
            sd[f"internal_model.{head}._model.0.weight"] = rng.standard_normal((n_out, dims[-1])).astype(np.float32)
            sd[f"internal_model.{head}._model.0.bias"] = rng.standard_normal(n_out).astype(np.float32)
        out[name] = sd
    return out


def test_rllib_per_slice_layers_keeps_slice_order_and_returns_the_value_branch():
    from intent_radio_sched_multi_slice_amd import adapters
    S, Us, widths = 4, 5, [16, 8]
    # (insertion order reversed: the reader must go by name, not by position)
    state = dict(reversed(list(_rllib_state(S, Us, widths, 3).items())))
    actors, critics = adapters.rllib_per_slice_layers(state, S)
    assert len(actors) == len(critics) == S
    for s in range(S):
        sd = state[f"intra_slice_sched_{s}"]
        assert [tuple(np.shape(w)) for w, _ in actors[s]] == [(16, 2 * Us + 9), (8, 16), (3, 8)]
        assert [tuple(np.shape(w)) for w, _ in critics[s]] == [(16, 2 * Us + 9), (8, 16), (1, 8)]
        assert np.array_equal(np.asarray(actors[s][0][0]), sd["internal_model._hidden_layers.0._model.0.weight"])
        assert np.array_equal(np.asarray(actors[s][-1][1]), sd["internal_model._logits._model.0.bias"])
        assert np.array_equal(np.asarray(critics[s][0][0]), sd["internal_model._value_branch_separate.0._model.0.weight"])
        assert np.array_equal(np.asarray(critics[s][-1][0]), sd["internal_model._value_branch._model.0.weight"])
    renamed = {k.replace("intra_slice_sched_", "agent_"): v for k, v in state.items()}
    assert len(adapters.rllib_per_slice_layers(renamed, S, policy_prefix="agent_")[0]) == S
    del state["intra_slice_sched_2"]
    with pytest.raises(KeyError, match="intra_slice_sched_2"):
        adapters.rllib_per_slice_layers(state, S)


def test_header_binding_and_library_agree_on_the_new_exports():
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.csrc import build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "ranenv.h")).read()
    declared = set(re.findall(r"\b(ranenv_[a-z_]+)\s*\(", header))
    for name in ("ranenv_set_intra_policy_networks", "ranenv_set_intra_value_networks"):
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
        proto = re.search(name + r"\(([^)]*)\)", header).group(1)
        assert [a.strip().split()[-1].lstrip("*") for a in proto.split(",")][:2] == ["h", "n"] and "const ranenv_mlp *const *" in proto
        assert len(_lib.FUNCTIONS[name][1]) == len(proto.split(",")) == 4
