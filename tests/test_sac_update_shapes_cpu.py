"""The shape grid of the SAC update without a GPU (tests/sac_update_shapes_ref.py): the conditions its synthetic inputs must meet -- the
GPU tests rely on them --, the LDS plan at its edge, the twin's planted slips against the yardstick on every grid case, and the proof
that a truncated Philox word would be seen at the values the GPU test passes."""
import numpy as np
import pytest
import torch

from intent_radio_sched_multi_slice_amd import adapters
from tests import ppo_update_ref as pu
from tests import sac_update_ref as su
from tests import sac_update_shapes_ref as sg
from tests.test_sac_update_cpu import GRAD_SLIPS, SLIP_CASES as BASE_SLIP_CASES

LEC = float(np.float32(np.log(su.ENT_INIT)))
_SHARED = {}


def shared(name):
    """The case's synthetic batch, nets and the twins of one step at lr 0 on all ROWS rows (computed once, never modified)."""
    if name not in _SHARED:
        case = sg.CASES[name]
        batch = su.synthetic_batch(case)
        actor, q1, q2 = su.case_layers(case)
        nets_ = (actor, q1, q2, q1, q2)
        kw = dict(steps=1, minibatch=su.ROWS, lr=0.0)
        _SHARED[name] = dict(case=case, batch=batch, nets=nets_, t64=su.twin(case, batch, nets_, LEC, **kw), t32=su.twin(case, batch, nets_, LEC, torch.float32, **kw))
    return _SHARED[name]


@pytest.mark.parametrize("name", list(sg.CASES))
def test_conditions_on_the_grid_inputs(name):
    c = shared(name)
    for n in (su.ROWS, 65, 33):
        rows = su.head(c["batch"], n)
        got = sg.census(c["case"], rows, c["nets"])
        ratio, gap, err = sg.tie_margin(c["case"], rows, c["nets"])
        print(name, n, got, f"tie margin {ratio:.3g} (smallest |Q1 - Q2| {gap:.3g}, largest float32 error of a Q {err:.3g})")
        sg.check_census(c["case"], got)
        assert ratio >= sg.TIE_MARGIN, (name, n, ratio, gap, err)
    su.grad_ratios(c["t64"]["grad"], c["t64"]["grad"], c["t32"]["grad"])      # (asserts: no twin gradient tensor is zero)


def test_the_lds_plan_at_its_edge():
    """S16_edge needs 162 816 of the 163 840 bytes -- by the library and by the header's formula --, every other grid case less; the pair
    one step of 32 further is beyond the plan"""
    from intent_radio_sched_multi_slice_amd.batched_env import sac_lds_bytes
    dims = lambda S, aw, qw: ([10 * S] + aw + [2 * S], [11 * S] + qw + [1])  # noqa: E731
    for name, (S, aw, _, qw, _) in sg.CASES.items():
        assert sac_lds_bytes(*dims(S, aw, qw)) == sg.lds_bytes(name) <= pu.LDS_MAX, name
    assert sg.lds_bytes("S16_edge") == sg.EDGE_LDS_BYTES == 162816 and pu.LDS_MAX == 163840
    assert all(sg.lds_bytes(name) < sg.EDGE_LDS_BYTES for name in sg.CASES if name != "S16_edge")
    assert sac_lds_bytes(*dims(16, sg.PAST_EDGE, sg.PAST_EDGE)) > pu.LDS_MAX
    # the actor owns the plan at S3_96x160_33, the critic at S8_255_511x3
    S, aw, _, qw, _ = sg.CASES["S3_96x160_33"]
    assert sac_lds_bytes(*dims(S, aw, qw)) > sac_lds_bytes(*dims(S, [32], qw))
    S, aw, _, qw, _ = sg.CASES["S8_255_511x3"]
    assert sac_lds_bytes(*dims(S, aw, qw)) > sac_lds_bytes(*dims(S, aw, [32]))


def test_the_action_columns_fall_where_the_grid_says():
    """sac_input_grad's 16-column blocks of layer 0, [10 S >> 4, (11 S + 15) >> 4): the sets the grid adds to {0}, {3}, {3, 4}, {10}"""
    blocks = lambda S: list(range((10 * S) >> 4, (11 * S + 15) >> 4))  # noqa: E731
    assert [blocks(su.CASES[c][0]) for c in ("deg", "base", "stride", "two_pair")] == [[0], [3], [3, 4], [10]]
    assert blocks(3) == [1, 2] and 10 * 3 < 32 <= 11 * 3 - 1      # columns 30..32: the last one lies behind the first 32 columns
    assert blocks(8) == [5] and (10 * 8) % 16 == 0 and (11 * 8) % 16 != 0
    assert blocks(10) == [6] and blocks(16) == [10]


# (at S 16 the action columns start at 160 = pad32(160): that slip changes nothing there -- test_sac_update_cpu.SLIP_CASES' rule)
SLIP_CASES = [(c, s) for c in sg.CASES for s in sorted(GRAD_SLIPS)
              if not (s == "action_columns_pad32" and pu.pad32(10 * sg.CASES[c][0]) == 10 * sg.CASES[c][0])]


def test_the_slip_rule_is_the_base_files():
    assert ("two_pair", "action_columns_pad32") not in BASE_SLIP_CASES and ("base", "action_columns_pad32") in BASE_SLIP_CASES
    assert len(SLIP_CASES) == 5 * len(GRAD_SLIPS) - 2 and ("S10_sb3", "action_columns_pad32") in SLIP_CASES


@pytest.mark.parametrize("name,slip", SLIP_CASES)
def test_planted_gradient_slips_leave_the_yardstick_on_the_grid(name, slip):
    """Each slip, planted into the float64 twin, puts its worst gradient tensor at least 1000 x the yardstick away"""
    c = shared(name)
    bad = su.twin(c["case"], c["batch"], c["nets"], LEC, steps=1, minibatch=su.ROWS, lr=0.0, slip=slip)
    ratios = su.grad_ratios(bad["grad"], c["t64"]["grad"], c["t32"]["grad"], GRAD_SLIPS[slip])
    worst = max(r[0] for r in ratios.values())
    print(name, slip, f"worst ratio {worst:.3g}")
    assert worst >= 1000.0 * su.FACTOR, (name, slip, worst)


def test_a_truncated_philox_word_would_be_seen():
    """The values the GPU test passes (sg.PHILOX) against the same with the seed, first_row or both cut to their low 32 bits: the actor
    pass's and the target's draws differ in every row; and the twin's gradients and targets move by far more than the yardstick."""
    S, n = su.CASES["base"][0], su.ROWS
    seed, draw, first = sg.PHILOX["seed"], sg.PHILOX["draw"], sg.PHILOX["first_row"]
    assert seed >> 32 and first >> 32 and 0 <= draw < 2 ** 32
    target_noise = lambda sd, fr: adapters._sac_noise(n, S, sd, draw, fr, adapters.SAC_TAG)  # noqa: E731
    full_a, full_t = adapters.sac_actor_noise(n, S, seed, draw, first), target_noise(seed, first)
    for sd, fr in ((seed & sg.LOW32, first), (seed, first & sg.LOW32), (seed & sg.LOW32, first & sg.LOW32)):
        assert (adapters.sac_actor_noise(n, S, sd, draw, fr) != full_a).any(axis=1).all(), (sd, fr)
        assert (target_noise(sd, fr) != full_t).any(axis=1).all(), (sd, fr)
    batch = su.synthetic_batch("base")
    actor, q1, q2 = su.case_layers("base")
    nets_ = (actor, q1, q2, q1, q2)
    kw = dict(steps=1, minibatch=n, lr=0.0, draw=draw)
    t64 = su.twin("base", batch, nets_, LEC, seed=seed, first_row=first, **kw)
    t32 = su.twin("base", batch, nets_, LEC, torch.float32, seed=seed, first_row=first, **kw)
    for sd, fr in ((seed & sg.LOW32, first), (seed, first & sg.LOW32)):
        cut = su.twin("base", batch, nets_, LEC, seed=sd, first_row=fr, **kw)
        worst = max(r[0] for r in su.grad_ratios(cut["grad"], t64["grad"], t32["grad"], ("actor", "log_ent_coef")).values())
        tgt = sg.target_ratio(cut["target"].numpy(), t64["target"].numpy(), t32["target"].numpy())[0]
        print(f"seed {sd:#x} first_row {fr:#x}: actor / coefficient gradient {worst:.3g}, target {tgt:.3g} x the yardstick")
        assert worst >= 1000.0 * su.FACTOR and tgt >= 1000.0 * su.FACTOR
