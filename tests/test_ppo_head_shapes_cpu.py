"""The shape grid of the head policies' PPO update without a GPU (tests/ppo_head_shapes_ref.py): the health of the float64 twin on
every grid case and on the long record (no zero gradient tensor, clip fractions strictly inside (0.1, 0.9)), the LDS plan at its
edge, the rule that decides S10_sb3's source, planted slips against the yardstick on the grid, and the proof that an advantage pass
that stops at 256 rows would be seen on the long record."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import ppo_head_ref as hd
from tests import ppo_head_shapes_ref as hg
from tests import ppo_update_ref as ref
from tests.test_ppo_head_cpu import SLIP_HP, _slip_tensors

ONE = dict(epochs=1, minibatch=hd.ALL, lr=0.0, grad_clip=0.0)


@pytest.mark.parametrize("name", list(hg.CASES))
def test_no_gradient_tensor_of_the_twin_is_zero_on_the_grid(name):
    """ppo_head_ref.ratios' condition on the 96 synthetic rows of every grid case, and the clip fraction"""
    case, lay, rec = hg.CASES[name], hg.layers(name), hg.synthetic_record(name)
    t64 = hd.twin(case, rec, hd.row_order(1), lay, **ONE, **hd.HP)
    t32 = hd.twin(case, rec, hd.row_order(1), lay, dtype=torch.float32, **ONE, **hd.HP)
    r = hd.ratios(hd.tensors(t32["grad"]), hd.tensors(t64["grad"]), hd.tensors(t32["grad"]))      # (asserts: no twin tensor is zero)
    assert all(np.all(np.isfinite(x)) for x in hd.tensors(t64["grad"]).values())
    assert len(r) == 2 * (len(lay[0]) + len(lay[2])) + 1 and 0.1 < t64["clip_fracs"][0] < 0.9, t64["clip_fracs"]
    print(name, f"clip fraction {t64['clip_fracs'][0]:.3g}, float32 twin's worst relative error {max(v[2] for v in r.values()):.3g}")


def test_the_lds_plan_at_its_edge():
    """S16_edge needs 161 792 of the 163 840 bytes -- by the library and by the header's formula --, every other grid case less; the pair
    one step of 32 further is beyond the plan"""
    from intent_radio_sched_multi_slice_amd.batched_env import ppo_lds_bytes
    for name in hg.CASES:
        assert ppo_lds_bytes(*hg.dims(name)) == hg.lds_bytes(name) <= ref.LDS_MAX, name
    assert hg.lds_bytes("S16_edge") == hg.EDGE_LDS_BYTES == 161792 and ref.LDS_MAX == 163840
    assert all(hg.lds_bytes(name) < hg.EDGE_LDS_BYTES for name in hg.CASES if name != "S16_edge")
    S = 16
    assert ppo_lds_bytes([10 * S] + hg.PAST_EDGE + [S], [10 * S] + hg.PAST_EDGE + [1]) > ref.LDS_MAX


def test_the_ibsched_reward_exists_under_the_inter_source_alone():
    """Why S10_sb3 runs under observation "inter" and S10_sb3_head under "twc": the column "ibsched" cannot be selected under "head\""""
    from intent_radio_sched_multi_slice_amd.batched_env import head_reward_column
    with pytest.raises(ValueError):
        head_reward_column("head", "ibsched")
    for name, case in hg.CASES.items():
        assert head_reward_column(case[5], case[6]) >= 0, name
    assert hg.CASES["S10_sb3"][:5] == hg.CASES["S10_sb3_head"][:5] == (10, [64, 64], "tanh", [64, 64], "tanh")
    assert hd.ENV_SIZES[10] == "S10U100"


@pytest.mark.parametrize("name", list(hg.CASES))
def test_planted_slips_leave_the_bound_by_a_factor_above_1000_on_the_grid(name):
    """tests/test_ppo_head_cpu.py's slip test on the grid: each slip of ppo_head_ref.SLIPS in the float32 restatement puts some tensor's
    ratio to the yardstick above 1000 (the GPU file allows 8)"""
    case, lay, rec, order = hg.CASES[name], hg.layers(name), hg.synthetic_record(name), hd.row_order(1)
    t64 = _slip_tensors(hd.twin(case, rec, order, lay, **SLIP_HP))
    t32 = _slip_tensors(hd.twin(case, rec, order, lay, dtype=torch.float32, **SLIP_HP))
    for slip in hd.SLIPS:
        got = _slip_tensors(hd.twin(case, rec, order, lay, dtype=torch.float32, slip=slip, **SLIP_HP))
        k, worst = max(((k, v[0]) for k, v in hd.ratios(got, t64, t32).items()), key=lambda kv: kv[1])
        print(f"{name} {slip}: worst ratio {worst:.3g} at {k}")
        assert worst > 1000.0, f"{name}: the slip {slip} stays within {worst:.3g} x the yardstick (worst tensor {k})"


def test_the_long_record():
    """288 synthetic rows at the base case.  As one minibatch under adv_norm: no zero tensor, the clip fraction inside (0.1, 0.9).  In
    minibatches of 257 and 31 rows over two epochs: every one's clip fraction inside.  And an advantage pass that stops after its first
    stride -- mean and deviation over the minibatch's first 256 entries -- puts the gradient > 1000 x the yardstick away."""
    rec, lay = hd.synthetic_record("base", T=hg.T_LONG), hd.layers("base")
    assert rec["logp"].numel() == hg.N_LONG == 288 > 256
    order = hd.row_order(1, n=hg.N_LONG)
    assert torch.equal(torch.sort(order[0]).values, torch.arange(hg.N_LONG, dtype=torch.int32))
    t64, t32 = hd.twin("base", rec, order, lay, **ONE, **hd.HP), hd.twin("base", rec, order, lay, dtype=torch.float32, **ONE, **hd.HP)
    g64, g32 = hd.tensors(t64["grad"]), hd.tensors(t32["grad"])
    hd.ratios(g32, g64, g32)
    assert 0.1 < t64["clip_fracs"][0] < 0.9
    two = hd.row_order(2, n=hg.N_LONG)
    assert [(ep, nb) for ep, _, nb in hg.long_chunks(two)] == [(0, 257), (0, 31), (1, 257), (1, 31)]
    t = hd.twin("base", rec, two, lay, epochs=2, minibatch=hg.LONG_MINIBATCH, lr=3e-4, grad_clip=0.5, **hd.HP)
    assert len(t["clip_fracs"]) == 4 and all(0.1 < f < 0.9 for f in t["clip_fracs"]), t["clip_fracs"]
    # the first stride's statistics in place of the minibatch's
    adv = rec["adv"].reshape(-1).double()
    first = adv[order[0, :256].long()]
    short = dict(rec, adv=((adv - first.mean()) / (first.std() + 1e-8)).reshape(rec["adv"].shape))
    bad = hd.tensors(hd.twin("base", short, order, lay, **ONE, **dict(hd.HP, adv_norm=False))["grad"])
    full = dict(rec, adv=((adv - adv.mean()) / (adv.std() + 1e-8)).reshape(rec["adv"].shape))
    same = hd.tensors(hd.twin("base", full, order, lay, **ONE, **dict(hd.HP, adv_norm=False))["grad"])
    ok = {k: v for k, v in hd.ratios(same, g64, g32).items() if k.startswith("actor") or k == "log_std"}
    assert max(v[0] for v in ok.values()) <= 1.0, ok      # (the restatement by hand is the twin's own normalisation)
    off = {k: v for k, v in hd.ratios(bad, g64, g32).items() if k.startswith("actor") or k == "log_std"}
    print("advantage statistics of the first 256 rows: " + ", ".join(f"{k} {v[0]:.3g}" for k, v in off.items()))
    assert max(v[0] for v in off.values()) > 1000.0, off
