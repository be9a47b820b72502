"""The SPREAD form of the head binding (ranenv_ppo_bind_head_spread; the kernels ranenv_ppo_spread_head_pass / _reduce / _apply) across
the shape grid of tests/ppo_head_shapes_ref.py (``hg``) -- what tests/test_gpu_ppo_head_spread.py runs at several slabs on its ``base``
case alone: every grid case (S 6 / 8 / 10 / 16, deep actors and critics, a 7-wide bottleneck, the edge of the LDS plan) at 3 slabs
against the float64 twin and through one Adam step; all 256 slabs on nine tiles; and the reduce held to the byte.

Records, nets, tolerances and comparison functions are tests/ppo_head_ref.py's (``hd``) and tests/ppo_bindings_shapes_ref.py's (``bs``):
the gradient per tensor -- ``log_std`` a tensor of its own -- within 8 x the float32 twin's error of the float64 twin (floor 1e-6),
statistics 1e-6, Adam 4 ulp of ref.adam_step_f32 on the call's own dev_grad, the norm 1e-9, byte equality between schedules.

Measured on one MI355X (printed by the tests):
    3 slabs, worst tensor's error / float32 twin's (bound 8): S10_sb3 0.239, S10_sb3_head 0.864, S16_edge 0.779, S8_deep_critic 0.976,
    S6_deep_actor 2.01; the five statistics within 2.2e-7 of the twin (bound 1e-6); clip fraction 0.427 in every case
    one Adam step at 3 slabs (weights and log_std / moments): 0 / 0 ulp in all five cases
    exact reduce: the weight part 0 ulp on all 10 432 floats (the descending restatement differs in 1203), the log_std tail 1 ulp"""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import ppo_bindings_shapes_ref as bs
from tests import ppo_head_ref as hd
from tests import ppo_head_shapes_ref as hg
from tests import ppo_spread_ref as sp
from tests.gpu_common import _ordered

pytestmark = pytest.mark.gpu

ONE = dict(epochs=1, minibatch=hd.ALL, lr=0.0, grad_clip=None, clip=0.2, vf_coeff=0.5, ent_coeff=0.01)      # one minibatch, weights unchanged
STAT_NAMES = ("policy_loss", "value_loss", "entropy", "kl", "clip_frac")


@pytest.mark.parametrize("case", bs.HEAD_CASES)
def test_three_slabs_against_the_float64_twin(case):
    """The 96 rows (three tiles, one per slab) in one minibatch at lr 0 under adv_norm: dev_grad per tensor within 8 x the float32
    twin's error, the statistics within 1e-6, the clip fraction strictly inside (0.1, 0.9)"""
    env, lay, rec = bs.head_env(case, 3)
    order = hd.row_order(1)
    out = env.ppo_update_head(rec, order=bs.to_dev(order, env), grad=True, **ONE)
    worst, misses = hd.check_head_against_twin(hg.CASES[case], rec, order, out, lay, f"head spread {case}, 3 slabs")
    assert not misses, misses
    assert 0.0 < worst <= hd.FACTOR
    assert out["rows"][0] == hd.N and 0.1 < out["clip_frac"][0] < 0.9, out["clip_frac"][0]
    env.close()


@pytest.mark.parametrize("case", bs.HEAD_CASES)
def test_one_adam_step_at_three_slabs(case):
    """One minibatch of the 96 rows with lr > 0 from zero moments at 3 slabs: weights, log_std, m and v within 4 ulp of
    ref.adam_step_f32 on the call's own dev_grad (bs.check_head_adam_step)"""
    env, lay, rec = bs.head_env(case, 3)
    S = hg.CASES[case][0]
    out = env.ppo_update_head(rec, order=bs.to_dev(hd.row_order(1), env), grad=True, eps=1e-5, **dict(ONE, lr=1e-3, grad_clip=0.05))
    bs.check_head_adam_step(env, lay, out, S, f"head spread {case}, 3 slabs", 1e-3, 0.05, 1e-5)
    env.close()


def test_256_slabs_on_nine_tiles_give_the_bytes_of_nine_slabs():
    """The 288-row ``base`` record in one minibatch at lr 0: slabs=256 runs a grid of min(9, 256) = 9, so dev_grad and every statistic
    equal those under slabs=9 byte for byte"""
    env, lay, rec = bs.head_env("base", 9, T=hd.T_LONG)
    assert rec["logp"].numel() == hd.N_LONG and sp.plan(hd.N_LONG, hd.ALL, 1, sp.SLABS_MAX) == (1, 9, 9) == sp.plan(hd.N_LONG, hd.ALL, 1, 9)
    order = hd.row_order(1, n=hd.N_LONG)
    outs = {}
    for slabs in (9, sp.SLABS_MAX):
        bs.head_bind(env, slabs)
        outs[slabs] = env.ppo_update_head(rec, order=bs.to_dev(order, env), grad=True, **ONE)
    a, b = outs[9], outs[sp.SLABS_MAX]
    assert a["grad"].cpu().numpy().any() and a["grad"].cpu().numpy().tobytes() == b["grad"].cpu().numpy().tobytes(), "9 and 256 slabs differ on nine tiles"
    for name in STAT_NAMES + ("grad_norm", "rows", "minibatches"):
        assert np.asarray(a[name]).tobytes() == np.asarray(b[name]).tobytes(), name
    assert a["rows"][0] == hd.N_LONG
    env.close()


def test_the_reduce_adds_the_slabs_in_ascending_order_to_the_byte():
    """128 rows of the ``base`` record at 4 slabs (one tile per slab), lr 0, advantages as given.  A twin handle under the plain head
    binding runs one call per slab on that slab's 32 rows: its dev_grad g_w carries the row weight 1 / 32, the spread call's 1 / 128, an
    exact factor 4.  The weight part of the spread dev_grad is ((g_0 / 4 + g_1 / 4) + g_2 / 4) + g_3 / 4 in float32, byte for byte, and
    not the descending sum.  The ``log_std`` tail is held to 1 ulp, not to the byte: the spread reduce adds the slabs' UNROUNDED float64
    partials in ascending order and rounds once (the kernel's header), whereas the plain kernel hands back each slab's partial already
    rounded to float32 -- the restatement adds those four in float64 in ascending order and rounds once, so it differs from the
    device by the four roundings of its inputs."""
    rows, slabs = 128, bs.EXACT_SLABS
    env_s, rec_s, env_p, rec_p, lay = bs.head_twins("base", slabs, None, T=hd.T_LONG)
    S = hd.CASES["base"][0]
    full = hd.row_order(1, n=hd.N_LONG)[:, :rows].contiguous()
    hp = dict(ONE, adv_norm=None)
    out = env_s.ppo_update_head(rec_s, order=bs.to_dev(full, env_s), grad=True, **hp)
    assert [len(t) for t in sp.walk(rows, slabs)] == [1] * slabs and out["rows"][0] == rows
    parts = []
    for share in bs.slab_rows(full[0].numpy(), rows, slabs):
        one = torch.as_tensor(share[None, :], dtype=torch.int32)
        parts.append(env_p.ppo_update_head(rec_p, order=bs.to_dev(one, env_p), grad=True, **hp)["grad"].cpu().numpy().copy())
    got = out["grad"].cpu().numpy()
    want, other = bs.reduce_f32([p[:-S] for p in parts], slabs), bs.reduce_f32([p[:-S] for p in parts], slabs, "descending")
    d = np.abs(_ordered(got[:-S]) - _ordered(want))
    tail = np.zeros(S, dtype=np.float64)
    for p in parts:
        tail = tail + p[-S:].astype(np.float64) / slabs
    d_tail = np.abs(_ordered(got[-S:]) - _ordered(tail.astype(np.float32)))
    print(f"head exact reduce: weights, worst ulp distance to the ascending restatement {int(d.max())}, {int((d != 0).sum())} of {d.size} differ; "
          f"the descending one differs in {int((want != other).sum())}; log_std tail, worst ulp distance {int(d_tail.max())}")
    assert got[:-S].any() and got[-S:].all()
    assert got[:-S].tobytes() == want.tobytes(), "the weight part of dev_grad is not the slabs' ascending float32 sum"
    assert want.tobytes() != other.tobytes(), "ascending and descending order give the same bytes: the equality compares nothing"
    assert d_tail.max() <= 1
    env_s.close()
    env_p.close()
