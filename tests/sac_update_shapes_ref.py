"""The shape grid of the SAC update (ranenv_sac.hip), stated once; tests/test_sac_update_shapes_cpu.py and
tests/test_gpu_sac_update_shapes.py run on it.  Built on tests/sac_update_ref.py (the nets' recipe, the synthetic rows, the twin, the
packed layout, the yardstick), whose four cases have seen S 1, 5, 6 and 16, widths up to 160, three hidden layers and three tiles.

What the grid reaches that those cases do not:

    S3_96x160_33    the action columns 30..32 across the 32-column boundary of the observation (sac_input_grad's blocks {1, 2}); the
                    actor owns the LDS plan
    S8_255_511x3    action columns 80..87: they start on a 16-column block's edge and end inside it; odd wide widths, a 3-wide bottleneck
                    (a 1-wide one under ReLU is dead: both critics constant, every row a tie)
    S10_sb3         the native workload S10U100 under SB3's default [256, 256] ReLU; columns 100..109
    S16_edge        [512, 448] on both sides: 162 816 of the plan's 163 840 bytes of LDS ([512, 480] is refused)
    S16_deep        five layers on both sides (NET_MAX_LAYERS): dQ/da carried back through all of them

and, at sac_update_ref's ``base`` case: tile walks of five tiles in which the workgroups walk unequal numbers of tiles and the last tile
has one row (TILE_ROWS under TILE_SLABS), and the high words of the Philox counter and key (PHILOX: a ``first_row`` beyond 2^32, a
seed beyond 2^32).

THE CONDITIONS tests/test_sac_update_shapes_cpu.py holds on the grid's synthetic inputs (nets of sac_update_ref.nets at NET_SEED 31, rows
of sac_update_ref.synthetic_batch at BATCH_SEED 5), on all 96 rows and on the first 65 and 33:
  - no gradient tensor of the float64 twin is zero (sac_update_ref.grad_ratios asserts it);
  - each critic is the smaller one on at least 25 % of the rows;
  - at least one log_std value lies below -20, at least one above 2, and at least half of them lie inside (FREE_SHARE; at S 3 the
    recipe leaves one free position of three -- 0 at the lower clamp, 1 above the upper one, 2 free --, so 0.3 there);
  - no row lies near a tie of the critics, by ``tie_margin``: the smallest |Q1 - Q2| over the rows is at least TIE_MARGIN = 1000 x the
    largest |Q_float32 - Q_float64| over the rows and both critics, Q evaluated on [obs | a32] by torch in both dtypes.
    sac_update_ref.conditions' "separated" cannot be the condition here: it uses sac_ref's rigorous float32 bound, which holds for ANY
    float32 evaluation and at the wide nets is about as large as |Q| itself (6 of 96 rows of S10_sb3 lie inside it, 62 and 67 of S16_edge
    and S16_deep).  The device is allowed 8 x the float32 twin's error everywhere else: a margin of 1000 leaves two orders of magnitude
    over that.
The GPU tests rely on these for the synthetic rows and compute ``tie_margin`` themselves, from the device's own nets, on the rows they
sample from the ring (SAMPLE_SEED; a seed whose rows miss the margin is replaced here, never skipped).
"""
from __future__ import annotations

import numpy as np
import torch

from tests import ppo_update_ref as pu
from tests import sac_update_ref as su

# name -> (S, actor widths, actor activation, critic widths, critic activation), sac_update_ref.CASES' form
CASES = {"S3_96x160_33": (3, [96, 160], "relu", [33], "tanh"),
         "S8_255_511x3": (8, [255], "tanh", [511, 3], "relu"),
         "S10_sb3": (10, [256, 256], "relu", [256, 256], "relu"),
         "S16_edge": (16, [512, 448], "relu", [512, 448], "tanh"),
         "S16_deep": (16, [64] * 4, "relu", [100, 7, 255, 32], "tanh")}
EDGE_LDS_BYTES = 162816                  # S16_edge: 5120 + 128 * (ld(192) + ld(512) + ld(448) + ld(32))
PAST_EDGE = [512, 480]                   # ... and the pair one step of 32 further: refused
TIE_MARGIN = 1000.0
FREE_SHARE = {3: 0.3}                    # (default 0.5)
SAMPLE_SEED = {c: 9 for c in CASES}      # replay_sample's seed per case (draw 1) of the GPU tests' ring rows: tie_margin holds on them
# The tile walks at ``base``: rows of a minibatch, slab counts.  129 rows = five tiles whose last has one row; under 2 slabs workgroup 0
# walks tiles 0, 2, 4 and workgroup 1 tiles 1, 3; under 3 slabs 2 + 2 + 1; TILE_EXACT slabs = one tile per workgroup.
TILE_ROWS, TILE_SLABS, TILE_EXACT = (129, 160), (1, 2, 3, 32), 5
TILE_SAMPLE_SEED = 12                    # (under seeds 9 and 11 one of the 160 rows lies inside sac_ref's bound: gap / bound 0.75; under 12: 5.3)
# The Philox words at ``base``: every high word set
PHILOX = dict(seed=(5 << 32) | 9, draw=4, first_row=(1 << 32) + 7)
PHILOX_SAMPLE_SEED = 11                  # (under these draws the rows of sample seed 9 come within 815 x the float32 error of a tie; 11: 5.4e3)
LOW32 = 0xFFFFFFFF


def lds_bytes(name):
    """The plan's figure for the grid case ``name`` by its formula, 5120 + 128 x the larger net's strides (widths padded to 32)"""
    S, aw, _, qw, _ = CASES[name]
    need = lambda dims: 128 * sum(pu.net_ld(pu.pad32(w)) for w in dims)  # noqa: E731
    return 5120 + max(need([10 * S] + aw + [2 * S]), need([11 * S] + qw + [1]))


def tie_margin(case, batch, nets_, seed=su.SEED, draw=su.DRAW, first_row=0):
    """(min over the rows of |Q1 - Q2|) / (max over the rows and both critics of |Q_float32 - Q_float64|) on [obs | a32] under the actor
    pass's own actions (``sac_actor_noise`` at the rows' global indices) -- ``nets_`` = (actor, q1, q2, ...) layer lists; the critics
    are the live ones.  Returns (the ratio, the gap, the float32 error)."""
    from intent_radio_sched_multi_slice_amd.adapters import sac_actor_noise
    S, _, aact, _, qact = su.spec(case)
    actor, q1, q2 = pu.as_sequential(nets_[0], aact), pu.as_sequential(nets_[1], qact), pu.as_sequential(nets_[2], qact)
    with torch.no_grad():
        obs = torch.as_tensor(batch["obs"]).detach().cpu().to(torch.float32)
        n = obs.shape[0]
        out = actor(obs).double()
        z = torch.from_numpy(sac_actor_noise(n, S, seed, draw, first_row))
        a32 = torch.tanh(out[:, :S] + torch.exp(out[:, S:].clamp(-20.0, 2.0)) * z).float()
        x = torch.cat([obs, a32], dim=1)
        v32 = torch.cat([q1(x), q2(x)], dim=1).double()
        v64 = torch.cat([q1.double()(x.double()), q2.double()(x.double())], dim=1)
    gap, err = float((v64[:, 0] - v64[:, 1]).abs().min()), float((v32 - v64).abs().max())
    return gap / err, gap, err


def census(case, batch, nets_, lec=None, seed=su.SEED, draw=su.DRAW, first_row=0):
    """The shares the inputs are held to: the rows on which each critic is the smaller one (float64, on [obs | a32] as ``tie_margin``
    takes them) and the clamp census of the actor's log_std over rows x positions"""
    from intent_radio_sched_multi_slice_amd.adapters import sac_actor_noise
    S, _, aact, _, qact = su.spec(case)
    actor, q1, q2 = pu.as_sequential(nets_[0], aact), pu.as_sequential(nets_[1], qact).double(), pu.as_sequential(nets_[2], qact).double()
    with torch.no_grad():
        obs = torch.as_tensor(batch["obs"]).detach().cpu().to(torch.float32)
        out = actor(obs).double()
        raw = out[:, S:]
        z = torch.from_numpy(sac_actor_noise(obs.shape[0], S, seed, draw, first_row))
        a32 = torch.tanh(out[:, :S] + torch.exp(raw.clamp(-20.0, 2.0)) * z).float()
        x = torch.cat([obs, a32], dim=1).double()
        v1, v2 = q1(x)[:, 0], q2(x)[:, 0]
    return {"q1_smaller": float((v1 < v2).double().mean()), "q2_smaller": float((v2 < v1).double().mean()),
            "clamped_low": int((raw < -20.0).sum()), "clamped_high": int((raw > 2.0).sum()),
            "free": float(((raw >= -20.0) & (raw <= 2.0)).double().mean())}


def check_census(case, got):
    S = su.spec(case)[0]
    assert got["q1_smaller"] >= 0.25 and got["q2_smaller"] >= 0.25, got
    assert got["clamped_low"] >= 1 and got["clamped_high"] >= 1 and got["free"] >= FREE_SHARE.get(S, 0.5), got


def target_ratio(dev, t64, t32):
    """dev_target under the yardstick: (e_dev / max(e_32, FLOOR), e_dev, e_32), relative in the 2-norm against the float64 twin's y"""
    x64, x32, xd = (np.asarray(x, dtype=np.float64) for x in (t64, t32, dev))
    n64 = np.linalg.norm(x64)
    assert n64 > 0.0 and xd.shape == x64.shape
    e_dev, e_32 = np.linalg.norm(xd - x64) / n64, np.linalg.norm(x32 - x64) / n64
    return e_dev / max(e_32, su.FLOOR), e_dev, e_32


# ---- the GPU side -------------------------------------------------------------------------------------------------------------------
def five(nets):
    """(actor, q1, q2, q1_target, q2_target) layer lists of a ``device_nets`` dict"""
    return tuple(nets[k] for k in ("actor", "q1", "q2", "q1_target", "q2_target"))


def stat_names():
    from intent_radio_sched_multi_slice_amd import _lib
    return _lib.SAC_STATS


def step_against_twin(case, env, batch, n, lr, what, names=su.TENSORS + ("log_ent_coef",), stats=True, target=False, **step):
    """One step on the first n rows from the nets as they are on the device now: dev_grad (its padding exact zeros: unpack_grad) and the
    statistics against the twins under sac_update_ref's yardstick; ``target``: dev_target against the twins' y as well.  ``step``:
    seed / draw / first_row in place of sac_update_ref's.  Returns (the worst gradient ratio, the call's output, the starting nets)."""
    kw = dict(gamma=su.GAMMA, tau=su.TAU, seed=su.SEED, draw=su.DRAW)
    kw.update(step)
    start = five(su.device_nets(env))
    lec = float(env.sac_log_ent_coef().cpu()[0])
    out = env.sac_update(su.head(batch, n), 1, minibatch=n, lr=lr, grad=True, target=target, **kw)
    dev = su.unpack_grad(out["grad"].cpu().numpy(), start[0], start[1])
    tw = dict(steps=1, minibatch=n, lr=lr, **{k: v for k, v in kw.items() if k in ("seed", "draw", "first_row")})
    t64, t32 = su.twin(case, su.head(batch, n), start, lec, **tw), su.twin(case, su.head(batch, n), start, lec, torch.float32, **tw)
    worst = su.check_grads(dev, t64["grad"], t32["grad"], what, names)
    if stats:
        su.check_stats([out[k][0] for k in stat_names()], t64["stats"][0], t32["stats"][0], what)
    if target:
        ratio, e, e32 = target_ratio(out["target"].cpu().numpy(), t64["target"].numpy(), t32["target"].numpy())
        print(f"{what}: dev_target, device / float32 torch yardstick: {ratio:.3g}")
        assert ratio <= su.FACTOR, f"{what}: dev_target: device {e:.3g}, float32 torch {e32:.3g}"
    return worst, out, start
