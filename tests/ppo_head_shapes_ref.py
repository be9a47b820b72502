"""The shape grid of the head policies' PPO update (ranenv_ppo_update_kernel_head), stated once; tests/test_ppo_head_shapes_cpu.py and
tests/test_gpu_ppo_head_shapes.py run on it.  Built on tests/ppo_head_ref.py (nets, records, the noise on logp, the twin, the packed
layout, the yardstick), whose four cases have seen S 1, 3, 5 and 16, widths up to 160, critics of two hidden layers and 96 rows.

What the grid reaches that those cases do not:

    S10_sb3          the native workload S10U100 under SB3's default [64, 64] tanh pair, as examples/train_sb3_ppo_on_device.py --agent
                     ibsched trains it: the "ibsched" reward, which exists under observation "inter" alone
    S10_sb3_head     the same nets under observation "head" with the "twc" reward (the reward "ibsched" cannot be selected there:
                     batched_env.head_reward_column raises), so that S 10 runs under both sources
    S16_edge         [512, 448] on both sides: 161 792 of the plan's 163 840 bytes of LDS ([512, 480] is refused)
    S8_deep_critic   a critic of four hidden layers, a 7-wide bottleneck under ReLU; S 8: log_std's own gradient loop at 8 positions
    S6_deep_actor    an actor of four hidden layers; S 6

and, at ppo_head_ref's ``base`` case, a record of B 12 x T_LONG 24 = 288 rows: one minibatch of all of them (nine tiles; the advantage
passes ``for (k = tid; k < nb; k += 256)`` take a second stride) and minibatches of 257 and 31 rows.

THE CONDITIONS tests/test_ppo_head_shapes_cpu.py holds on the grid's inputs (nets of ppo_head_ref.head_nets at NET_SEED, the synthetic
record of ppo_head_ref.synthetic_record): no gradient tensor of the float64 twin is zero (ppo_head_ref.ratios asserts it) and the
twin's clip fraction lies strictly inside (0.1, 0.9) -- on the 96 rows of every grid case, on the long record's 288 rows as one
minibatch and on each of its minibatches of 257 and 31 rows.  The GPU tests hold the device's clip fractions to the same interval on
the real records.
"""
from __future__ import annotations

from tests import ppo_head_ref as hd
from tests import ppo_update_ref as ref

# name -> (S, actor widths, actor activation, critic widths, critic activation, observation, reward), ppo_head_ref.CASES' form
CASES = {"S10_sb3": (10, [64, 64], "tanh", [64, 64], "tanh", "inter", "ibsched"),
         "S10_sb3_head": (10, [64, 64], "tanh", [64, 64], "tanh", "head", "twc"),
         "S16_edge": (16, [512, 448], "tanh", [512, 448], "relu", "head", "colran"),
         "S8_deep_critic": (8, [255], "tanh", [100, 7, 255, 32], "relu", "head", "twc"),
         "S6_deep_actor": (6, [64, 7, 255, 33], "relu", [33], "tanh", "head", "twc")}
# the nets' seed per case: tests/test_ppo_head_shapes_cpu.py guards that no gradient tensor of the twin is zero with it
NET_SEED = {c: 61 for c in CASES}
EDGE_LDS_BYTES = 161792                  # S16_edge: 4096 + 128 * (ld(160) + ld(512) + ld(448) + ld(32))
PAST_EDGE = [512, 480]                   # ... and the pair one step of 32 further: refused
T_LONG, N_LONG, LONG_MINIBATCH = hd.T_LONG, hd.N_LONG, hd.LONG_MINIBATCH


def dims(name):
    """(actor widths [in, hidden..., out], critic widths) of a grid case"""
    S, aw, _, cw, _ = CASES[name][:5]
    return [10 * S] + aw + [S], [10 * S] + cw + [1]


def lds_bytes(name):
    """The plan's figure by its formula, 4096 + 128 x the larger net's strides (widths padded to 32)"""
    return 4096 + 128 * max(sum(ref.net_ld(ref.pad32(w)) for w in d) for d in dims(name))


def layers(name):
    return hd.layers(CASES[name], NET_SEED[name])


def synthetic_record(name):
    return hd.synthetic_record(CASES[name], net_seed=NET_SEED[name])


def make_env(name, **kw):
    """ppo_head_ref.make_env on a grid case: (env, (actor layers, log_std, critic layers))"""
    return hd.make_env(CASES[name], net_seed=NET_SEED[name], **kw)


def long_chunks(order):
    """The minibatches of a call of minibatch LONG_MINIBATCH on the long record: [(epoch, first entry, entries)]"""
    return [(ep, c0, min(LONG_MINIBATCH, order.shape[1] - c0)) for ep in range(order.shape[0]) for c0 in range(0, order.shape[1], LONG_MINIBATCH)]
