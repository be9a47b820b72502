"""numpy restatement of the serving order of member lines (include/ranenv.h, "MEMBER LINES": ranenv_member_serving_order): which
slot -- pass slot // 8, cluster slot % 8 -- serves each of a wave's 64 lanes, and how many passes keep the masked sum."""
import numpy as np


def bits(mask):
    return np.array([(int(mask) >> l) & 1 for l in range(64)], dtype=bool)


def serving_order(member_mask, holder_mask, nl, dq):
    """-> (slots [64], masked_passes, prefix lanes, passes walked)."""
    m, h = bits(member_mask), bits(holder_mask)
    pre = 8 * -(-dq // nl)
    lanes = np.arange(64)
    behind = lanes >= pre
    order = np.concatenate([lanes[~behind], lanes[behind & h], lanes[behind & m & ~h], lanes[behind & ~m]])
    slots = np.empty(64, dtype=np.int64)
    slots[order] = lanes
    top = int(lanes[m].max()) + 1 if m.any() else 0
    passes = -(-top // 8)
    want = pre // 8 + -(-int((behind & h).sum()) // 8)
    return slots, min(want, passes), pre, passes
