"""numpy restatement of the member-lines copy of the SE pool (include/ranenv.h, "MEMBER LINES"): numpy's pairwise leaves, the line
plan, and the layout of one row and of a whole pool.  Shared by tests/test_member_lines_cpu.py and tests/test_gpu_member_lines.py.

numpy's pairwise sum (numpy/core/src/umath/loops_utils.h.src, pairwise_sum): a row of n <= 128 elements is a leaf (eight
accumulators over its whole groups of 8, a fixed tree, the n % 8 last elements one after the other); a longer one is cut at
n // 2 rounded down to a multiple of 8 and the halves are added.  So every leaf but the last is a multiple of 8 long."""
import numpy as np


def leaves_of(lo, n):
    if n <= 128:
        return [(lo, n)]
    n2 = n // 2
    n2 -= n2 % 8
    return leaves_of(lo, n2) + leaves_of(lo + n2, n - n2)


def plan_of(R):
    """[(leaf, first RB, whole groups held)] per line; the tail line holds 0 groups."""
    lv = leaves_of(0, R)
    plan = []
    for k, (lo, n) in enumerate(lv):
        G = n // 8
        plan += [(k, lo + 32 * c, min(4, G - 4 * c)) for c in range((G + 3) // 4)]
    if R % 8:
        plan.append((len(lv) - 1, R - R % 8, 0))
    return plan


def lay_out_pool(rb):
    """RB-major tiles [n, R, U] -> member lines [n, U, lines, 32]: position 4 j + g of a chunk line = RB first + 8 g + j, the tail
    line's position p = RB first + p, +0.0 everywhere else."""
    n, R, U = rb.shape
    plan = plan_of(R)
    out = np.zeros((n, U, len(plan), 32), dtype=np.float32)
    for l, (_, rb0, ng) in enumerate(plan):
        if ng == 0:
            out[:, :, l, :R % 8] = rb[:, rb0:, :].transpose(0, 2, 1)
        for g in range(ng):
            for j in range(8):
                out[:, :, l, 4 * j + g] = rb[:, rb0 + 8 * g + j, :]
    return out


def lay_out(row):
    """One row [R] -> its lines [lines, 32]."""
    return lay_out_pool(np.asarray(row, dtype=np.float32).reshape(1, -1, 1))[0, 0]
