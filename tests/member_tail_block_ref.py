"""numpy restatement of the PACKED member-lines copy (include/ranenv.h, "MEMBER LINES": the handle's copy): per tile the whole-group
lines [U][nlw][32] of tests/member_lines_ref.py's plan, then -- R % 8 != 0 -- one tail block [U][8] with UE u's last R % 8 RBs at
the head of its 32-byte slot, the tile rounded up to whole 128-byte lines; +0.0 wherever nothing is stored.  Shared by
tests/test_member_tail_block_cpu.py and tests/test_gpu_member_tail_block.py."""
import numpy as np

from tests.member_lines_ref import lay_out_pool, plan_of


def packed_layout(U, R):
    """(walked lines per UE, the block's byte offset within a tile, a tile's bytes)."""
    tail = R % 8
    nlw = len(plan_of(R)) - (1 if tail else 0)
    off = U * nlw * 128
    return nlw, off, (off + (32 * U if tail else 0) + 127) // 128 * 128


def lay_out_pool_packed(rb):
    """RB-major tiles [n, R, U] -> packed tiles [n, tile floats]."""
    n, R, U = rb.shape
    nlw, off, nbytes = packed_layout(U, R)
    lines = lay_out_pool(rb)                                   # [n, U, lines, 32], the tail line last
    out = np.zeros((n, nbytes // 4), dtype=np.float32)
    out[:, :off // 4] = lines[:, :, :nlw, :].reshape(n, -1)
    if R % 8:
        out[:, off // 4:off // 4 + 8 * U] = lines[:, :, nlw, :8].reshape(n, -1)
    return out
