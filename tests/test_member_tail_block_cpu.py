"""The packed member-lines copy, host side (include/ranenv.h, "MEMBER LINES": the handle's copy): the layout arithmetic
(ranenv_member_lines_packed_layout) and the restatement of cluster part + owner's finish on a UE's walk lines and its 8-float slot
of the tail block (ranenv_member_lines_packed_sums_host) -- bit for bit np.sum of the float32 row as float64, and bit for bit
ranenv_member_lines_owner_tail_sums_host on the same row laid out the old way (tail line behind the walked lines).  No GPU."""
import ctypes as C

import numpy as np
import pytest

from tests.member_lines_ref import lay_out, leaves_of, plan_of
from tests.member_tail_block_ref import packed_layout
from tests.test_member_tail_cpu import ranges_of, rows_of

US = [1, 7, 25, 33, 100]
# R < 8; one leaf with every R % 8 (8 .. 15) and its longest; two leaves (the headline's 135 among them); three, four, five leaves
RS = [1, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 71, 128, 130, 135, 136, 256, 263, 300, 419, 488, 520, 527]


@pytest.fixture(scope="module")
def lib():
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.csrc import build
    build.build()
    return _lib.load()


def test_the_grid_covers_what_it_should():
    assert sorted({len(leaves_of(0, R)) for R in RS}) == [1, 2, 3, 4, 5]
    assert sorted({R % 8 for R in RS}) == list(range(8)) and sorted({R % 8 for R in RS if 8 <= R <= 128}) == list(range(8))
    assert any(R < 8 for R in RS)
    for R in (135, 263, 419, 71):
        kinds = {w for _, _, w in ranges_of(R)}
        assert {"ends exactly at R - tail", "starts exactly at R - tail", "straddles R - tail", "strictly inside the tail"} <= kinds, R


@pytest.mark.parametrize("U", US)
def test_layout_arithmetic(lib, U):
    for R in RS:
        nlw, off, nbytes = C.c_int32(-1), C.c_int64(-1), C.c_int64(-1)
        assert lib.ranenv_member_lines_packed_layout(U, R, C.byref(nlw), C.byref(off), C.byref(nbytes)) == 0
        tail = R % 8
        assert off.value == U * nlw.value * 128, (U, R)
        assert nbytes.value % 128 == 0 and nbytes.value >= off.value + (32 * U if tail else 0), (U, R)
        assert nbytes.value < off.value + (32 * U if tail else 0) + 128, (U, R)          # (rounded up, no more)
        if tail == 0:
            assert nbytes.value == off.value == U * len(plan_of(R)) * 128, (U, R)          # no block: the copy as it was
        if R < 8:
            assert nlw.value == 0 and off.value == 0, (U, R)                               # the block only
        # nlw is what the owner-tail restatement says the clusters walk
        x = np.ascontiguousarray(lay_out(np.ones(R, dtype=np.float32)))
        f, p, walked = C.c_double(), C.c_double(), C.c_int32(-1)
        assert lib.ranenv_member_lines_owner_tail_sums_host(C.c_void_p(x.ctypes.data), R, 0, R, C.byref(f), C.byref(p), C.byref(walked)) == 0
        assert nlw.value == walked.value, (U, R)
        assert (nlw.value, off.value, nbytes.value) == packed_layout(U, R), (U, R)
    n, o, b = C.c_int32(), C.c_int64(), C.c_int64()
    assert lib.ranenv_member_lines_packed_layout(100, 135, C.byref(n), C.byref(o), C.byref(b)) == 0
    assert (n.value, o.value, b.value) == (4, 51200, 54400)
    assert lib.ranenv_member_lines_packed_layout(25, 135, C.byref(n), C.byref(o), C.byref(b)) == 0
    assert (n.value, o.value, b.value) == (4, 12800, 13696)                               # 800 bytes of block, 96 of padding
    assert lib.ranenv_member_line_plan(135, 0, None, None, None) == 5                     # the public plan keeps its tail line


@pytest.mark.parametrize("R", RS)
def test_packed_sums_equal_numpy_and_the_old_layout_bit_for_bit(lib, R):
    tail = R % 8
    nlw = len(plan_of(R)) - (1 if tail else 0)
    bits = lambda v: np.float64(v).view(np.int64)
    for trial, row in rows_of(R):
        lines = np.ascontiguousarray(lay_out(row))
        # the packed pieces, each in memory of its own with poison around it: the walk lines alone, the 8-float slot alone
        walk = np.full((nlw + 1) * 32, np.float32(np.nan)); walk[:nlw * 32] = lines[:nlw].reshape(-1)
        slot = np.full(16, np.float32(np.nan)); slot[:8] = lines[nlw, :8] if tail else 0.0
        assert not tail or (np.array_equal(slot[:tail], row[R - tail:]) and not slot[tail:8].any())
        row64 = row.astype(np.float64)
        for s, c, what in ranges_of(R):
            full, part = C.c_double(-1.0), C.c_double(-1.0)
            assert lib.ranenv_member_lines_packed_sums_host(C.c_void_p(walk.ctypes.data) if nlw else None, C.c_void_p(slot.ctypes.data) if tail else None,
                                                            R, s, c, C.byref(full), C.byref(part)) == 0
            masked = np.zeros(R, dtype=np.float64)
            masked[s:s + c] = row64[s:s + c]
            want_full, want_part = np.sum(row64), np.sum(masked)
            assert bits(full.value) == want_full.view(np.int64), (R, trial, what, s, c, full.value, want_full)
            assert bits(part.value) == want_part.view(np.int64), (R, trial, what, s, c, part.value, want_part)
            f0, p0, w0 = C.c_double(-1.0), C.c_double(-1.0), C.c_int32()
            assert lib.ranenv_member_lines_owner_tail_sums_host(C.c_void_p(lines.ctypes.data), R, s, c, C.byref(f0), C.byref(p0), C.byref(w0)) == 0
            assert bits(f0.value) == bits(full.value) and bits(p0.value) == bits(part.value), (R, trial, what)


def test_bad_arguments_are_refused(lib):
    n, o, b, d = C.c_int32(), C.c_int64(), C.c_int64(), C.c_double()
    assert lib.ranenv_member_lines_packed_layout(0, 135, C.byref(n), C.byref(o), C.byref(b)) < 0
    assert lib.ranenv_member_lines_packed_layout(100, 0, C.byref(n), C.byref(o), C.byref(b)) < 0
    assert lib.ranenv_member_lines_packed_layout(100, 135, None, C.byref(o), C.byref(b)) < 0
    assert lib.ranenv_member_lines_packed_layout(100, 135, C.byref(n), None, C.byref(b)) < 0
    assert lib.ranenv_member_lines_packed_layout(100, 135, C.byref(n), C.byref(o), None) < 0
    x = np.zeros(64, dtype=np.float32)
    p = C.c_void_p(x.ctypes.data)
    assert lib.ranenv_member_lines_packed_sums_host(None, p, 9, 0, 9, C.byref(d), C.byref(d)) < 0          # walk lines missing
    assert lib.ranenv_member_lines_packed_sums_host(p, None, 9, 0, 9, C.byref(d), C.byref(d)) < 0          # slot missing
    assert lib.ranenv_member_lines_packed_sums_host(p, p, 9, 0, 9, None, C.byref(d)) < 0
    assert lib.ranenv_member_lines_packed_sums_host(p, p, 9, 0, 9, C.byref(d), None) < 0
    assert lib.ranenv_member_lines_packed_sums_host(p, p, 0, 0, 0, C.byref(d), C.byref(d)) < 0
    assert lib.ranenv_member_lines_packed_sums_host(p, p, 9, -1, 2, C.byref(d), C.byref(d)) < 0
    assert lib.ranenv_member_lines_packed_sums_host(p, p, 9, 0, -1, C.byref(d), C.byref(d)) < 0
    assert lib.ranenv_member_lines_packed_sums_host(p, None, 8, 0, 8, C.byref(d), C.byref(d)) == 0         # no tail: no slot needed
    assert lib.ranenv_member_lines_packed_sums_host(None, p, 5, 0, 5, C.byref(d), C.byref(d)) == 0         # R < 8: no walk lines needed
    # the packed retile refuses what its sibling refuses, before any launch
    assert lib.ranenv_se_retile_member_lines_packed(None, 0, 135 * 100, p, 1, 100, 135, None) < 0
    assert lib.ranenv_se_retile_member_lines_packed(p, 0, 135 * 100, None, 1, 100, 135, None) < 0
    assert lib.ranenv_se_retile_member_lines_packed(p, 0, 135 * 100, p, -1, 100, 135, None) < 0
    assert lib.ranenv_se_retile_member_lines_packed(p, 0, 135 * 100 - 1, p, 1, 100, 135, None) < 0       # a stride below a tile
    assert lib.ranenv_se_retile_member_lines_packed(p, 0, 135 * 100, C.c_void_p(x.ctypes.data + 4), 1, 100, 135, None) < 0      # misaligned
