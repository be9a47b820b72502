"""The member-lines copy of the SE pool (include/ranenv.h, "MEMBER LINES"), host side: the line plan against numpy's own leaf
cutting (tests/member_lines_ref.py), and the sums of a row laid out in lines -- walked in the kernels' order by plain C++ --
against np.sum, bit for bit.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from tests.member_lines_ref import lay_out, leaves_of, plan_of

R_ALL = [r for r in range(1, 521) if not 489 <= r <= 511]
R_SUMS = [1, 5, 7, 8, 9, 64, 127, 128, 129, 130, 135, 256, 257, 300, 419, 488, 512, 520]


@pytest.fixture(scope="module")
def lib():
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.csrc import build
    build.build()
    return _lib.load()


def test_line_plan_follows_numpys_leaves(lib):
    assert [n for _, n in leaves_of(0, 135)] == [64, 71] and len(plan_of(135)) == 5
    i32 = C.POINTER(C.c_int32)
    for R in R_ALL:
        want = plan_of(R)
        n = lib.ranenv_member_line_plan(R, 0, None, None, None)
        assert n == len(want), R
        leaf, rb0, ng = (np.full(n + 2, -7, dtype=np.int32) for _ in range(3))
        assert lib.ranenv_member_line_plan(R, n, leaf.ctypes.data_as(i32), rb0.ctypes.data_as(i32), ng.ctypes.data_as(i32)) == n
        assert list(zip(leaf[:n].tolist(), rb0[:n].tolist(), ng[:n].tolist())) == want, R
        assert (leaf[n:] == -7).all() and (rb0[n:] == -7).all() and (ng[n:] == -7).all(), R       # nothing written past max_lines
        # every RB sits in exactly one position
        seen = np.zeros(R, dtype=np.int32)
        for _, first, groups in want:
            seen[first:first + (8 * groups if groups else R % 8)] += 1
        assert (seen == 1).all(), R
    assert lib.ranenv_member_line_plan(135, 0, None, None, None) == 5
    assert lib.ranenv_member_line_plan(0, 0, None, None, None) < 0


def ranges_of(R):
    lv = leaves_of(0, R)
    cut = lv[1][0] if len(lv) > 1 else R // 2
    out = [(0, 0), (R // 3, 0), (0, R), (R // 2, 1), (R - 1, 1), (0, 1)]
    out.append((max(cut - 3, 0), min(7, R - max(cut - 3, 0))))            # straddles a leaf boundary (the row's middle where it has one leaf)
    out.append((max(R - (R % 8) - 2, 0), R - max(R - (R % 8) - 2, 0)))    # ends in the tail (at the row's end)
    if len(lv) > 2:
        out.append((lv[1][0] + 5, lv[2][0] + 9 - lv[1][0] - 5))
    return out


@pytest.mark.parametrize("R", R_SUMS)
def test_row_sums_from_lines_equal_numpy_bit_for_bit(lib, R):
    rng = np.random.default_rng(1000 + R)
    for trial in range(4):
        row = (rng.random(R, dtype=np.float32) * np.float32(8.0)).astype(np.float32)
        # a subnormal, a zero and a large value where the row has room for them
        for k, v in enumerate((np.float32(1e-41), np.float32(0.0), np.float32(3e30))):
            if R > k and trial > 0:
                row[int(rng.integers(0, R))] = v
        if trial == 3:
            row[:] = row * np.float32(1e-3)
        lines = np.ascontiguousarray(lay_out(row))
        row64 = row.astype(np.float64)
        for s, c in ranges_of(R):
            full, part = C.c_double(-1.0), C.c_double(-1.0)
            assert lib.ranenv_member_lines_row_sums_host(C.c_void_p(lines.ctypes.data), R, s, c, C.byref(full), C.byref(part)) == 0
            masked = np.zeros(R, dtype=np.float64)
            masked[s:s + c] = row64[s:s + c]
            want_full, want_part = np.sum(row64), np.sum(masked)
            assert np.float64(full.value).view(np.int64) == want_full.view(np.int64), (R, trial, s, c, full.value, want_full)
            assert np.float64(part.value).view(np.int64) == want_part.view(np.int64), (R, trial, s, c, part.value, want_part)


def test_row_sums_host_refuses_bad_arguments(lib):
    x = np.zeros(32, dtype=np.float32)
    d = C.c_double()
    assert lib.ranenv_member_lines_row_sums_host(None, 8, 0, 8, C.byref(d), C.byref(d)) < 0
    assert lib.ranenv_member_lines_row_sums_host(C.c_void_p(x.ctypes.data), 0, 0, 0, C.byref(d), C.byref(d)) < 0
    assert lib.ranenv_member_lines_row_sums_host(C.c_void_p(x.ctypes.data), 8, -1, 2, C.byref(d), C.byref(d)) < 0
