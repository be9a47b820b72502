"""The per-slice spread binding without a GPU: the three new exports in the header, the ctypes table and the built library; the unit
geometry (ranenv_ppo_slices_spread_plan, the function the update sizes its launches with) against its restatement in
tests/ppo_per_slice_spread_ref.py on 200 seeded draws, with three planted slips shown to be caught; the byte formula
(ranenv_ppo_slices_spread_bytes) on 200 seeded shapes; what the entries refuse before they touch a handle; and the combination rules of
``ppo_bind`` and the caps of ``ppo_update_per_slice``."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from intent_radio_sched_multi_slice_amd import _lib
from intent_radio_sched_multi_slice_amd import batched_env as be
from tests import ppo_bindings_shapes_ref as bs
from tests import ppo_per_slice_spread_ref as ps
from tests import ppo_spread_ref as sp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = {"ranenv_ppo_bind_slices_spread": 4, "ranenv_ppo_slices_spread_bytes": 8, "ranenv_ppo_slices_spread_plan": 9}
E_INVALID = -1


def _lib_plan(lib, n_inter, first, minibatch, epochs, slabs):
    n = len(first) - 1
    steps, grid, call = (C.c_int64 * (1 + n))(*[-7] * (1 + n)), (C.c_int32 * (1 + n))(*[-7] * (1 + n)), C.c_int64(-7)
    f = np.ascontiguousarray(first, dtype=np.int32)
    assert lib.ranenv_ppo_slices_spread_plan(n, n_inter, f.ctypes.data_as(C.POINTER(C.c_int32)), minibatch, epochs, slabs, steps, grid, C.byref(call)) == 0
    return list(steps), list(grid), call.value


def test_header_binding_and_library_agree_on_the_new_exports():
    hdr = open(os.path.join(REPO, "include", "ranenv.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name, n_args in NEW_EXPORTS.items():
        proto = re.search(r"^int " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
        assert proto, f"{name} is not declared in include/ranenv.h"
        assert len(proto.group(1).split(",")) == n_args, name
        assert name in _lib.EXPORTS and len(_lib.FUNCTIONS[name][1]) == n_args and hasattr(lib, name), name
    assert "Nets per slice over the chip" in hdr and "THE CONTRACT" in hdr


def test_the_unit_geometry_against_the_library_on_200_seeded_draws():
    """Steps and first grid per unit and the call's steps; the units' numbering; and per step the launch grid the restatement gives:
    never below a live unit's own grid, zero exactly when every unit is through"""
    lib = _lib.load()
    seen_s, empty, below_tile, uneven = set(), 0, 0, 0
    for n_inter, first, minibatch, epochs, slabs in ps.draws():
        got = _lib_plan(lib, n_inter, first, minibatch, epochs, slabs)
        want = ps.plan(n_inter, first, minibatch, epochs, slabs)
        assert got == want, (n_inter, first.tolist(), minibatch, epochs, slabs)
        steps, grid, call = got
        rows = ps.unit_rows(n_inter, first)
        n = len(first) - 1
        seen_s.add(n)
        empty += any(r == 0 for r in rows[1:])
        below_tile += any(0 < r < sp.NET_ROWS for r in rows[1:])
        uneven += len(set(steps)) > 1
        assert [ps.unit_of(u) for u in range(1 + n)] == [(0, 0)] + [(1, s) for s in range(n)]
        assert all((s == 0) == (r == 0 or epochs == 0) and (g == 0) == (r == 0) for s, g, r in zip(steps, grid, rows))
        assert all(steps[u] == epochs * -(-rows[u] // minibatch) for u in range(1 + n)) and call == max(steps)
        for step in sorted({0, min(steps), max(call - 1, 0), call}):
            grids = ps.step_grids(n_inter, first, minibatch, epochs, slabs, step)
            assert [g > 0 for g in grids] == [step < s for s in steps], (step, steps)
            assert ps.launch_grid(n_inter, first, minibatch, epochs, slabs, step) == (max(grids), 1 + n)
            if step == 0 and epochs > 0:
                assert grids == grid
    assert seen_s == set(range(1, 17)) and empty > 50 and below_tile > 50 and uneven > 120      # (one draw in six has 0 epochs: no unit has a step)
    # the GPU cases' shares: 20, 100 and 250 rows beside 288 inter rows, minibatch 72, 2 epochs
    first = np.array([0, 20, 120, 370], dtype=np.int32)
    assert _lib_plan(lib, 288, first, 72, 2, 2) == ([8, 2, 4, 8], [2, 1, 2, 2], 8)
    assert _lib_plan(lib, 288, first, 72, 2, 8) == ([8, 2, 4, 8], [3, 1, 3, 3], 8)
    assert ps.step_grids(288, first, 72, 2, 8, 1) == [3, 1, 1, 3] and ps.step_grids(288, first, 72, 2, 8, 4) == [3, 0, 0, 3]
    # the large-batch example at S 5: 262 144 inter rows, 4 epochs, minibatch 8192, 64 slabs
    big = np.arange(6, dtype=np.int32) * 200000
    assert _lib_plan(lib, 262144, big, 8192, 4, 64) == ([128] + [100] * 5, [64] * 6, 128)
    assert lib.ranenv_ppo_slices_spread_plan(3, 288, first.ctypes.data_as(C.POINTER(C.c_int32)), 72, 2, 8, None, None, None) == 0


@pytest.mark.parametrize("slip", ps.SLIPS)
def test_planted_slips_of_the_unit_geometry_are_caught(slip):
    """The inter pair given slice 0's share, every unit given the steps of the largest share, the table read one entry on: each leaves
    the library's figures on most of the 200 draws (one in six has 0 epochs, where no unit has a step and the second slip is silent)"""
    lib = _lib.load()
    caught = sum(ps.plan(*d, slip) != _lib_plan(lib, *d) for d in ps.draws())
    print(f"{slip}: caught on {caught} of 200 draws")
    assert caught >= 120


def test_slices_spread_bytes_against_the_restated_formula_on_200_seeded_shapes():
    rng = np.random.default_rng(78)
    for i in range(200):
        n_slices, us, slabs = int(rng.integers(1, 17)), int(rng.integers(1, 17)), int(rng.integers(1, sp.SLABS_MAX + 1))
        hidden = [int(x) for x in rng.integers(1, 513, size=int(rng.integers(1, 5)))]
        hidden_c = [int(x) for x in rng.integers(1, 513, size=int(rng.integers(1, 5)))]
        n_in = 2 * us + 9 + (us if i % 2 else 0)
        inter = ([10 * n_slices] + hidden + [2 * n_slices], [10 * n_slices] + hidden_c + [1])
        intra = ([n_in] + hidden + [3], [n_in] + hidden_c + [1] if i % 5 else None)
        for wide in (False, True):
            got = be.ppo_slices_spread_bytes(*inter, *intra, n_slices, slabs, wide)
            assert got == ps.slices_spread_bytes(*inter, *intra, n_slices, slabs, wide), (inter, intra, n_slices, slabs, wide)
            assert got == be.ppo_spread_bytes(*inter, slabs, wide) + n_slices * be.ppo_spread_bytes(*intra, slabs, wide)
    # the header's warning: S 10, 256 slabs, [512] x 3 -- 12.7 gigabytes, 13.3 under the wide plan
    verybig = ([100, 512, 512, 512, 20], [100, 512, 512, 512, 1], [19, 512, 512, 512, 3], [19, 512, 512, 512, 1])
    assert round(be.ppo_slices_spread_bytes(*verybig, 10, 256) / 1e9, 1) == 12.7 and round(be.ppo_slices_spread_bytes(*verybig, 10, 256, wide=True) / 1e9, 1) == 13.3


GRID_SLICES, GRID_SLABS, GRID_INTER = (1, 10, 13, 16), (2, 3, 8, 256), (0, ps.SMALL, ps.B * ps.T)


def _grid_tables(n_slices):
    """The first-tables tests/test_gpu_ppo_per_slice_spread_shapes.py runs at ``n_slices``: one share of 100 rows, its right neighbour 20,
    every other slice all its live rows (192 .. 288 of them); the same with the last share empty; S 1: the one share of 20 or of 100"""
    if n_slices == 1:
        tables = [[ps.SMALL], [ps.MID]]
    else:
        shares = [192 + (37 * s) % 97 for s in range(n_slices)]
        big = n_slices // 3
        shares[big], shares[(big + 1) % n_slices] = ps.MID, ps.SMALL
        tables = [shares, shares[:-1] + [0]]
    return [np.concatenate([[0], np.cumsum(t)]).astype(np.int32) for t in tables]


def test_plan_on_the_shape_grid_and_the_planted_slips_at_sixteen_slices():
    """S 1, 10, 13 and 16 at minibatch 72 and 2 epochs, under 2, 3, 8 and 256 slabs, beside an inter list of 0, 20 and 288 rows, with and
    without an empty share: ranenv_ppo_slices_spread_plan gives the restatement's figures, and at S 16 each of the three planted slips
    leaves them on every table"""
    lib = _lib.load()
    assert {bs.slice_spec(c)[0] for c in bs.SLICE_SHAPES} == set(GRID_SLICES) and GRID_INTER == (0, 20, 288)
    for n_slices in GRID_SLICES:
        for first in _grid_tables(n_slices):
            for n_inter in GRID_INTER:
                for slabs in GRID_SLABS:
                    args = (n_inter, first, ps.MB, ps.EPOCHS, slabs)
                    got = _lib_plan(lib, *args)
                    assert got == ps.plan(*args), (n_slices, first.tolist(), n_inter, slabs)
                    steps, grid, call = got
                    rows = ps.unit_rows(n_inter, first)
                    assert steps == [ps.EPOCHS * -(-r // ps.MB) for r in rows] and call == max(steps)
                    assert grid == [min(sp.tiles_of(min(r, ps.MB)), slabs) for r in rows]
                    if n_slices == 16:
                        for slip in ps.SLIPS:
                            assert ps.plan(*args, slip) != got, (slip, first.tolist(), n_inter, slabs)
    # the shares of 20 and 100 rows beside 288 inter rows: 2, 4 and 8 steps; an inter list of 20 rows is through first
    first = _grid_tables(16)[0]
    steps = _lib_plan(lib, 288, first, ps.MB, ps.EPOCHS, 3)[0]
    assert steps[0] == 8 and sorted(set(steps[1:])) == [2, 4, 6, 8]
    assert _lib_plan(lib, 20, first, ps.MB, ps.EPOCHS, 3)[0][0] == 2 and _lib_plan(lib, 0, first, ps.MB, ps.EPOCHS, 3)[0][0] == 0


def test_slices_spread_bytes_of_every_grid_case_against_the_restated_formula():
    """Every case tests/test_gpu_ppo_per_slice_spread_shapes.py binds, at 2, 3, 8 and 256 slabs, under both plans"""
    for case in bs.SLICE_SPREAD_SHAPES + bs.SLICE_BEYOND:
        n_slices, dims = bs.slice_spec(case)[0], bs.slice_dims(case)
        for slabs in GRID_SLABS:
            for wide in (False, True):
                got = be.ppo_slices_spread_bytes(*dims["inter"], *dims["intra"], n_slices, slabs, wide)
                assert got == ps.slices_spread_bytes(*dims["inter"], *dims["intra"], n_slices, slabs, wide), (case, slabs, wide)
                assert got == 4 * slabs * sum(n * (f + (bs.wd.wide_scratch_floats(*dims[k]) if wide else 0))
                                              for k, n, f in (("inter", 1, bs.slice_kind_floats(case)["inter"][1]), ("intra", n_slices, bs.slice_kind_floats(case)["intra"][1])))
    b, c = bs.slice_dims("B"), bs.slice_dims("C")
    assert be.ppo_slices_spread_bytes(*b["inter"], *b["intra"], 13, 256) == 454033408 < 512 << 20 < be.ppo_slices_spread_bytes(*c["inter"], *c["intra"], 16, 256) == 546209792


def test_the_entries_refuse_their_arguments_before_a_handle():
    lib, out = _lib.load(), C.c_int64(-7)
    for slabs in (0, 257):
        assert lib.ranenv_ppo_bind_slices_spread(None, slabs, 0, None) == E_INVALID and f"slabs {slabs} (1..256)".encode() in lib.ranenv_last_error(None)
    assert lib.ranenv_ppo_bind_slices_spread(None, 64, 2, None) == E_INVALID and b"wide 2" in lib.ranenv_last_error(None)
    assert lib.ranenv_ppo_bind_slices_spread(None, 64, 1, None) == E_INVALID and b"null handle" in lib.ranenv_last_error(None)
    actor, critic = _lib.Mlp(), _lib.Mlp()
    actor.n_hidden, actor.dims[0], actor.dims[1], actor.dims[2] = 1, 50, 64, 10
    critic.n_hidden, critic.dims[0], critic.dims[1], critic.dims[2] = 1, 50, 64, 1
    a, c = C.byref(actor), C.byref(critic)
    assert lib.ranenv_ppo_slices_spread_bytes(None, c, a, c, 5, 4, 0, C.byref(out)) == E_INVALID and out.value == -7
    assert lib.ranenv_ppo_slices_spread_bytes(a, c, None, c, 5, 4, 0, C.byref(out)) == E_INVALID and out.value == -7
    assert lib.ranenv_ppo_slices_spread_bytes(a, c, a, c, 5, 4, 0, None) == E_INVALID
    for slabs in (0, 257):
        assert lib.ranenv_ppo_slices_spread_bytes(a, c, a, c, 5, slabs, 0, C.byref(out)) == E_INVALID and out.value == -7
        assert f"slabs {slabs} (1..256)".encode() in lib.ranenv_last_error(None)
    assert lib.ranenv_ppo_slices_spread_bytes(a, c, a, c, 5, 4, 2, C.byref(out)) == E_INVALID and b"wide 2" in lib.ranenv_last_error(None)
    assert lib.ranenv_ppo_slices_spread_bytes(a, c, a, c, 0, 4, 0, C.byref(out)) == E_INVALID and b"n_slices 0" in lib.ranenv_last_error(None)
    assert lib.ranenv_ppo_slices_spread_bytes(a, None, a, None, 5, 4, 0, C.byref(out)) == 0 and out.value == 6 * sp.spread_bytes([50, 64, 10], None, 4, False)
    first = (C.c_int32 * 3)(0, 10, 30)
    for bad in ((0, 5, first, 8, 1, 4), (2, -1, first, 8, 1, 4), (2, 5, None, 8, 1, 4), (2, 5, first, 0, 1, 4), (2, 5, first, 8, -1, 4), (2, 5, first, 8, 1, 0),
                (2, 5, first, 8, 1, 257), (2, 5, (C.c_int32 * 3)(1, 10, 30), 8, 1, 4), (2, 5, (C.c_int32 * 3)(0, 10, 9), 8, 1, 4)):
        assert lib.ranenv_ppo_slices_spread_plan(*bad, None, None, None) == E_INVALID, bad[:2] + bad[3:]


class _Reached(Exception):
    pass


class _NoLibrary:
    """Stands where the library would: every entry reached raises with its name"""
    def __getattr__(self, name):
        raise _Reached(name)


def test_ppo_bind_checks_the_per_slice_spread_combinations_before_the_handle(monkeypatch):
    import contextlib
    env = object.__new__(be.BatchedRanEnv)      # (refused before the handle is touched: no GPU needed)
    for wide in (dict(), dict(wide=True)):
        with pytest.raises(ValueError) as e:    # (slabs has no default in this form: the two together raise as they always did)
            env.ppo_bind(per_slice=True, spread=True, **wide)
        assert "spread and per_slice" in str(e.value)
    for kw, word in ((dict(head=True), "spread and per_slice"), (dict(mixed=True), "spread and mixed"), (dict(bf16=True), "bf16 and per_slice"),
                     (dict(head=True, wide=True), "head, spread and wide")):
        with pytest.raises(ValueError) as e:
            env.ppo_bind(per_slice=True, spread=True, slabs=8, **kw)
        assert word in str(e.value), kw
    assert not hasattr(env, "_ppo_spread") and not hasattr(env, "_ppo_slices_spread")
    env.device, env._lib = torch.device("cpu"), _NoLibrary()
    monkeypatch.setattr(be.torch.cuda, "device", lambda d: contextlib.nullcontext())      # (no device to select here)
    for wide in (dict(), dict(wide=True)):      # (with slabs the form reaches the library, and its own entry)
        with pytest.raises(_Reached, match="^ranenv_ppo_bind_slices_spread$"):
            env.ppo_bind(per_slice=True, spread=True, slabs=8, **wide)
    with pytest.raises(_Reached, match="^ranenv_ppo_bind_slices$"):
        env.ppo_bind(per_slice=True)
    with pytest.raises(_Reached, match="^ranenv_ppo_bind_spread$"):
        env.ppo_bind(spread=True, slabs=8)


def test_update_per_slice_drops_the_row_cap_under_the_per_slice_spread_binding_alone():
    """The caps are checked before the library is reached: under the per-slice binding 2^21 rows x epochs of a policy are refused; under
    its spread form they pass and the call goes on to the record and the library (which this test does not have); the cap on
    optimiser steps holds per policy under both"""
    n = 1 << 21
    order = {"order_inter": torch.zeros((1, n), dtype=torch.int32), "first_inter": np.array([0, n], dtype=np.int32)}
    for spread in (False, True):
        env = object.__new__(be.BatchedRanEnv)
        env.device, env._lib, env._ppo_slices_spread, env.S, env.B = torch.device("cpu"), _NoLibrary(), spread, 3, 4
        if spread:
            with pytest.raises((_Reached, KeyError, AttributeError)):      # (past the caps: the empty record, or the library, is what the call misses next)
                env.ppo_update_per_slice({}, epochs=1, minibatch=65536, order=order)
        else:
            with pytest.raises(be.RanEnvError, match="rows x epochs"):
                env.ppo_update_per_slice({}, epochs=1, minibatch=65536, order=order)
        few = order if spread else {"order_inter": order["order_inter"][:, :1 << 19].contiguous(), "first_inter": np.array([0, 1 << 19], dtype=np.int32)}
        with pytest.raises(be.RanEnvError, match="optimiser steps"):
            env.ppo_update_per_slice({}, epochs=1, minibatch=32, order=few)
