"""What the tests of the PER-SLICE SPREAD binding of the PPO update share (tests/test_ppo_per_slice_spread_cpu.py,
tests/test_gpu_ppo_per_slice_spread.py): the unit geometry of include/ranenv.h's "Nets per slice over the chip" restated in Python --
unit u -> kind, mem, its rows n_u, its optimiser steps, its pass grid per step, and the call's steps --, the byte formula of
ranenv_ppo_slices_spread_bytes, and the GPU cases.  ``slip`` plants one of three mistakes into the restatement, for the CPU test that
shows each is caught.  Built on tests/ppo_update_ref.py (``ref``), tests/ppo_bindings_shapes_ref.py (``bs``) and tests/ppo_spread_ref.py
(``sp``), which stay as they are.

THE GPU CASES.  S 3, Us 4, B 12, T 24 (288 inter rows; 288 cells per slice at most), nets of ``ref.CASES``, S DISTINCT pairs per slice,
minibatch 72 = two full tiles and one of 8 rows, 2 epochs.  ``bs.slice_order`` gives the slice with the most live rows MID = 100 rows
(72 + 28: a short last minibatch of ONE tile, fewer than every slab count but 1), its right neighbour SMALL = 20 (below one tile: one
step per epoch) and the third all its live rows (at least 73: several minibatches); the inter pair walks 288 rows in four minibatches.
So the units' step counts differ -- 2, 4, 2 x ceil(live / 72) and 8 -- and units finish while others go on.  SLABS = (2, 3, 8): fewer
than, equal to and more than a minibatch's three tiles."""
from __future__ import annotations

import numpy as np

from tests import ppo_bindings_shapes_ref as bs
from tests import ppo_spread_ref as sp
from tests import ppo_update_ref as ref

SLIPS = ("unit 0 as a slice", "steps of the largest share", "first shifted by one")

# ---- the GPU cases ------------------------------------------------------------------------------------------------------------------
S, US, B, T, MB, EPOCHS = 3, 4, 12, 24, 72, 2
SMALL, MID = 20, 100
SLABS = (2, 3, 8)
MB_TILES = sp.tiles_of(MB)
NET_SEED = 4100
assert MB_TILES == 3 and MB % sp.NET_ROWS != 0 and min(SLABS) < MB_TILES == SLABS[1] < max(SLABS)
assert SMALL < sp.NET_ROWS and MID > MB and sp.tiles_of(MID - MB) == 1 < min(SLABS)


def nets(case, n_slices=S, us=US, seed=NET_SEED):
    """The inter pair and ``n_slices`` distinct intra pairs of a ``ref.CASES`` shape: {"inter", "v_inter": net, "intra", "v_intra": [nets]}"""
    widths, act, layout = ref.CASES[case]
    per = [ref.make_role_nets(n_slices, us, widths, act, layout, seed + 10 * s) for s in range(n_slices)]
    return {"inter": per[0]["inter"], "v_inter": per[0]["v_inter"], "intra": [p["intra"] for p in per], "v_intra": [p["v_intra"] for p in per]}


# ---- the unit geometry --------------------------------------------------------------------------------------------------------------
def unit_rows(n_inter, first_slice, slip=None):
    """[n_u] for the 1 + S units: unit 0 the inter pair's n_inter rows, unit 1 + s the entries [first_slice[s], first_slice[s + 1])"""
    first = [int(x) for x in first_slice]
    n_slices = len(first) - 1
    if slip == "first shifted by one":
        first = first[1:] + first[-1:]
    rows = [int(n_inter)] + [first[s + 1] - first[s] for s in range(n_slices)]
    if slip == "unit 0 as a slice":
        rows[0] = rows[1]
    return rows


def unit_of(u):
    """(kind, mem) of unit u: ppo_update_body<.., SLICES>'s numbering"""
    return (1, u - 1) if u > 0 else (0, 0)


def plan(n_inter, first_slice, minibatch, epochs, slabs, slip=None):
    """(unit_steps [1 + S], unit_grid [1 + S], call_steps): ranenv_ppo_slices_spread_plan's three"""
    rows = unit_rows(n_inter, first_slice, slip)
    per_unit = [sp.plan(n, minibatch, epochs, slabs) for n in rows]
    steps, grid = [p[0] for p in per_unit], [p[1] for p in per_unit]
    if slip == "steps of the largest share":
        steps = [max(steps)] * len(steps)
    return steps, grid, max(steps)


def step_grids(n_inter, first_slice, minibatch, epochs, slabs, step):
    """[the pass grid of unit u at optimiser step ``step``; 0: the unit is through or has no rows]"""
    out = []
    for n in unit_rows(n_inter, first_slice):
        sizes = sp.minibatches(n, minibatch)
        out.append(sp.grid_of(sizes[step % len(sizes)], slabs) if sizes and step < epochs * len(sizes) else 0)
    return out


def launch_grid(n_inter, first_slice, minibatch, epochs, slabs, step):
    """(x, y) of the pass launch of a step: the largest grid over the live units, 1 + S"""
    return max(step_grids(n_inter, first_slice, minibatch, epochs, slabs, step)), len(first_slice)


# ---- bytes --------------------------------------------------------------------------------------------------------------------------
def slices_spread_bytes(inter_actor, inter_critic, intra_actor, intra_critic, n_slices, slabs, wide):
    """ranenv_ppo_slices_spread_bytes restated: the inter pair's ranenv_ppo_spread_bytes plus n_slices times one intra pair's"""
    return sp.spread_bytes(inter_actor, inter_critic, slabs, wide) + n_slices * sp.spread_bytes(intra_actor, intra_critic, slabs, wide)


def draws(seed=31337, n=200):
    """(n_inter, first_slice [S + 1], minibatch, epochs, slabs): S 1..16, one share in five empty, one in five below a tile"""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        n_slices = int(rng.integers(1, 17))
        shares = []
        for _s in range(n_slices):
            k = int(rng.integers(0, 5))
            shares.append(0 if k == 0 else (int(rng.integers(1, sp.NET_ROWS)) if k == 1 else int(rng.integers(sp.NET_ROWS, 3000))))
        first = np.concatenate([[0], np.cumsum(shares)]).astype(np.int32)
        yield int(rng.integers(0, 5001)), first, int(rng.integers(1, 601)), int(rng.integers(0, 6)), int(rng.integers(1, sp.SLABS_MAX + 1))


def slice_order(rec, epochs, empty=None, seed=3):
    """``bs.slice_order`` at the cases' figures: (order, the slices' shares [S]); asserts the docstring's hazards"""
    order, counts = bs.slice_order(rec, epochs, MB, SMALL, MID, empty, seed)
    rest = [c for c in counts if c not in (SMALL, MID, 0)]
    assert empty is not None or (counts.count(SMALL) >= 1 and counts.count(MID) >= 1 and len(rest) == S - 2 and all(c > MB for c in rest)), counts
    return order, counts
