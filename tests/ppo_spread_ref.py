"""What the tests of the SPREAD binding of the PPO update share (tests/test_ppo_spread_cpu.py, tests/test_gpu_ppo_spread.py): the
geometry of include/ranenv.h's "One agent over the chip" restated in Python -- optimiser steps per kind, the pass grid of a step, which
slab walks which tiles, the tiles of the tail minibatch -- and the byte formula of ranenv_ppo_spread_bytes.  ``slip`` plants one of
three mistakes into the restatement, for the CPU test that shows each is caught.  Built on tests/ppo_update_ref.py and
tests/ppo_wide_ref.py, which stay as they are."""
from __future__ import annotations

from tests import ppo_update_ref as ref
from tests import ppo_wide_ref as wd

NET_ROWS = 32                            # rows of a tile
SLABS_MAX = 256
SLIPS = ("tiles in blocks", "grid of slabs", "full tail")


def tiles_of(rows):
    return -(-rows // NET_ROWS)


def minibatches(n_rows, minibatch, slip=None):
    """The entries of an epoch's minibatches in order: full ones, then the short tail"""
    sizes = [min(minibatch, n_rows - c0) for c0 in range(0, n_rows, minibatch)]
    if slip == "full tail" and sizes:
        sizes[-1] = minibatch
    return sizes


def grid_of(rows, slabs, slip=None):
    """Workgroups of the pass over a minibatch of ``rows`` entries"""
    return slabs if slip == "grid of slabs" else min(tiles_of(rows), slabs)


def plan(n_rows, minibatch, epochs, slabs, slip=None):
    """(optimiser steps of the kind, the first minibatch's grid, the tiles of an epoch's last minibatch): ranenv_ppo_spread_plan's three"""
    sizes = minibatches(n_rows, minibatch, slip)
    if not sizes:
        return 0, 0, 0
    return epochs * len(sizes), grid_of(sizes[0], slabs, slip), tiles_of(sizes[-1])


def walk(rows, slabs, slip=None):
    """[slab w's tiles in the order it walks them] for a minibatch of ``rows`` entries"""
    tiles, grid = tiles_of(rows), grid_of(rows, slabs, slip)
    if slip == "tiles in blocks":
        per = -(-tiles // grid)
        return [list(range(w * per, min((w + 1) * per, tiles))) for w in range(grid)]
    return [list(range(w, tiles, grid)) for w in range(grid)]


def walk_faults(got, rows, slabs):
    """What is wrong with a walk, by the header's own words: min(tiles, slabs) workgroups, none idle; workgroup w walks tiles w,
    w + grid, ... in ascending order; every tile once"""
    tiles, faults = tiles_of(rows), []
    if len(got) != min(tiles, slabs):
        faults.append(f"{len(got)} workgroups for {tiles} tiles and {slabs} slabs")
    if any(not t for t in got):
        faults.append("a workgroup without a tile")
    if sorted(x for t in got for x in t) != list(range(tiles)):
        faults.append("not every tile once")
    for w, t in enumerate(got):
        if t and (t[0] != w or any(b - a != len(got) for a, b in zip(t, t[1:]))):
            faults.append(f"workgroup {w} walks {t[:4]}")
            break
    return faults


def packed_floats(dims):
    """Floats of a net's packed copy: per layer W [np][kp] and b [np], widths padded to 32"""
    p = wd.padded(dims)
    return sum(n * k + n for k, n in zip(p[:-1], p[1:]))


def spread_bytes(actor, critic, slabs, wide):
    """ranenv_ppo_spread_bytes restated: 4 x slabs x (actor floats + critic floats + (wide: the pair's parked floats))"""
    floats = packed_floats(actor) + (packed_floats(critic) if critic is not None else 0)
    return 4 * slabs * (floats + (wd.wide_scratch_floats(actor, critic) if wide else 0))


def one_agent_nets(case, seed=4100):
    """{role: net} of ONE agent of a ref.CASES shape"""
    widths, act, layout = ref.CASES[case]
    return ref.make_role_nets(ref.S, ref.US, widths, act, layout, seed)
