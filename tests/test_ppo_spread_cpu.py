"""The spread binding of the PPO update without a GPU: the geometry the host computes (ranenv_ppo_spread_plan) and the byte formula
(ranenv_ppo_spread_bytes) against their restatements in tests/ppo_spread_ref.py; three planted slips of the geometry shown to be caught;
the three new exports in the header, the ctypes table and the built library; ``ppo_order_firsts`` under the spread caps; and what
``ppo_bind`` refuses before it reaches the library."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from intent_radio_sched_multi_slice_amd import _lib
from intent_radio_sched_multi_slice_amd import batched_env as be
from tests import ppo_spread_ref as sp
from tests import ppo_update_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = {"ranenv_ppo_bind_spread": 4, "ranenv_ppo_spread_bytes": 5, "ranenv_ppo_spread_plan": 7}
E_INVALID = -1


def _draws():
    rng = np.random.default_rng(20250)
    for _ in range(200):
        yield int(rng.integers(1, 5001)), int(rng.integers(1, 601)), int(rng.integers(0, 6)), int(rng.integers(1, sp.SLABS_MAX + 1))


def _lib_plan(lib, n_rows, minibatch, epochs, slabs):
    steps, grid, tail = C.c_int64(-7), C.c_int32(-7), C.c_int32(-7)
    assert lib.ranenv_ppo_spread_plan(n_rows, minibatch, epochs, slabs, C.byref(steps), C.byref(grid), C.byref(tail)) == 0
    return steps.value, grid.value, tail.value


def test_header_binding_and_library_agree_on_the_new_exports():
    hdr = open(os.path.join(REPO, "include", "ranenv.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name, n_args in NEW_EXPORTS.items():
        proto = re.search(r"^int " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
        assert proto, f"{name} is not declared in include/ranenv.h"
        assert len(proto.group(1).split(",")) == n_args, name
        assert name in _lib.EXPORTS and len(_lib.FUNCTIONS[name][1]) == n_args and hasattr(lib, name), name
    assert re.search(r"^#define RANENV_ABI_VERSION 10\b", hdr, re.M), "added entries leave the ABI version at 10"


def test_the_geometry_against_the_library_on_200_seeded_draws():
    """Steps per kind, the first minibatch's grid and the tail minibatch's tiles; and the restated walk -- which slab walks which tiles --
    against the header's words for every minibatch size the draw has"""
    lib = _lib.load()
    tails = 0
    for n_rows, minibatch, epochs, slabs in _draws():
        assert _lib_plan(lib, n_rows, minibatch, epochs, slabs) == sp.plan(n_rows, minibatch, epochs, slabs), (n_rows, minibatch, epochs, slabs)
        sizes = sp.minibatches(n_rows, minibatch)
        assert sum(sizes) == n_rows and all(0 < s <= minibatch for s in sizes)
        tails += sizes[-1] != minibatch
        for rows in {sizes[0], sizes[-1]}:
            assert not sp.walk_faults(sp.walk(rows, slabs), rows, slabs), (rows, slabs)
    assert tails > 50
    assert _lib_plan(lib, 0, 64, 3, 8) == (0, 0, 0)
    assert _lib_plan(lib, 96, ref.ALL, 1, 32) == (1, 3, 3)           # (the GPU tests' inter kind: three tiles under 32 slabs)
    assert _lib_plan(lib, 262144, 65536, 4, 64) == (16, 64, 2048)
    for bad in ((-1, 64, 1, 8), (10, 0, 1, 8), (10, 64, -1, 8), (10, 64, 1, 0), (10, 64, 1, 257)):
        assert lib.ranenv_ppo_spread_plan(*bad, None, None, None) == E_INVALID, bad


@pytest.mark.parametrize("slip", sp.SLIPS)
def test_planted_slips_of_the_geometry_are_caught(slip):
    """Tiles handed out in blocks instead of strided, a grid of ``slabs`` where a minibatch has fewer tiles, a tail minibatch counted
    as full: each leaves the library's figures or the header's walk on many of the 200 draws"""
    lib = _lib.load()
    caught = 0
    for n_rows, minibatch, epochs, slabs in _draws():
        wrong = sp.plan(n_rows, minibatch, epochs, slabs, slip) != _lib_plan(lib, n_rows, minibatch, epochs, slabs)
        sizes = {min(minibatch, n_rows), sp.minibatches(n_rows, minibatch)[-1]}
        for rows in sizes:
            wrong = wrong or bool(sp.walk_faults(sp.walk(rows, slabs, slip), rows, slabs))
        caught += wrong
        if slip == "tiles in blocks":          # (blocks and strides part exactly where a workgroup has a second tile and is not alone)
            assert wrong == any(1 < slabs < sp.tiles_of(rows) for rows in sizes), (n_rows, minibatch, slabs)
    print(f"{slip}: caught on {caught} of 200 draws")
    # (minibatches of at most 600 entries have at most 19 tiles: few draws have fewer slabs than that and more than one)
    assert caught >= (1 if slip == "tiles in blocks" else 20)


def test_spread_bytes_against_the_restated_formula_on_200_seeded_shapes():
    rng = np.random.default_rng(77)
    for i in range(200):
        hidden = [int(x) for x in rng.integers(1, 513, size=int(rng.integers(1, 5)))]
        hidden_c = [int(x) for x in rng.integers(1, 513, size=int(rng.integers(1, 5)))]
        n_in, n_out, slabs = int(rng.integers(1, 300)), int(rng.integers(1, 40)), int(rng.integers(1, sp.SLABS_MAX + 1))
        actor, critic = [n_in] + hidden + [n_out], ([n_in] + hidden_c + [1] if i % 5 else None)
        for wide in (False, True):
            assert be.ppo_spread_bytes(actor, critic, slabs, wide) == sp.spread_bytes(actor, critic, slabs, wide), (actor, critic, slabs, wide)
    # the reference's verybig inter pair at S 5: 64 slabs of its 1.15 M parameters
    verybig = ([50, 512, 512, 512, 10], [50, 512, 512, 512, 1])
    assert be.ppo_spread_bytes(*verybig, 64) == 4 * 64 * sum(sp.packed_floats(d) for d in verybig)
    assert be.ppo_spread_bytes(*verybig, 64, wide=True) - be.ppo_spread_bytes(*verybig, 64) == 4 * 64 * be.ppo_wide_scratch_floats(*verybig)
    lib, out = _lib.load(), C.c_int64(-7)
    actor = _lib.Mlp()
    actor.n_hidden, actor.dims[0], actor.dims[1], actor.dims[2] = 1, 50, 64, 10
    assert lib.ranenv_ppo_spread_bytes(None, None, 4, 0, C.byref(out)) == E_INVALID and out.value == -7
    assert lib.ranenv_ppo_spread_bytes(C.byref(actor), None, 0, 0, C.byref(out)) == E_INVALID and b"slabs 0" in lib.ranenv_last_error(None)
    assert lib.ranenv_ppo_spread_bytes(C.byref(actor), None, 257, 0, C.byref(out)) == E_INVALID and out.value == -7
    assert lib.ranenv_ppo_spread_bytes(C.byref(actor), None, 4, 2, C.byref(out)) == E_INVALID and b"wide 2" in lib.ranenv_last_error(None)
    assert lib.ranenv_ppo_spread_bytes(C.byref(actor), None, 4, 0, C.byref(out)) == 0 and out.value == sp.spread_bytes([50, 64, 10], None, 4, False)


def test_bind_spread_refuses_its_arguments_before_the_handle():
    lib = _lib.load()
    assert lib.ranenv_ppo_bind_spread(None, 0, 0, None) == E_INVALID and b"slabs 0 (1..256)" in lib.ranenv_last_error(None)
    assert lib.ranenv_ppo_bind_spread(None, 257, 0, None) == E_INVALID and b"slabs 257" in lib.ranenv_last_error(None)
    assert lib.ranenv_ppo_bind_spread(None, 64, 2, None) == E_INVALID and b"wide 2" in lib.ranenv_last_error(None)
    assert lib.ranenv_ppo_bind_spread(None, 64, 1, None) == E_INVALID and b"null handle" in lib.ranenv_last_error(None)


def test_order_firsts_under_the_spread_caps():
    """2^22 rows x epochs of one agent: refused under the default caps (one compute unit would walk them), taken under the spread
    binding's; the cap on optimiser steps holds under both"""
    n = 1 << 22
    order = {"order_inter": torch.zeros((1, n), dtype=torch.int32), "first_inter": np.array([0, n], dtype=np.int32)}
    with pytest.raises(be.RanEnvError) as e:
        be.ppo_order_firsts(order, {"inter": 1, "intra": 1}, 1, 65536)
    assert "rows x epochs" in str(e.value)
    firsts = be.ppo_order_firsts(order, {"inter": 1, "intra": 1}, 1, 65536, be.PPO_SPREAD_CAPS)
    assert firsts["inter"].tolist() == [0, n]
    assert be.PPO_SPREAD_CAPS[1] == be.PPO_STEPS_CAP
    with pytest.raises(be.RanEnvError) as e:
        be.ppo_order_firsts(order, {"inter": 1, "intra": 1}, 1, 64, be.PPO_SPREAD_CAPS)
    assert "optimiser steps" in str(e.value)


def test_ppo_bind_spread_excludes_mixed_head_and_per_slice():
    env = object.__new__(be.BatchedRanEnv)      # (refused before the handle is touched: no GPU needed)
    for other in ("mixed", "head", "per_slice"):
        with pytest.raises(ValueError) as e:
            env.ppo_bind(spread=True, **{other: True})
        assert "spread and " + other in str(e.value)
