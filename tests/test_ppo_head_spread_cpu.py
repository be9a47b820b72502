"""The spread form of the head binding without a GPU: the two new exports in the header, the ctypes table and the built library; the byte
formula (ranenv_ppo_head_spread_bytes) against its restatement on 200 seeded shapes, with two planted slips of the formula shown to be
caught; what the entries refuse before they touch a handle; and the argument checks of ``ppo_bind`` and the caps of ``ppo_update_head``."""
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

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = {"ranenv_ppo_bind_head_spread": 3, "ranenv_ppo_head_spread_bytes": 5}
E_INVALID = -1
SLIPS = ("log_std partials as float32", "no log_std partials")


def head_spread_bytes(actor, critic, S, slabs, slip=None):
    """The header's words: slabs x (4 x (actor floats + critic floats) + 8 x S)"""
    per_slab = 4 * (sp.packed_floats(actor) + sp.packed_floats(critic))
    per_slab += {None: 8 * S, SLIPS[0]: 4 * S, SLIPS[1]: 0}[slip]
    return slabs * per_slab


def _shapes():
    rng = np.random.default_rng(4711)
    for _ in range(200):
        S = int(rng.integers(1, 17))
        hidden = [int(x) for x in rng.integers(1, 513, size=int(rng.integers(1, 5)))]
        hidden_c = [int(x) for x in rng.integers(1, 513, size=int(rng.integers(1, 5)))]
        yield [10 * S] + hidden + [S], [10 * S] + hidden_c + [1], S, int(rng.integers(1, sp.SLABS_MAX + 1))


def test_header_binding_and_library_agree_on_the_new_exports():
    hdr = open(os.path.join(REPO, "include", "ranenv.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name, n_args in NEW_EXPORTS.items():
        proto = re.search(r"^int " + name + r"\(([^;]*)\);", hdr, re.M | re.S)
        assert proto, f"{name} is not declared in include/ranenv.h"
        assert len(proto.group(1).split(",")) == n_args, name
        assert name in _lib.EXPORTS and len(_lib.FUNCTIONS[name][1]) == n_args and hasattr(lib, name), name
    assert "Head policies over the chip" in hdr


def test_head_spread_bytes_against_the_restated_formula_on_200_seeded_shapes():
    for actor, critic, S, slabs in _shapes():
        assert be.ppo_head_spread_bytes(actor, critic, S, slabs) == head_spread_bytes(actor, critic, S, slabs), (actor, critic, S, slabs)
    # SB3's default pair at S 5 under 64 slabs: 64 x (4 x (64 x 64 + 64 + 64 x 64 + 64 + 32 x 64 + 32) x 2 + 8 x 5)
    sb3 = ([50, 64, 64, 5], [50, 64, 64, 1])
    assert be.ppo_head_spread_bytes(*sb3, 5, 64) == 64 * (4 * 2 * (2 * (64 * 64 + 64) + 32 * 64 + 32) + 40)
    assert be.ppo_head_spread_bytes(*sb3, 5, 64) - be.ppo_spread_bytes(*sb3, 64) == 64 * 8 * 5      # (the IBSched form's slabs, plus gls)


@pytest.mark.parametrize("slip", SLIPS)
def test_planted_slips_of_the_byte_formula_are_caught(slip):
    caught = sum(be.ppo_head_spread_bytes(a, c, S, slabs) != head_spread_bytes(a, c, S, slabs, slip) for a, c, S, slabs in _shapes())
    assert caught == 200, f"{slip}: caught on {caught} of 200 shapes"


def test_the_entries_refuse_their_arguments_before_a_handle():
    lib, out = _lib.load(), C.c_int64(-7)
    actor, critic = _lib.Mlp(), _lib.Mlp()
    actor.n_hidden, actor.dims[0], actor.dims[1], actor.dims[2] = 1, 50, 64, 5
    critic.n_hidden, critic.dims[0], critic.dims[1], critic.dims[2] = 1, 50, 64, 1
    a, c = C.byref(actor), C.byref(critic)
    assert lib.ranenv_ppo_head_spread_bytes(None, c, 5, 4, C.byref(out)) == E_INVALID and out.value == -7
    assert lib.ranenv_ppo_head_spread_bytes(a, None, 5, 4, C.byref(out)) == E_INVALID and out.value == -7
    assert lib.ranenv_ppo_head_spread_bytes(a, c, 5, 4, None) == E_INVALID
    for slabs in (0, 257, -3):
        assert lib.ranenv_ppo_head_spread_bytes(a, c, 5, slabs, C.byref(out)) == E_INVALID and out.value == -7
        assert f"slabs {slabs} (1..256)".encode() in lib.ranenv_last_error(None)
        assert lib.ranenv_ppo_bind_head_spread(None, slabs, None) == E_INVALID and f"slabs {slabs} (1..256)".encode() in lib.ranenv_last_error(None)
    for S in (0, 17):
        assert lib.ranenv_ppo_head_spread_bytes(a, c, S, 4, C.byref(out)) == E_INVALID and f"n_slices {S}".encode() in lib.ranenv_last_error(None)
    assert lib.ranenv_ppo_head_spread_bytes(a, c, 5, 4, C.byref(out)) == 0 and out.value == head_spread_bytes([50, 64, 5], [50, 64, 1], 5, 4)
    assert lib.ranenv_ppo_bind_head_spread(None, 64, None) == E_INVALID and b"null handle" in lib.ranenv_last_error(None)


class _Refused(Exception):
    pass


class _NoLibrary:
    """Stands where the library would: every entry reached is an error of the test"""
    def __getattr__(self, name):
        raise _Refused(name)


def test_ppo_bind_checks_the_head_combinations_before_the_handle():
    env = object.__new__(be.BatchedRanEnv)      # (refused before the handle is touched: no GPU needed)
    for kw, word in ((dict(head=True, spread=True, wide=True), "head, spread and wide"), (dict(head=True, wide=True), "wide and head"),
                     (dict(head=True, mixed=True), "mixed and head"), (dict(head=True, per_slice=True), "per_slice excludes"),
                     (dict(head=True, spread=True, mixed=True), "spread and mixed"), (dict(head=True, spread=True, per_slice=True), "spread and per_slice")):
        for slabs in (dict(), dict(slabs=64)):
            with pytest.raises(ValueError) as e:
                env.ppo_bind(**kw, **slabs)
            assert word in str(e.value), kw
    with pytest.raises(ValueError) as e:        # (slabs has no default in the head binding's spread form)
        env.ppo_bind(head=True, spread=True)
    assert "spread and head" in str(e.value) and "slabs" in str(e.value)
    assert not hasattr(env, "_ppo_spread") and not hasattr(env, "_ppo_head_spread")


def test_update_head_drops_the_row_cap_under_the_spread_head_binding_alone():
    """The caps are checked before the library is reached: under the plain head binding 2^21 rows x epochs are refused; under the spread
    one they pass the cap and go on to the record and the library (which this test does not have); the cap on optimiser steps holds under both"""
    n = 1 << 21
    order = torch.zeros((1, n), dtype=torch.int32)
    for spread in (False, True):
        env = object.__new__(be.BatchedRanEnv)
        env.device, env._lib, env._ppo_head_spread = torch.device("cpu"), _NoLibrary(), spread
        if spread:
            with pytest.raises((_Refused, KeyError)):      # (past the caps: the empty record, or the library, is what the call misses next)
                env.ppo_update_head({}, epochs=1, minibatch=65536, order=order)
        else:
            with pytest.raises(be.RanEnvError, match="rows x epochs"):
                env.ppo_update_head({}, epochs=1, minibatch=65536, order=order)
        few = order if spread else order[:, :1 << 19].contiguous()      # (the plain binding: under its row cap, 16 384 steps of 32 rows)
        with pytest.raises(be.RanEnvError, match="optimiser steps"):
            env.ppo_update_head({}, epochs=1, minibatch=32, order=few)
