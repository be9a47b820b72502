"""The serving order of member lines (include/ranenv.h, "MEMBER LINES"), host side: ranenv_member_serving_order restates what a
wave of the members step kernels computes after the allocation -- the lanes of the passes requested ahead keep their slot, behind
them the holders of an RB are served first, and the passes behind the last holder keep no masked sum.  Checked property by
property and against tests/member_order_ref.py.  No GPU.

"Slots of members are a permutation of 0 .. members-1" holds as stated when the members are the wave's first lanes (as they are in
an env); for any other pattern a prefix lane without a member keeps its slot too, so the statement that holds -- and implies the
first -- is: the slots are a permutation of the wave, and behind the prefix the members take the slots right behind it."""
import ctypes as C

import numpy as np
import pytest

from tests.member_order_ref import bits, serving_order

DQ = 4
ALL = (1 << 64) - 1


@pytest.fixture(scope="module")
def lib():
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.csrc import build
    build.build()
    return _lib.load()


def first(n):
    return (1 << n) - 1


def call(lib, member, holder, nl, dq=DQ):
    slots = np.full(66, -7, dtype=np.int32)
    mp = C.c_int32(-7)
    rc = lib.ranenv_member_serving_order(member, holder, nl, dq, slots[1:].ctypes.data_as(C.POINTER(C.c_int32)), C.byref(mp))
    assert slots[0] == -7 and slots[65] == -7          # nothing written around the 64 slots
    return rc, slots[1:65].astype(np.int64), mp.value


def directed(nl, rng):
    pre = 8 * -(-DQ // nl)
    out = [(0, 0), (1, 0), (1, 1), (1 << 37, 1 << 37)]                                  # no member; one member (first lane, another lane)
    for n in (8, 9, 63, 64):
        m = first(n)
        some = int(rng.integers(0, 1 << 63)) & m
        out += [(m, 0), (m, m), (m, some), (m, m & first(pre)), (m, m & ~first(max(n - 5, 0)))]   # no holder, all, random, in the prefix only, last lanes only
    for m in (first(20) << 30, first(64) & ~first(40), 0x5555555555555555, (first(10) << 3) | (first(7) << 50)):   # members that are not the first lanes
        out += [(m, 0), (m, m), (m, int(rng.integers(0, 1 << 63)) & m)]
    return out


def check(lib, member, holder, nl):
    rc, slots, mp = call(lib, member, holder, nl)
    assert rc == 0, (hex(member), hex(holder), nl)
    m, h = bits(member), bits(holder)
    pre = 8 * -(-DQ // nl)
    lanes = np.arange(64)
    behind = lanes >= pre
    tag = (hex(member), hex(holder), nl)
    assert sorted(slots.tolist()) == list(range(64)), tag                                # a permutation of the wave
    assert (slots[:pre] == lanes[:pre]).all(), tag                                       # the prefix lanes keep their lane number
    n_behind = int((m & behind).sum())
    assert sorted(slots[m & behind].tolist()) == list(range(pre, pre + n_behind)), tag   # members: the slots right behind the prefix
    if member == first(int(m.sum())):
        assert sorted(slots[m].tolist()) == list(range(int(m.sum()))), tag               # ... so, in an env: a permutation of 0 .. members-1
    hs, ns, os_ = slots[h & behind], slots[m & ~h & behind], slots[~m & behind]
    if hs.size and ns.size:
        assert hs.max() < ns.min(), tag                                                  # every holder in front of every non-holder
    if n_behind and os_.size:
        assert slots[m & behind].max() < os_.min(), tag                                  # lanes without a member behind the last member
    for grp in (hs, ns, os_):
        assert (np.diff(grp) > 0).all(), tag                                             # lane order inside each group
    top = int(lanes[m].max()) + 1 if m.any() else 0
    passes = -(-top // 8)
    need = min(pre // 8, passes)                                                         # the prefix (what of it the wave walks)
    if hs.size:
        need = max(need, int(hs.max()) // 8 + 1)                                         # ... and every holder
    assert mp == need and mp <= passes, (tag, mp, need, passes)
    want_slots, want_mp, _, _ = serving_order(member, holder, nl, DQ)
    assert (slots == want_slots).all() and mp == want_mp, tag


@pytest.mark.parametrize("nl", [1, 2, 5, 14])
def test_serving_order_directed_masks(lib, nl):
    rng = np.random.default_rng(40 + nl)
    for member, holder in directed(nl, rng):
        check(lib, member, holder, nl)


@pytest.mark.parametrize("nl", [1, 2, 5, 14])
def test_serving_order_random_masks(lib, nl):
    rng = np.random.default_rng(90 + nl)
    for trial in range(300):
        if trial % 2:                      # an env's shape: the first n lanes, holders with a density drawn per trial
            member = first(int(rng.integers(0, 65)))
        else:
            member = int(rng.integers(0, 1 << 63)) | (int(rng.integers(0, 2)) << 63)
        p = rng.random()
        holder = sum(1 << l for l in range(64) if (member >> l) & 1 and rng.random() < p)
        check(lib, member, holder, nl)


def test_prefix_sizes(lib):
    """R = 135: 5 lines, one pass ahead; a one-line row: four passes, half the wave."""
    for nl, pre in ((5, 8), (14, 8), (4, 8), (3, 16), (2, 16), (1, 32)):
        _, slots, _ = call(lib, ALL, ALL & ~first(48), nl)
        assert (slots[:pre] == np.arange(pre)).all() and slots[48] == pre, (nl, slots)


def test_serving_order_refuses_bad_arguments(lib):
    slots = (C.c_int32 * 64)()
    mp = C.c_int32()
    assert lib.ranenv_member_serving_order(3, 1, 5, 4, None, C.byref(mp)) < 0
    assert lib.ranenv_member_serving_order(3, 1, 5, 4, slots, None) < 0
    assert lib.ranenv_member_serving_order(3, 1, 0, 4, slots, C.byref(mp)) < 0
    assert lib.ranenv_member_serving_order(3, 1, 5, 0, slots, C.byref(mp)) < 0
    assert lib.ranenv_member_serving_order(3, 4, 5, 4, slots, C.byref(mp)) < 0           # a holder that is no member
    assert lib.ranenv_member_serving_order(3, 1, 1, 72, slots, C.byref(mp)) < 0          # a prefix beyond the wave
    assert lib.ranenv_member_serving_order(3, 1, 5, 4, slots, C.byref(mp)) == 0
