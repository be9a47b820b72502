"""Member lines, the row's tail added by the owner (include/ranenv.h, "MEMBER LINES"): the clusters of the members step kernels walk
a row's whole-group lines only, and the lane that owns a member adds the row's last R mod 8 RBs itself, from its own tail line and
over its own RB range.  Every number of a rollout stays, bit for bit, what the whole-tile build (member_lines 0: lane = UE, no
lines, no clusters) gives: for the lean build of several TTIs and the streaming persistent build, on the directed scenarios of
tests/test_gpu_member_lines.py (member counts at the edges of a cluster and of a wave), at rows of one walked line + a tail of 4,
the headline's two leaves + 7, three leaves + 7 and four leaves + 3 -- with RB groups of one RB, so that ranges end anywhere.
The whole-tile run's own rb_start / rb_count show that the compared TTIs held what the owner's masked chain tells apart."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.gpu_common import need_gpu
from tests.test_gpu_member_lines import LEAN, PERSIST, _directed, _persist_batch, _same, _set, _snap

pytestmark = pytest.mark.gpu

MEMBERS = (1, 7, 8, 9, 63, 64, 65, 100)
ROWS = {12: (1, 2), 135: (2, 5), 263: (3, 9), 419: (4, 17)}        # R: (leaves, lines per UE in the copy)


def _kinds(views, tables, scen, R):
    """What the ranges of one TTI hold, per wave of 64 lanes (lane l of an env owns its l-th member in ascending UE order)."""
    tail = R % 8
    t0 = R - tail
    start, count = views["rb_start"].cpu().numpy(), views["rb_count"].cpu().numpy()
    seen = set()
    for b in range(start.shape[0]):
        member = np.flatnonzero(tables.ue_slice[scen[b]] >= 0)
        s, c = start[b][member].astype(np.int64), count[b][member].astype(np.int64)
        hold = c > 0
        if (hold & (s < t0) & (s + c > t0)).any():
            seen.add("straddles")
        if (hold & (s >= t0)).any():
            seen.add("inside")
        for w0 in range(0, member.size, 64):
            w = slice(w0, w0 + 64)
            if not (hold[w] & (s[w] + c[w] > t0)).any():
                seen.add("wave with holders, none reaching the tail" if hold[w].any() else "wave without a holder")
    return seen


@pytest.mark.parametrize("build", ["lean", "persist"])
@pytest.mark.parametrize("R", sorted(ROWS))
def test_owner_added_tail_equals_whole_tiles_bit_for_bit(R, build):
    need_gpu()
    from intent_radio_sched_multi_slice_amd import _lib
    from tests.member_lines_ref import leaves_of
    assert R % 8 != 0 and len(leaves_of(0, R)) == ROWS[R][0] and _lib.load().ranenv_member_line_plan(R, 0, None, None, None) == ROWS[R][1]
    dev = torch.device("cuda", 0)
    persistent = build == "persist"
    B = _persist_batch(128) if persistent else 24
    scen = np.arange(B) % len(MEMBERS)
    outs, seen = [], set()
    for ml in (0, 1):
        env, t = _directed(MEMBERS, R, B, dev)
        env.set_se_mode("stream")
        _set(env, PERSIST if persistent else LEAN, ml)
        env.reset()
        snaps = [_snap(env, t)]
        for k in (5, 9):
            env.rollout(k)
            snaps.append(_snap(env, t))
            assert env.get_option("last_rollout_member_lines") == ml
            assert env.get_option("last_rollout_persistent") == (1 if persistent else 0)
            if ml == 0:          # the precondition comes from the whole-tile run: the ranges the LAST TTI of the call summed over
                seen |= _kinds(snaps[-1][0], t, scen, R)
        if persistent:
            assert env.get_option("persist_errors") == 0
        outs.append(snaps)
        env.close()
    print("R", R, build, "the whole-tile run's ranges held:", sorted(seen))
    assert {"straddles", "inside"} <= seen and seen & {"wave with holders, none reaching the tail", "wave without a holder"}, (R, build, sorted(seen))
    for i, (a, b) in enumerate(zip(*outs)):
        _same(a, b, (R, build, i))
