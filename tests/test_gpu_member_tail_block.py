"""The packed member-lines copy on the device (include/ranenv.h, "MEMBER LINES": the handle's copy): per tile the whole-group lines
[U][nlw][32], then one tail block [U][8] -- a 32-byte slot per UE instead of a 128-byte tail line per UE.  The packed retile is an
index transform of the pool (compared as bits against a numpy layout; bytes behind the block inside the tile stride are +0.0, and
nothing outside the tiles is written), and every number of a rollout stays, bit for bit, what the whole-tile build (member_lines 0)
gives: lean and persistent builds, member counts at the edges of a cluster and of a wave, rows of the block only (R 5), one walked
line + a tail of 4 (12), the headline's row (135) and three leaves (263), one env on the pool's last tile, and a shape whose tile
stride carries padding (U 25)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.gpu_common import need_gpu
from tests.member_tail_block_ref import lay_out_pool_packed, packed_layout
from tests.test_gpu_member_lines import LEAN, PERSIST, SHAPES, _directed, _persist_batch, _same, _set, _snap, _walk
from tests.test_gpu_member_tail import _kinds

pytestmark = pytest.mark.gpu

MEMBERS = (1, 7, 8, 9, 63, 64, 65, 100)
ROWS = {5: 0, 12: 1, 135: 4, 263: 8}          # R: the lines per UE the clusters walk


@pytest.mark.parametrize("quad", [0, 1])
@pytest.mark.parametrize("U,R", [(100, 135), (25, 135), (7, 5), (33, 8), (64, 130), (40, 419)])
def test_packed_retile_is_an_index_transform(U, R, quad):
    need_gpu()
    from intent_radio_sched_multi_slice_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    n = 5
    g = torch.Generator(device=dev); g.manual_seed(U * 1000 + R)
    rb = torch.rand((n, R, U), generator=g, device=dev, dtype=torch.float32)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    src, stride = rb, R * U
    if quad:
        Rq = (R + 3) // 4
        src = torch.empty((n, Rq, U, 4), device=dev, dtype=torch.float32)
        assert lib.ranenv_se_retile_quad(C.c_void_p(rb.data_ptr()), C.c_void_p(src.data_ptr()), n, U, R, stream) == 0
        stride = Rq * U * 4
    nlw, off, nbytes = C.c_int32(), C.c_int64(), C.c_int64()
    assert lib.ranenv_member_lines_packed_layout(U, R, C.byref(nlw), C.byref(off), C.byref(nbytes)) == 0
    assert (nlw.value, off.value, nbytes.value) == packed_layout(U, R)
    per = nbytes.value // 4
    guard = 64                                    # floats behind the last tile: nobody's, they keep their -1.0
    out = torch.full((n * per + guard,), -1.0, device=dev, dtype=torch.float32)
    assert lib.ranenv_se_retile_member_lines_packed(C.c_void_p(src.data_ptr()), quad, stride, C.c_void_p(out.data_ptr()), n, U, R, stream) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = lay_out_pool_packed(rb.cpu().numpy())
    assert want.shape == (n, per)
    assert np.array_equal(got[:n * per].reshape(n, per).view(np.int32), want.view(np.int32))        # (bits: every padding float is +0.0)
    assert (got[n * per:] == -1.0).all()


def _compare(R, build, make):
    """member_lines 0 against 1 after reset and after rollouts of 5 and 9 TTIs; returns what the whole-tile run's ranges held."""
    persistent = build == "persist"
    outs, seen = [], set()
    for ml in (0, 1):
        env, t, scen = make()
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
    for i, (a, b) in enumerate(zip(*outs)):
        _same(a, b, (R, build, i))
    return seen


@pytest.mark.parametrize("build", ["lean", "persist"])
@pytest.mark.parametrize("R", sorted(ROWS))
def test_tail_block_equals_whole_tiles_bit_for_bit(R, build):
    """The directed scenarios of tests/test_gpu_member_lines.py (1 .. 100 members), the last env on the pool's last tile."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd import _lib
    lib = _lib.load()
    nlw, off, nbytes = C.c_int32(), C.c_int64(), C.c_int64()
    assert lib.ranenv_member_lines_packed_layout(100, R, C.byref(nlw), C.byref(off), C.byref(nbytes)) == 0
    assert R % 8 != 0 and nlw.value == ROWS[R] and nbytes.value == 100 * (nlw.value * 128 + 32)
    dev = torch.device("cuda", 0)
    B = _persist_batch(128) if build == "persist" else 24
    scen = np.arange(B) % len(MEMBERS)

    def make():
        env, t = _directed(MEMBERS, R, B, dev)          # (last_tile_env: env B - 1 starts at the pool's last tile)
        return env, t, scen

    seen = _compare(R, build, make)
    print("R", R, build, "the whole-tile run's ranges held:", sorted(seen))
    no_tail_wave = seen & {"wave with holders, none reaching the tail", "wave without a holder"}
    if R < 8:
        # the whole row IS the tail: R - tail = 0, no range starts in front of it, so nothing can straddle it and every holder is inside
        assert "inside" in seen and "wave without a holder" in seen, (R, build, sorted(seen))
    else:
        assert {"straddles", "inside"} <= seen and no_tail_wave, (R, build, sorted(seen))


@pytest.mark.parametrize("build", ["lean-1", "lean-3", "persist"])
def test_a_tile_stride_with_padding(build):
    """U 25, R 135: 12 800 bytes of walk lines + an 800-byte block, the tile stride rounded up to 13 696."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    from tests.test_gpu_member_lines import CALLS
    kw = SHAPES[1]
    assert packed_layout(kw["n_ues"], kw["n_rbs"]) == (4, 12800, 13696)
    dev = torch.device("cuda", 0)
    persistent = build == "persist"
    B = _persist_batch(64) if persistent else 300
    outs = []
    for ml in (0, 1):
        wl = make_mult_slice_workload(B, dev, n_scenarios=12, n_traces=6, trace_len=20, max_steps=1000, **kw)
        snaps, used = _walk(wl, PERSIST if persistent else LEAN, ml, 1 if persistent else int(build[-1]), persistent)
        assert used == [ml if (persistent or k > 1) else 0 for k in CALLS], (build, ml, used)
        if persistent:
            assert wl.env.get_option("persist_errors") == 0
        outs.append(snaps)
        wl.env.close()
    for i, (a, b) in enumerate(zip(*outs)):
        _same(a, b, (build, i))
