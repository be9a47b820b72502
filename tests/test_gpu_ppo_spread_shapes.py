"""The SPREAD binding of the PPO update (ranenv_ppo_bind_spread; the pass, reduce and apply kernels of ranenv_ppo_spread.hip) across net
shapes and slab counts -- what tests/test_gpu_ppo_spread.py checks on one workload, two narrow nets and at most 32 slabs, here on the
spread grid of tests/ppo_bindings_shapes_ref.py (``bs``):

    the shape grid   ONE agent of ref.SHAPES A..F and of ``lopsided`` (A's inter pair beside a [24] intra pair) at B 12, T 8: one slab
                     against the plain binding byte for byte, three slabs against the float64 twin, one Adam step, the layout.  What
                     the grid covers by its reduce / apply block counts is asserted from the device's own float counts.
    wide             ``past_limit`` and ``deepest`` under spread + wide against the twin; refused without ``wide``
    all 256 slabs    [24] nets on 16 896 inter rows: one minibatch of 528 tiles, then an epoch of two (264 tiles each) whose statistics
                     pass through the running sums that lie behind wstat[255]
    exact reduce     128 and 256 rows at 4 slabs: dev_grad is, byte for byte, the plain binding's four per-slab gradients added in
                     ascending slab order in float32 -- and not those added in descending order
    one kind alone   an update without intra lists, and one whose intra list is empty
    rebinding        shape A at 3 slabs, then [24] nets at 5 slabs on the same handle, against a fresh handle

Comparisons and tolerances are tests/ppo_update_ref.py's: the gradient per layer tensor within 8x the float32-torch error of the float64
twin (floor 1e-6 relative), statistics 1e-6, Adam 4 float32 ulp of adam_step_f32 on the call's own dev_grad, the norm 1e-9, byte
equality wherever two paths promise the same adds.

Measured on one MI355X (printed by the tests):
    3 slabs, worst tensor's error / float32 twin's (bound 8): A 0.584, B 0.284, C 0.635, D 0.825, E 0.472, F 0.787, lopsided 0.441;
    spread + wide: past_limit 0.304, deepest 0.665; 256 slabs, one minibatch of 16 896 rows: 0.488, the last call 0.525; the five statistics within
    2.2e-7 of the twin everywhere (bound 1e-6); the epoch of two minibatches under 256 slabs: within 2.2e-9
    one Adam step at 3 slabs (weights / moments): 0 / 0 ulp on all seven grid cases
    reduce / apply blocks (inter, intra): A 613, 581; B 50, 30; C 51, 30; D 11, 11; E 98, 98; F 103, 85; lopsided 613, 5
    exact reduce, ulp distance of dev_grad to the ascending float32 restatement: 0 on every element of both kinds at 128 and at 256
    rows (tanh40x24: 14 592 floats per kind, E: 100 256); the descending restatement differs in 1508 .. 1984 elements (tanh40x24) and in
    16 886 .. 23 430 (E)"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import ppo_bindings_shapes_ref as bs
from tests import ppo_spread_ref as sp
from tests import ppo_update_ref as ref
from tests import ppo_wide_ref as wd
from tests.gpu_common import _ordered, need_gpu, shaped_workload

pytestmark = pytest.mark.gpu

E_STATE = -3
ALL, B, T = ref.ALL, bs.SPREAD_B, bs.SPREAD_T
GRID = bs.SPREAD_SHAPES + (bs.LOPSIDED,)
HP_LOOP = dict(lr=2e-3, clip=0.2, vf_coeff=0.5, ent_coeff=0.01, grad_clip=0.5)
STAT_NAMES = ("policy_loss", "value_loss", "entropy", "kl", "clip_frac")
ONE = dict(epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, grad=True)


def _env(case, batch=B, **bind):
    """A reset env under ONE agent of the case's nets, bound as ``bind`` says (empty: the plain binding).  The cases of ref.SHAPES and
    ``lopsided`` run on ``shaped_workload(S, Us, batch)``, those of ref.CASES and wd.BEYOND on ``ref.native_workload(batch)``."""
    need_gpu()
    S, Us, layout = bs.spread_spec(case)[:3]
    if case in GRID:
        env = shaped_workload(S, Us, batch, seed=40 + GRID.index(case)).env
    else:
        env = ref.native_workload(batch)
    nets = bs.spread_nets(case)
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=ref.SEED, intra_input=layout)
    env.set_value_network(nets["v_inter"], nets["v_intra"])
    env.ppo_bind(**bind)
    env.reset()
    return env


def _record(env, n_steps=T, full=True):
    """collect(); for S > 1 the record holds masked sorted positions and -- ``full``: on ``shaped_workload``; every env of
    ``ref.native_workload`` plays a scenario with an inactive slice -- rows with every position unmasked, for S 1 every row is active"""
    rec = env.collect(n_steps)
    torch.cuda.synchronize()
    n_act = (rec["mask_inter"] != 0).sum(dim=2)
    if env.S > 1:
        assert 1 <= int(n_act.min()) < env.S, int(n_act.min())
        assert int(n_act.max()) == env.S or not full, int(n_act.max())
    else:
        assert bool((n_act == 1).all())
    return rec


def _twin_records(env_a, env_b, n_steps=T, full=True):
    rec_a, rec_b = _record(env_a, n_steps, full), _record(env_b, n_steps, full)
    for k in rec_a:
        assert torch.equal(rec_a[k], rec_b[k]), k
    return rec_a, rec_b


def _order(rec, epochs, seed=3, batch=B):
    from intent_radio_sched_multi_slice_amd.adapters import ppo_row_order
    return ppo_row_order(rec, [0, batch], epochs, seed)


def _cut(order, n):
    """The first n entries of the first epoch's list of both kinds"""
    out = {}
    for kind in ("inter", "intra"):
        assert int(order["first_" + kind][1]) >= n
        out["order_" + kind], out["first_" + kind] = order["order_" + kind][:1, :n].contiguous(), np.array([0, n], dtype=np.int32)
    return out


def _twin_args(case):
    _, _, layout, aa, ca, _ = bs.spread_spec(case)
    return aa, ca, layout


# ---- 1. the shape grid ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GRID)
def test_one_slab_gives_the_plain_bindings_gradient_bit_for_bit(case):
    """slabs=1 on every shape: one minibatch of all rows at lr 0, and lists cut to 33 and 65 rows (a tile and one row, two and one):
    dev_grad of both kinds equals the plain twin handle's byte for byte"""
    env_s, env_p = _env(case, spread=True, slabs=1), _env(case)
    rec_s, rec_p = _twin_records(env_s, env_p)
    order = _order(rec_s, 1)
    assert int(order["first_inter"][1]) == T * B and int(order["first_intra"][1]) >= 65
    for what, lst in [("all rows", order)] + [(f"{n} rows", _cut(order, n)) for n in (33, 65)]:
        out_s, out_p = env_s.ppo_update(rec_s, order=lst, **ONE), env_p.ppo_update(rec_p, order=lst, **ONE)
        assert torch.equal(out_s["grad"], out_p["grad"]), f"{case}, {what}: dev_grad differs from the plain binding's"
        assert bool(out_s["grad"][0, 0].any()) and bool(out_s["grad"][0, 1].any())
        assert np.array_equal(out_s["rows"], out_p["rows"]) and np.array_equal(out_s["minibatches"], out_p["minibatches"])
    env_s.close()
    env_p.close()


@pytest.mark.parametrize("case", GRID)
def test_three_slabs_against_the_float64_twin(case):
    """One minibatch of all rows at lr 0 (the inter kind: three tiles, one per slab; the intra kind: a slab walks several): dev_grad per
    layer tensor within 8x the float32-torch yardstick of the float64 twin, the statistics within 1e-6"""
    env = _env(case, spread=True, slabs=3)
    rec = _record(env)
    order = _order(rec, 1)
    out = env.ppo_update(rec, order=order, **ONE)
    worst, misses = ref.check_against_twin(rec, order, out, ref.weights(env, 1), range(1), f"spread {case}, 3 slabs", *_twin_args(case))
    assert 0.0 < worst <= 8.0
    assert not misses, misses
    assert env.S == 1 or sp.tiles_of(int(order["first_intra"][1])) > 3, "a slab of the intra kind walks a second tile"
    env.close()


@pytest.mark.parametrize("case", GRID)
def test_one_adam_step_at_three_slabs(case):
    env = _env(case, spread=True, slabs=3)
    rec = _record(env)
    order = _order(rec, 1)
    w0 = ref.weights(env, 1)
    hp = dict(lr=np.array([1e-3]), grad_clip=np.array([0.05]), betas=(0.9, 0.999), eps=1e-8)
    out = env.ppo_update(rec, epochs=1, minibatch=ALL, order=order, grad=True, **hp)
    w1 = ref.weights(env, 1)
    ref.check_adam_step(env, out, w0, w1, hp, 1, f"spread {case}, 3 slabs")
    for r in ref.ROLES:
        assert all(not np.array_equal(x[0], y[0]) for x, y in zip(w0[r][0], w1[r][0])), f"a layer of {r} did not move"
    env.close()


def test_the_layout_is_the_formula_and_the_grid_covers_what_it_claims():
    """``ppo_member_layout`` of every grid case under the spread binding: the pair's packed floats and LDS bytes by the restated
    formulas.  From those floats: the grid holds a kind with the fewest reduce / apply blocks a pair can have (5; a padded layer alone
    is 1056 floats, so no kind has one block), a kind with more than 256 blocks (shape A), a case whose kinds' block counts differ by
    more than 10x, and an actor / critic boundary that is no multiple of PPO_SPREAD_BLOCK."""
    floats = {}
    for case in GRID:
        env = _env(case, spread=True, slabs=3)
        for kind, (a, c) in bs.spread_spec(case)[5].items():
            lay = env.ppo_member_layout(0, kind)
            assert (lay["actor"], lay["critic"]) == (sp.packed_floats(a), sp.packed_floats(c)), (case, kind)
            assert lay["lds_bytes"] == ref.pair_lds_bytes(a, c) <= ref.LDS_MAX, (case, kind)
            floats[case, kind] = (lay["actor"], lay["actor"] + lay["critic"])
        assert floats[case, "inter"] == bs.kind_floats(case)["inter"] and floats[case, "intra"] == bs.kind_floats(case)["intra"]
        env.close()
    blocks = {k: bs.blocks_of(f) for k, (_, f) in floats.items()}
    print("reduce / apply blocks per (case, kind):", blocks)
    assert min(blocks.values()) == bs.MIN_PAIR_BLOCKS == blocks[bs.LOPSIDED, "intra"]
    assert blocks["A", "inter"] > 256 and blocks["A", "intra"] > 256
    assert any(max(blocks[c, "inter"], blocks[c, "intra"]) > 10 * min(blocks[c, "inter"], blocks[c, "intra"]) for c in GRID)
    assert any(af % bs.SPREAD_BLOCK != 0 for af, _ in floats.values())


# ---- 2. wide beyond the plan ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bs.SPREAD_BEYOND)
def test_beyond_the_plan_under_spread_and_wide_against_the_float64_twin(case):
    """3 slabs, one minibatch of all rows at lr 0: dev_grad within 8x the float32-torch yardstick of the float64 twin, the statistics
    within 1e-6; without ``wide`` the pair is refused as ppo_bind refuses it"""
    widths, _, layout = wd.BEYOND[case]
    env = _env(case, spread=True, slabs=3, wide=True)
    rec = _record(env, full=False)
    order = _order(rec, 1)
    out = env.ppo_update(rec, order=order, **ONE)
    worst, misses = ref.check_against_twin(rec, order, out, ref.weights(env, 1), range(1), f"spread {case}, 3 slabs, wide", *_twin_args(case))
    assert 0.0 < worst <= 8.0
    assert not misses, misses
    for kind, dims in wd.kind_dims(widths, layout).items():
        assert env.ppo_member_layout(0, kind)["lds_bytes"] == wd.wide_lds_bytes(*dims)
    code, text = ref.refusal(lambda: env.ppo_bind(spread=True, slabs=3))
    need = ref.lds_bytes(ref.S, ref.US, layout, widths, widths)
    assert need > ref.LDS_MAX and code == E_STATE and "LDS" in text and str(need) in text, text
    env.close()


# ---- 3. all 256 slabs -----------------------------------------------------------------------------------------------------------------
def test_all_256_slabs_and_a_second_minibatch_that_reads_the_running_sums_behind_them():
    """[24] relu nets on the native workload at B 96, T 176: 16 896 inter rows.  As ONE minibatch (528 tiles) 256 pass workgroups run,
    each walks two or three tiles, and the last writes the last entry of wstat[256]: gradient and statistics of both kinds against the
    twin, ``rows`` exact.  Then one real step, and at the new weights an lr 0 call of ONE epoch in minibatches of 8448 rows -- two of
    264 tiles for the inter kind, more for the intra kind, every one on all 256 slabs.  ``run``, the epoch's running sums, lies right
    behind wstat[255] in the same allocation and is stored by every step but an epoch's last and read by every step but its first
    (``ppo_spread_stats``): the pass of step 1 writes wstat[255] between the two, so a write that reached into ``run`` leaves the
    epoch's statistics, which are held to the twin's at 1e-6 with ``rows`` and ``minibatches`` exact.  A last call of one minibatch
    against the twin again: slabs that a step left unzeroed would show in its gradient."""
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.adapters import ppo_update_reference
    case, batch, n_steps, mb = "relu24", bs.ALL_SLABS_B, bs.ALL_SLABS_T, bs.ALL_SLABS_MB
    env = _env(case, batch=batch, spread=True, slabs=sp.SLABS_MAX)
    rec = _record(env, n_steps, full=False)
    order = _order(rec, 1, batch=batch)
    n_inter, n_intra = int(order["first_inter"][1]), int(order["first_intra"][1])
    assert n_inter == batch * n_steps == 2 * mb and n_intra > n_inter
    lib, steps, grid, tail = _lib.load(), C.c_int64(), C.c_int32(), C.c_int32()
    for n in (n_inter, n_intra):
        assert lib.ranenv_ppo_spread_plan(n, ALL, 1, sp.SLABS_MAX, C.byref(steps), C.byref(grid), C.byref(tail)) == 0
        assert (steps.value, grid.value) == (1, 256) and tail.value == sp.tiles_of(n) >= 2 * 264
        walk = sp.walk(n, sp.SLABS_MAX)
        assert len(walk) == 256 and min(len(t) for t in walk) >= 2, "every slab is used, and every workgroup walks a second tile"
        assert lib.ranenv_ppo_spread_plan(n, mb, 1, sp.SLABS_MAX, C.byref(steps), C.byref(grid), C.byref(tail)) == 0
        assert steps.value == -(-n // mb) >= 2 and grid.value == 256, "a second minibatch on all 256 slabs"
    args = (range(1), )
    out = env.ppo_update(rec, order=order, **ONE)
    worst, misses = ref.check_against_twin(rec, order, out, ref.weights(env, 1), *args, "relu24, 256 slabs", *_twin_args(case))
    assert 0.0 < worst <= 8.0
    assert not misses, misses
    assert out["rows"][0, 0, 0] == n_inter and out["rows"][0, 1, 0] == n_intra
    env.ppo_update(rec, epochs=1, minibatch=ALL, order=order, **HP_LOOP)
    w1 = ref.weights(env, 1)
    # one epoch of several minibatches at lr 0: the epoch's statistics pass through ``run`` behind wstat[255]
    out = env.ppo_update(rec, epochs=1, minibatch=mb, lr=0.0, grad_clip=None, order=order)
    aa, ca, layout = _twin_args(case)
    host = {k: v.cpu() for k, v in rec.items()}
    misses = []
    for kind_i, (kind, n) in enumerate((("inter", n_inter), ("intra", n_intra))):
        twin = ppo_update_reference(host, kind, ref.as_torch(w1[kind][0]), ref.as_torch(w1["v_" + kind][0]), order["order_" + kind].cpu(), 0, n, epochs=1,
                                    minibatch=mb, lr=0.0, grad_clip=0.0, act_actor=aa, act_critic=ca, layout=layout)["stats"]
        assert out["rows"][0, kind_i, 0] == twin[0, 6] == n and out["minibatches"][0, kind_i, 0] == twin[0, 7] == -(-n // mb) >= 2
        for i, name in enumerate(STAT_NAMES):
            got, want = out[name][0, kind_i, 0], twin[0, i]
            print(f"relu24, 256 slabs, minibatches of {mb} {kind} {name}: device {got:.9g} twin {want:.9g}")
            if not abs(got - want) <= 1e-6 * max(1.0, abs(want)):
                misses.append(f"{kind} {name}: device {got:.9g}, twin {want:.9g}")
    assert not misses, misses
    out = env.ppo_update(rec, order=order, **ONE)
    worst, misses = ref.check_against_twin(rec, order, out, w1, *args, "relu24, 256 slabs, the last call", *_twin_args(case))
    assert 0.0 < worst <= 8.0
    assert not misses, misses
    assert out["rows"][0, 0, 0] == n_inter and out["minibatches"][0, 1, 0] == 1
    t = ref.state(env, 1)
    assert int(t["inter/0/t"][0]) == 3 + 2 and int(t["intra/0/t"][0]) == 3 + -(-n_intra // mb)
    env.close()


# ---- 4. the exact reduce ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bs.EXACT_CASES)
def test_the_reduce_adds_the_slabs_in_ascending_order_to_the_byte(case):
    """Lists of exactly 128 rows per kind (one tile per slab) and of exactly 256 (slab w walks tiles w and w + 4) at 4 slabs, lr 0,
    advantages as given.  A twin handle under the plain binding runs one call per slab on that slab's rows in walk order: its dev_grad
    g_w carries the row weight 1 / 32 (1 / 64), the spread call's rows 1 / 128 (1 / 256) -- a factor 4, exact in every product, as
    every term of the loss is linear in the row weight once the advantages are not standardised.  So the spread dev_grad must be
    ((g_0 / 4 + g_1 / 4) + g_2 / 4) + g_3 / 4 in float32, byte for byte; the same four arrays added in descending order give other
    bytes, so the equality compares something."""
    env_s, env_p = _env(case, spread=True, slabs=bs.EXACT_SLABS), _env(case)
    rec_s, rec_p = _twin_records(env_s, env_p, bs.EXACT_T, full=case in GRID)
    order = _order(rec_s, 1)
    hp = dict(ONE, adv_norm=None)
    for rows in (128, 256):
        lst = _cut(order, rows)
        out = env_s.ppo_update(rec_s, order=lst, **hp)
        assert [len(t) for t in sp.walk(rows, bs.EXACT_SLABS)] == [rows // 128] * bs.EXACT_SLABS
        shares = {k: bs.slab_rows(lst["order_" + k][0].cpu().numpy(), rows, bs.EXACT_SLABS) for k in ("inter", "intra")}
        parts = [[], []]
        for w in range(bs.EXACT_SLABS):
            one = {}
            for k in ("inter", "intra"):
                one["order_" + k] = torch.as_tensor(shares[k][w][None, :], device=env_p.device).contiguous()
                one["first_" + k] = np.array([0, len(shares[k][w])], dtype=np.int32)
            o = env_p.ppo_update(rec_p, order=one, **hp)
            for kind_i in range(2):
                parts[kind_i].append(o["grad"][0, kind_i].cpu().numpy().copy())
        for kind_i, kind in enumerate(("inter", "intra")):
            got = out["grad"][0, kind_i].cpu().numpy()
            want, other = bs.reduce_f32(parts[kind_i], bs.EXACT_SLABS), bs.reduce_f32(parts[kind_i], bs.EXACT_SLABS, "descending")
            d = np.abs(_ordered(got) - _ordered(want))
            print(f"exact reduce {case}, {rows} rows, {kind}: worst ulp distance to the ascending restatement {int(d.max())}, "
                  f"{int((d != 0).sum())} of {d.size} differ; the descending one differs in {int((want != other).sum())}")
            assert got.any() and out["rows"][0, kind_i, 0] == rows
            assert got.tobytes() == want.tobytes(), f"{case}, {rows} rows, {kind}: dev_grad is not the slabs' ascending float32 sum"
            assert want.tobytes() != other.tobytes(), "ascending and descending order give the same bytes: the equality compares nothing"
    env_s.close()
    env_p.close()


# ---- 5. one kind alone ------------------------------------------------------------------------------------------------------------------
def test_an_update_of_the_inter_kind_alone_leaves_the_intra_pair_and_equals_the_inter_kind_of_a_full_update():
    """tanh40x24, 3 slabs, two epochs of minibatches of 40: (a) an ``order`` without ``order_intra`` and (b) ``first_intra = [0, 0]`` --
    the host gives the intra kind zero steps while the launches stay sized for both -- against (c) both kinds on a twin handle.  In (a)
    and (b) the intra pair keeps its bytes and its statistics are zero; the inter pair's state, statistics and dev_grad are (c)'s byte
    for byte (the kinds are independent optimisers).  A later call with both kinds on (a) trains the intra pair from counter 0: to
    (c)'s intra bytes."""
    case = "tanh40x24"
    envs = {k: _env(case, spread=True, slabs=3) for k in "abc"}
    recs = {k: _record(e, full=False) for k, e in envs.items()}
    for k in recs["a"]:
        assert torch.equal(recs["a"][k], recs["b"][k]) and torch.equal(recs["a"][k], recs["c"][k]), k
    order = _order(recs["a"], 2)
    start = ref.state(envs["a"], 1)
    hp = dict(epochs=2, minibatch=40, grad=True, **HP_LOOP)
    inter_only = {k: v for k, v in order.items() if k.endswith("inter")}
    empty_intra = dict(inter_only, order_intra=order["order_intra"][:, :0].contiguous(), first_intra=np.array([0, 0], dtype=np.int32))
    outs = {"a": envs["a"].ppo_update(recs["a"], order=inter_only, **hp), "b": envs["b"].ppo_update(recs["b"], order=empty_intra, **hp),
            "c": envs["c"].ppo_update(recs["c"], order=order, **hp)}
    states = {k: ref.state(e, 1) for k, e in envs.items()}
    n_mb = -(-T * B // 40)
    assert int(states["c"]["inter/0/t"][0]) == 2 * n_mb and int(states["c"]["intra/0/t"][0]) > 2 * n_mb
    for k in "ab":
        for name, x in states[k].items():
            if name.split("/")[0] in ("intra", "v_intra"):
                assert x.tobytes() == start[name].tobytes(), f"({k}) an update of the inter kind alone moved {name}"
            else:
                assert x.tobytes() == states["c"][name].tobytes(), f"({k}) {name} differs from the full update's"
        assert int(states[k]["intra/0/t"][0]) == 0 and int(states[k]["inter/0/t"][0]) == 2 * n_mb
        for name in STAT_NAMES + ("grad_norm", "rows", "minibatches"):
            assert not outs[k][name][0, 1].any(), f"({k}) intra statistics {name}"
            assert outs[k][name][0, 0].tobytes() == outs["c"][name][0, 0].tobytes(), f"({k}) inter statistics {name}"
        assert torch.equal(outs[k]["grad"][0, 0], outs["c"]["grad"][0, 0]) and bool(outs[k]["grad"][0, 0].any())
        assert not bool(outs[k]["grad"][0, 1].any())
    assert states["a"]["inter/0/w0"].tobytes() != start["inter/0/w0"].tobytes()
    # a later call with both kinds on handle (a): the intra kind starts at counter 0, on the record and lists (c) saw
    later = envs["a"].ppo_update(recs["a"], order=order, **hp)
    after = ref.state(envs["a"], 1)
    for name, x in after.items():
        if name.split("/")[0] in ("intra", "v_intra"):
            assert x.tobytes() == states["c"][name].tobytes(), f"the later call: {name} differs from the full update's"
    assert int(after["intra/0/t"][0]) == int(states["c"]["intra/0/t"][0]) and int(after["inter/0/t"][0]) == 4 * n_mb
    assert torch.equal(later["grad"][0, 1], outs["c"]["grad"][0, 1])
    for e in envs.values():
        e.close()


# ---- 6. rebinding to a smaller net ------------------------------------------------------------------------------------------------------
def test_a_handle_rebound_from_shape_a_to_small_nets_equals_a_fresh_handle():
    """Shape A at 3 slabs takes one real step; then the same handle binds [24] relu nets and ``ppo_bind(spread=True, slabs=5)`` -- the
    larger slab allocation is kept, ``slab_stride`` and the block count shrink -- and takes one step on the record of a fresh handle
    that only ever saw those nets at 5 slabs: weights, moments, counters, statistics and dev_grad byte for byte"""
    small = "relu24"
    layout = ref.CASES[small][2]
    assert bs.spread_spec("A")[:3] == (ref.S, ref.US, layout)
    nets = bs.spread_nets(small)

    def bind_small(env):
        env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=ref.SEED, intra_input=layout)
        env.set_value_network(nets["v_inter"], nets["v_intra"])
        env.ppo_bind(spread=True, slabs=5)

    used = _env("A", spread=True, slabs=3)
    rec_a = _record(used)
    before = ref.state(used, 1)
    used.ppo_update(rec_a, epochs=1, minibatch=40, order=_order(rec_a, 1), **HP_LOOP)
    assert ref.state(used, 1)["inter/0/w0"].tobytes() != before["inter/0/w0"].tobytes()
    fresh = shaped_workload(ref.S, ref.US, B, seed=40 + GRID.index("A")).env
    bind_small(fresh)
    fresh.reset()
    rec = {k: v.clone() for k, v in _record(fresh).items()}
    order = _order(rec, 2)
    bind_small(used)
    ref.same_state(ref.state(used, 1), ref.state(fresh, 1), "the rebound handle before the step")
    hp = dict(epochs=2, minibatch=40, order=order, grad=True, **HP_LOOP)
    out_u, out_f = used.ppo_update(rec, **hp), fresh.ppo_update(rec, **hp)
    ref.same_state(ref.state(used, 1), ref.state(fresh, 1), "a handle rebound from shape A to [24] nets at 5 slabs")
    assert out_u.keys() == out_f.keys()
    for name in out_u:
        if name == "grad":
            assert torch.equal(out_u[name], out_f[name]) and bool(out_u[name][0, 0].any()) and bool(out_u[name][0, 1].any())
        else:
            assert np.asarray(out_u[name]).tobytes() == np.asarray(out_f[name]).tobytes(), name
    assert int(ref.state(used, 1)["inter/0/t"][0]) == 2 * -(-T * B // 40)
    used.close()
    fresh.close()
