"""The shape grid of the three newest PPO bindings -- per slice (ranenv_ppo_bind_slices), spread (ranenv_ppo_bind_spread) and head-spread
(ranenv_ppo_bind_head_spread) --, stated once: tests/test_ppo_bindings_shapes_cpu.py guards its inputs, and
tests/test_gpu_ppo_per_slice_shapes.py, tests/test_gpu_ppo_spread_shapes.py and tests/test_gpu_ppo_head_spread_shapes.py run on it.
Built on tests/ppo_update_ref.py (``ref``), tests/ppo_wide_ref.py (``wd``), tests/ppo_spread_ref.py (``sp``), tests/ppo_head_ref.py
(``hd``) and tests/ppo_head_shapes_ref.py (``hg``); ``ref`` gained ``pair_lds_bytes``, the per-kind LDS formula its ``lds_bytes`` is built on.  The list and state helpers of
tests/test_gpu_ppo_per_slice.py that the new per-slice module needs again live here, and that module imports them.

PER SLICE.  Every case: B 12, T 8, minibatch 12, S DISTINCT actor / critic pairs.  The explicit row lists give one slice SMALL = 20 rows
(a partial tile; 12 + 8), the slice with the most live rows BIG = 40 (a tile and a quarter; 12 + 12 + 12 + 4) and every other slice all
its live rows.  S 1 has one slice, which cannot hold both shares: the twin test gives it SMALL, the bit-for-bit test BIG.
    plain plan (ref.SHAPES):   D  S 1          C  S 16, Us 16, mask_obs, critic deeper          F  S 10, a 7-wide bottleneck
                               B  S 13, mask_obs, relu, critic shallower
    beyond the plan (wd.BEYOND at S 2, Us 5):   verybig [512] x 3 tanh          past_limit [512, 512, 96] relu, mask_obs
tests/test_gpu_ppo_per_slice_spread_shapes.py runs the same cases, and ``intra_heavy`` (S 3; below), under the per-slice SPREAD binding
(ranenv_ppo_bind_slices_spread) at the figures of tests/ppo_per_slice_spread_ref.py; ``slice_block_claims`` states what that grid covers.

SPREAD.  One agent of ref.SHAPES A..F at B 12, T 8, plus ``lopsided``: shape A's inter pair beside relu24's intra pair on the native
shape.  ref.make_role_nets gives the two kinds of an agent the same hidden widths, so no shape of A..F has kinds whose packed floats differ
by 10x; ``lopsided`` has (613 blocks against 5).  A layer's padded copy is at least 32 x 32 + 32 = 1056 floats, more than
PPO_SPREAD_BLOCK: no kind has ONE reduce / apply block.  An actor / critic pair with one hidden layer each (four layers of 1056 floats)
has 5, the fewest of any pair; ``lopsided``'s intra kind is one.  (A kind without a bound critic could have 3; the grid binds critics.)  ``block_claims`` states what the grid covers; the CPU test and the GPU module assert it.

THE EXACT REDUCE.  ``slab_rows`` / ``reduce_f32`` restate the header's "workgroup w walks tiles w, w + grid, ..." and "summed in ascending
slab order" on numpy arrays; ``slip`` plants a walk of tiles w, w + 1 or a descending sum."""
from __future__ import annotations

import numpy as np
import torch

from tests import ppo_head_ref as hd
from tests import ppo_head_shapes_ref as hg
from tests import ppo_spread_ref as sp
from tests import ppo_update_ref as ref
from tests import ppo_wide_ref as wd

STAT_NAMES = ("policy_loss", "value_loss", "entropy", "kl", "clip_frac", "grad_norm", "rows", "minibatches")
SPREAD_BLOCK = 1024                      # PPO_SPREAD_BLOCK of csrc/ranenv_internal.h
MIN_PAIR_BLOCKS = 5                      # an actor / critic pair with one hidden layer each, every width <= 32: four layers of 32 x 32 + 32 floats

# ---- per slice ----------------------------------------------------------------------------------------------------------------------
SLICE_B, SLICE_T, SLICE_MB, SMALL, BIG = 12, 8, 12, 20, 40
SLICE_SHAPES = ("D", "C", "F", "B")
SLICE_BEYOND = ("verybig", "past_limit")
BEYOND_S, BEYOND_US = 2, 5
SLICE_SEED = 6300                        # the nets' seed: tests/test_ppo_bindings_shapes_cpu.py guards the twin's gradients with it
# PER SLICE OVER THE CHIP (ranenv_ppo_bind_slices_spread; tests/test_gpu_ppo_per_slice_spread_shapes.py) runs the six cases above at the
# figures of tests/ppo_per_slice_spread_ref.py (T 24, minibatch 72, shares of 20 and 100 rows) and one case more.  ref.make_role_nets gives
# the two kinds the same hidden widths and 10 S >= the intra input, so in all six the inter pair has at least the intra pair's reduce /
# apply blocks; ``intra_heavy`` is the other way round: a [24] inter pair (5 blocks, the fewest a pair can have) beside S 3 intra pairs of
# [160, 96] / [255] (40 blocks).  ``slice_block_claims`` states what that grid covers.
SLICE_LOPSIDED = "intra_heavy"
LOPSIDED_S, LOPSIDED_US, LOPSIDED_LAYOUT, LOPSIDED_ACT = 3, 4, "obs", "tanh"
LOPSIDED_WIDTHS = {"inter": ([24], [24]), "intra": ([160, 96], [255])}      # kind -> (actor hidden widths, critic hidden widths)
SLICE_SPREAD_SHAPES = SLICE_SHAPES + (SLICE_LOPSIDED,)


def slice_spec(case):
    """(S, Us, layout, (actor widths, activation), (critic widths, activation)) of a per-slice case"""
    if case in ref.SHAPES:
        return ref.SHAPES[case]
    if case == SLICE_LOPSIDED:               # (the widths are the intra pairs'; the inter pair's are LOPSIDED_WIDTHS["inter"])
        aw, cw = LOPSIDED_WIDTHS["intra"]
        return LOPSIDED_S, LOPSIDED_US, LOPSIDED_LAYOUT, (aw, LOPSIDED_ACT), (cw, LOPSIDED_ACT)
    widths, act, layout = wd.BEYOND[case]
    return BEYOND_S, BEYOND_US, layout, (widths, act), (widths, act)


def slice_nets(case, seed=SLICE_SEED):
    """The inter pair and S distinct intra pairs of the case: {"inter", "v_inter": net, "intra", "v_intra": [S nets]}"""
    S, Us, layout, (aw, aa), (cw, ca) = slice_spec(case)
    per = [ref.make_role_nets(S, Us, aw, aa, layout, seed + 10 * s, cw, ca) for s in range(S)]
    if case == SLICE_LOPSIDED:
        small = ref.make_role_nets(S, Us, LOPSIDED_WIDTHS["inter"][0], aa, layout, seed + 7, LOPSIDED_WIDTHS["inter"][1], ca)
        per[0] = dict(per[0], inter=small["inter"], v_inter=small["v_inter"])
    return {"inter": per[0]["inter"], "v_inter": per[0]["v_inter"], "intra": [p["intra"] for p in per], "v_intra": [p["v_intra"] for p in per]}


def kind_dims(S, Us, layout, aw, cw):
    """{kind: (actor widths [in, hidden..., out], critic widths)}"""
    n_in = ref.intra_width(Us, layout)
    return {"inter": ([10 * S] + list(aw) + [2 * S], [10 * S] + list(cw) + [1]), "intra": ([n_in] + list(aw) + [3], [n_in] + list(cw) + [1])}


def slice_dims(case):
    S, Us, layout, (aw, _), (cw, _) = slice_spec(case)
    if case == SLICE_LOPSIDED:
        return {"inter": kind_dims(S, Us, layout, *LOPSIDED_WIDTHS["inter"])["inter"], "intra": kind_dims(S, Us, layout, aw, cw)["intra"]}
    return kind_dims(S, Us, layout, aw, cw)


def slice_kind_floats(case):
    """{kind: (the actor's packed floats ``af``, the pair's)} of a per-slice case; one intra pair's, not S times it"""
    return {k: (sp.packed_floats(a), sp.packed_floats(a) + sp.packed_floats(c)) for k, (a, c) in slice_dims(case).items()}


def slice_block_claims(cases=None):
    """What the per-slice spread grid covers, from the packed float counts alone: {claim: the cases that hold it}.  The reduce / apply
    grid of a step is the larger kind's blocks for every unit: the units of the smaller kind return beyond their own."""
    cases = SLICE_SPREAD_SHAPES + SLICE_BEYOND if cases is None else cases
    out = {"inter pair has more blocks": [], "intra pair has more blocks": [], "af off the block grid, inter": [], "af off the block grid, intra": []}
    for case in cases:
        kf = slice_kind_floats(case)
        b = {k: blocks_of(f) for k, (_, f) in kf.items()}
        if b["inter"] > b["intra"]:
            out["inter pair has more blocks"].append(case)
        if b["intra"] > b["inter"]:
            out["intra pair has more blocks"].append(case)
        for k in kf:
            if kf[k][0] % SPREAD_BLOCK != 0:
                out[f"af off the block grid, {k}"].append(case)
    return out


def slice_order(rec, epochs, minibatch, small, big_rows, empty=None, seed=3, only=None):
    """Explicit row lists of a per-slice call: the slice with the most live rows keeps ``big_rows``, its right neighbour ``small``, every
    other slice all its live rows (at least a tile), ``empty`` none; S 1: the one slice keeps ``only`` rows.  One random stream per
    draw: an emptied share moves no other draw.  Returns (order, the slices' shares [S]).  Asserts the counts."""
    mask = rec["mask_inter"].cpu().numpy() != 0
    T, B, S = mask.shape
    live = [np.nonzero(mask[:, :, s].reshape(-1))[0] * S + s for s in range(S)]          # rows (t * B + b) * S + s, ascending
    rng = lambda *key: np.random.default_rng([seed, *key])  # noqa: E731
    if S == 1:
        assert only in (small, big_rows) and len(live[0]) >= only
        keep = {0: rng(100, 0).permutation(live[0])[:only]}
        big = small_s = None
    else:
        big = int(np.argmax([len(x) for x in live]))
        small_s = (big + 1) % S
        assert len(live[big]) >= big_rows and len(live[small_s]) >= small, [len(x) for x in live]
        assert all(len(live[s]) >= 32 for s in range(S) if s not in (big, small_s)), [len(x) for x in live]
        keep = {s: live[s] for s in range(S)}
        keep[big], keep[small_s] = rng(100, big).permutation(live[big])[:big_rows], rng(100, small_s).permutation(live[small_s])[:small]
    if empty is not None:
        keep[empty] = keep[empty][:0]
    counts = [len(keep[s]) for s in range(S)]
    if S > 1:
        assert empty == small_s or (counts[small_s] == small and small < 32 and small % minibatch != 0), "a share below one tile with a short last minibatch"
        assert empty == big or (counts[big] == big_rows and big_rows > 32 and big_rows % minibatch != 0), "a share beyond one tile with a short last minibatch"
    else:
        assert counts[0] % minibatch != 0 and counts[0] != 32
    assert empty is None or counts[empty] == 0
    intra = np.stack([np.concatenate([rng(ep, s).permutation(keep[s]) for s in range(S)]) for ep in range(epochs)]).astype(np.int32)
    inter = np.stack([rng(ep, S).permutation(T * B) for ep in range(epochs)]).astype(np.int32)
    dev = rec["logp"].device
    order = {"order_inter": torch.as_tensor(inter, device=dev).contiguous(), "first_inter": np.array([0, T * B], dtype=np.int32),
             "order_intra": torch.as_tensor(intra.reshape(epochs, -1), device=dev).contiguous(),
             "first_intra": np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)}
    return order, counts


def share(order, s):
    """The lists of a plain one-member call that trains the inter pair and slice s's share alone"""
    lo, hi = int(order["first_intra"][s]), int(order["first_intra"][s + 1])
    return dict(order, order_intra=order["order_intra"][:, lo:hi].contiguous(), first_intra=np.array([0, hi - lo], dtype=np.int32))


def host(layers):
    return [(w.cpu().numpy().copy(), b.cpu().numpy().copy()) for w, b in layers]


def slice_state(env, s):
    """Slice s's trainable state (s None: the inter pair's) as host bytes: weights, moments, counter"""
    out = {}
    for r in (("inter", "v_inter") if s is None else ("intra", "v_intra")):
        for i, (w, b) in enumerate(host(env.net_weights(r) if s is None else env.net_weights(r, slice=s))):
            out[f"{r}/w{i}"], out[f"{r}/b{i}"] = w, b
        for k, v in env.ppo_state(r, slice=0 if s is None else s).items():
            out[f"{r}/{k}"] = v.cpu().numpy().copy()
    return out


def plain_state(env, kind):
    """The same of a one-member handle's kind (0 inter, 1 intra)"""
    out = {}
    for r in (("inter", "v_inter") if kind == 0 else ("intra", "v_intra")):
        for i, (w, b) in enumerate(host(env.net_weights(r))):
            out[f"{r}/w{i}"], out[f"{r}/b{i}"] = w, b
        for k, v in env.ppo_state(r).items():
            out[f"{r}/{k}"] = v.cpu().numpy().copy()
    return out


def wg_row(out, wg):
    """Workgroup wg's statistics [epochs, 8] and gradient bytes of a per-slice call"""
    return np.stack([out[n][wg] for n in STAT_NAMES], axis=-1), out["grad"][wg].cpu().numpy()


class SliceView:
    """Slice s of a per-slice handle as the one member of the comparisons in tests/ppo_update_ref.py"""
    def __init__(self, env, s):
        self.env, self.s = env, s

    def ppo_state(self, role, m=0):
        return self.env.ppo_state(role, slice=self.s)

    def weights(self):
        return {"inter": {0: host(self.env.net_weights("inter"))}, "v_inter": {0: host(self.env.net_weights("v_inter"))},
                "intra": {0: host(self.env.net_weights("intra", slice=self.s))}, "v_intra": {0: host(self.env.net_weights("v_intra", slice=self.s))}}

    def out(self, out):
        """A per-slice call's result in ``ppo_update``'s shape for one member: kind 0 the inter pair, kind 1 this slice"""
        o = {n: np.stack([out[n][0], out[n][1 + self.s]])[None] for n in STAT_NAMES}
        o["grad"] = torch.stack([out["grad"][0], out["grad"][1 + self.s]])[None]
        return o


# ---- spread -------------------------------------------------------------------------------------------------------------------------
SPREAD_B, SPREAD_T = 12, 8
SPREAD_SHAPES = tuple(ref.SHAPES)        # A .. F
LOPSIDED = "lopsided"                    # shape A's inter pair beside relu24's intra pair, on the native shape (S 5, Us 5, "obs")
SPREAD_BEYOND = ("past_limit", "deepest")
EXACT_CASES = ("tanh40x24", "E")
EXACT_T = 24                             # B 12 x T 24 = 288 inter rows: lists of 128 and of 256 rows per kind
EXACT_SLABS = 4
# relu24 on the native workload: 16 896 inter rows -- one minibatch of 528 tiles, or two of 8448 rows (264 tiles each) -- under 256 slabs
ALL_SLABS_B, ALL_SLABS_T, ALL_SLABS_MB = 96, 176, 8448


def spread_spec(case):
    """(S, Us, layout, activation of the actors, of the critics, {kind: (actor widths, critic widths)}) of a one-agent case"""
    if case in ref.SHAPES:
        S, Us, layout, (aw, aa), (cw, ca) = ref.SHAPES[case]
        return S, Us, layout, aa, ca, kind_dims(S, Us, layout, aw, cw)
    if case == LOPSIDED:
        _, _, layout, (aw, aa), (cw, ca) = ref.SHAPES["A"]
        small = ref.CASES["relu24"][0]
        assert layout == ref.CASES["relu24"][2]
        # (one activation per role pair: the inter pair keeps A's tanh, and the twin is told the same for the intra pair)
        return ref.S, ref.US, layout, aa, ca, {"inter": kind_dims(ref.S, ref.US, layout, aw, cw)["inter"], "intra": kind_dims(ref.S, ref.US, layout, small, small)["intra"]}
    widths, act, layout = ref.CASES[case] if case in ref.CASES else wd.BEYOND[case]
    return ref.S, ref.US, layout, act, act, kind_dims(ref.S, ref.US, layout, widths, widths)


def spread_nets(case):
    """{role: net} of ONE agent of the case"""
    if case in ref.SHAPES:
        nets = ref.shape_nets(case, 1)
        return {r: nets[r][0] for r in ref.ROLES}
    if case == LOPSIDED:
        big = ref.shape_nets("A", 1)
        _, _, layout, (_, aa), _ = ref.SHAPES["A"]
        small = ref.make_role_nets(ref.S, ref.US, ref.CASES["relu24"][0], aa, layout, ref.SHAPE_SEED + 7)
        return {"inter": big["inter"][0], "v_inter": big["v_inter"][0], "intra": small["intra"], "v_intra": small["v_intra"]}
    if case in ref.CASES:
        return sp.one_agent_nets(case)
    nets = wd.beyond_nets(case, n=1)
    return {r: nets[r][0] for r in ref.ROLES}


def kind_floats(case):
    """{kind: (the actor's packed floats ``af``, the pair's)}"""
    return {k: (sp.packed_floats(a), sp.packed_floats(a) + sp.packed_floats(c)) for k, (a, c) in spread_spec(case)[5].items()}


def blocks_of(floats):
    return -(-floats // SPREAD_BLOCK)


def block_claims(cases=SPREAD_SHAPES + (LOPSIDED,)):
    """What the spread grid covers, from the packed float counts alone: {claim: the cases (and kinds) that hold it}"""
    out = {"fewest blocks": [], "more than 256 blocks": [], "kinds differ by more than 10x": [], "af off the block grid": []}
    for case in cases:
        kf = kind_floats(case)
        b = {k: blocks_of(f) for k, (_, f) in kf.items()}
        for k in kf:
            if b[k] == MIN_PAIR_BLOCKS:
                out["fewest blocks"].append((case, k))
            if b[k] > 256:
                out["more than 256 blocks"].append((case, k))
            if kf[k][0] % SPREAD_BLOCK != 0:
                out["af off the block grid"].append((case, k))
        if max(b.values()) > 10 * min(b.values()):
            out["kinds differ by more than 10x"].append(case)
    return out


def slab_rows(row, rows, slabs, slip=None):
    """[slab w's entries of the list ``row`` in the order it walks them]: tiles w, w + grid, ...; ``slip`` "neighbour tiles": w, w + 1"""
    walk = sp.walk(rows, slabs)
    if slip == "neighbour tiles":
        walk = [[w, w + 1] for w in range(len(walk))]
    assert slip is not None or not sp.walk_faults(walk, rows, slabs)
    return [np.concatenate([np.asarray(row[t * sp.NET_ROWS:min((t + 1) * sp.NET_ROWS, rows)]) for t in tiles]) for tiles in walk]


def reduce_f32(parts, factor, slip=None):
    """The reduce restated: float32 arrays ``parts`` [slab] -- a slab's own gradient at a row weight ``factor`` (a power of two) times
    the spread call's --, each divided by ``factor`` (exact) and added in ascending slab order; ``slip`` "descending": the other order"""
    f = np.float32
    terms = [p.astype(f) / f(factor) for p in parts]
    if slip == "descending":
        terms = terms[::-1]
    g = terms[0].copy()
    for t in terms[1:]:
        g = (g + t).astype(f)
    return g


# ---- head-spread --------------------------------------------------------------------------------------------------------------------
HEAD_CASES = tuple(hg.CASES)


def check_head_adam_step(env, lay, out, S, what, lr, grad_clip, eps):
    """One minibatch with lr > 0 from zero moments under a head binding: weights, log_std, m and v (read back behind the call) within
    4 ulp of ref.adam_step_f32 on the call's own dev_grad at ``lay``; grad_norm within 1e-9 of the restatement's and further than
    100 x that from the norm without log_std's gradient; the counter reads 1.  Returns the two worst ulp distances."""
    from tests.gpu_common import _ordered
    g = hd.unpack_head_grad(out["grad"].cpu().numpy(), lay[0], lay[2], S, dtype=np.float32)
    none = np.zeros(0, dtype=np.float32)
    w0 = [(w.numpy(), b.numpy()) for w, b in lay[0] + lay[2]] + [(lay[1].numpy(), none)]
    want, norm, want_m, want_v = ref.adam_step_f32(w0, g["actor"] + g["critic"] + [(g["log_std"], none)], 1, lr, grad_clip, (0.9, 0.999), eps, moments=True)
    assert abs(out["grad_norm"][0] - norm) <= 1e-9 * norm and norm > grad_clip
    no_ls = float(np.sqrt(sum(float((x.astype(np.float64) ** 2).sum()) for pair in g["actor"] + g["critic"] for x in pair)))
    assert abs(out["grad_norm"][0] - no_ls) > 100 * 1e-9 * norm, "a norm without log_std's gradient"
    a1, ls1, c1 = hd.head_weights(env)
    got = [(w.numpy(), b.numpy()) for w, b in a1 + c1] + [(ls1.numpy(), none)]
    worst = 0
    for (xw, xb), (yw, yb) in zip(want, got):
        for x, y in ((xw, yw), (xb, yb)):
            if x.size:
                worst = max(worst, int(np.abs(_ordered(x) - _ordered(y)).max()))
    st = {k: env.ppo_head_state(k) for k in ("actor", "critic", "log_std")}
    assert st["log_std"]["m"].numel() == S and int(st["actor"]["t"].cpu()[0]) == 1
    worst_mv = 0
    for name, want_x in (("m", want_m), ("v", want_v)):
        nets = ref.unpack_grad(np.concatenate([st["actor"][name].cpu().numpy(), st["critic"][name].cpu().numpy()]), lay[0], lay[2], dtype=np.float32)
        got_x = nets["actor"] + nets["critic"] + [(st["log_std"][name].cpu().numpy(), none)]
        for (xw, xb), (yw, yb) in zip(want_x, got_x):
            for x, y in ((xw, yw), (xb, yb)):
                if x.size:
                    worst_mv = max(worst_mv, int(np.abs(_ordered(x) - _ordered(y)).max()))
    print(f"{what}: Adam step, worst ulp distance {worst} (weights, log_std), {worst_mv} (moments)")
    assert worst <= 4 and worst_mv <= 4
    assert not np.array_equal(ls1.numpy(), lay[1].numpy()) and st["log_std"]["m"].cpu().numpy().any()
    return worst, worst_mv


def head_spec(case):
    return hg.CASES[case] if case in hg.CASES else case


def head_bind(env, slabs):
    """The plain head binding (slabs None) or the spread one"""
    if slabs is None:
        env.ppo_bind(head=True)
    else:
        env.ppo_bind(head=True, spread=True, slabs=slabs)


def head_env(case, slabs=None, T=hd.T, **kw):
    """(env, layers, noisy record) of a case of hd.CASES or hg.CASES under the plain head binding (slabs None) or the spread one"""
    from tests.gpu_common import need_gpu
    need_gpu()
    env, lay = (hg.make_env(case, ppo=False, **kw) if case in hg.CASES else hd.make_env(case, ppo=False, **kw))
    head_bind(env, slabs)
    return env, lay, hd.with_noise(hd.collect(env, head_spec(case), T=T))


def head_twins(case, slabs_a, slabs_b, **kw):
    """Two handles of a case that hold the same record: (env a, record a, env b, record b, layers)"""
    a, lay, rec_a = head_env(case, slabs_a, **kw)
    b, _, rec_b = head_env(case, slabs_b, **kw)
    for k in rec_a:
        assert torch.equal(rec_a[k], rec_b[k]), k
    return a, rec_a, b, rec_b, lay


def to_dev(order, env):
    return order.to(env.device).contiguous()
