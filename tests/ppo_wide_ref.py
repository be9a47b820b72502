"""What the tests of the WIDE binding of the PPO update share (tests/test_ppo_wide_cpu.py, tests/test_gpu_ppo_wide.py): the wide
plan's two formulas restated from include/ranenv.h, the nets beyond the plain plan, the mixed population that holds one of them, and
one synthetic record per population whose logp column is each member's own log-probability plus a perturbation (ratios on both sides
of the clip).  Built on tests/ppo_update_ref.py and tests/ppo_mixed_ref.py, which stay as they are."""
from __future__ import annotations

import torch

from tests import ppo_update_ref as ref

S, US, T = ref.S, ref.US, ref.T          # the native shape, as ref.native_workload builds it
FIRST = ref.FIRST                        # members of 2, 4 and 6 envs: 16, 32 and 48 inter rows
MINIBATCH = ref.MINIBATCH
G = len(FIRST) - 1
WIDE_LDS_MAX = 136192                    # 4096 + 128 * 2 * ld(512)
SEED = 7400                              # the nets' seed: tests/test_ppo_wide_cpu.py guards that no gradient tensor of the twin is zero with it
RECORD_SEED = 23
# name -> (hidden widths, activation, intra input layout): the reference's `verybig`, and the shape one step past the plain plan's limit
# (170 496 bytes there, tests/test_gpu_ppo_update_shapes.py)
# (170 496 bytes there, tests/test_gpu_ppo_update_shapes.py), and `deepest`, the largest net the acting path accepts: the wide plan's LDS
# need does not grow with depth, its parked rows and its layer loop do
BEYOND = {"verybig": ([512, 512, 512], "tanh", "obs"), "past_limit": ([512, 512, 96], "relu", "mask_obs"),
          "deepest": ([512, 512, 512, 512], "tanh", "obs")}
# The shapes of ref.SHAPES that fit BOTH plans: the bit-identity test of the GPU file runs on every one of them
BOTH_PLANS_SHAPES = ("A", "B", "C", "D", "E", "F")
# The mixed population: [(hidden widths, activation)] per member, actor and critic alike; members 0 and 2 fit the plain plan
MIXED = [([64, 64], "tanh"), ([512, 512, 512], "tanh"), ([256, 256, 256], "relu")]
MIXED_LAYOUT = "obs"
# ... and re-binds of a member of it: one that fits every member's extent and parks more rows than the bind allocated (4 slabs behind
# the input's against 3), one that is larger than the extent
OUTGROWS_SCRATCH = [512, 512, 256, 256]
OUTGROWS_EXTENT = [512, 512, 512, 512]


def padded(dims):
    return [ref.pad32(int(d)) for d in dims]


def wide_lds_bytes(*nets):
    """The wide plan's LDS bytes for nets given as widths [in, hidden..., out]: 4096 + 128 * max over the nets and layers of
    (ld(layer's input width) + ld(layer's output width)), widths padded to 32"""
    return 4096 + 128 * max(ref.net_ld(a) + ref.net_ld(b) for dims in nets if dims is not None for a, b in zip(padded(dims)[:-1], padded(dims)[1:]))


def wide_scratch_floats(*nets):
    """... and the floats one workgroup parks: 32 * max over the nets of the sum over the layers of ld(layer's input width)"""
    return 32 * max(sum(ref.net_ld(a) for a in padded(dims)[:-1]) for dims in nets if dims is not None)


def kind_dims(widths, layout, S_=S, Us=US):
    """{kind: (actor widths, critic widths)} of a member whose four nets share the hidden ``widths``"""
    n_in = ref.intra_width(Us, layout)
    return {"inter": ([10 * S_] + list(widths) + [2 * S_], [10 * S_] + list(widths) + [1]), "intra": ([n_in] + list(widths) + [3], [n_in] + list(widths) + [1])}


def beyond_nets(case, n=G, seed=SEED):
    """{role: [member's net]}: n distinct net sets of the BEYOND case's shape"""
    widths, act, layout = BEYOND[case]
    per = [ref.make_role_nets(S, US, widths, act, layout, seed + 10 * m) for m in range(n)]
    return {r: [p[r] for p in per] for r in ref.ROLES}


def mixed_nets(shapes=MIXED, seed=SEED + 500):
    per = [ref.make_role_nets(S, US, w, a, MIXED_LAYOUT, seed + 10 * m) for m, (w, a) in enumerate(shapes)]
    return {r: [p[r] for p in per] for r in ref.ROLES}


def twin_nets(m, shapes=MIXED, seed=SEED + 500):
    """The UNIFORM twin population of member ``m`` of the mixed one: every member has m's shape, position m holds m's own weights"""
    w, a = shapes[m]
    per = [ref.make_role_nets(S, US, w, a, MIXED_LAYOUT, seed + 10 * i + (0 if i == m else 5)) for i in range(len(shapes))]
    return {r: [p[r] for p in per] for r in ref.ROLES}


_RECORDS = {}


def record(key, nets, acts, layout):
    """A synthetic record (host tensors, computed once per ``key`` and left unchanged): ref.synthetic_record with, for every member's
    rows, logp = the member's own actor's log-probability + 0.25 N(0, 1), rounded to float32.  ``acts``: the members' activations."""
    from intent_radio_sched_multi_slice_amd import adapters as ad
    if key in _RECORDS:
        return _RECORDS[key]
    B = FIRST[-1]
    rec = ref.synthetic_record(B=B, seed=RECORD_SEED, layout=layout)
    g = torch.Generator().manual_seed(5)
    view = rec["logp"].reshape(-1, S + 1)
    for kind in ("inter", "intra"):
        rows = torch.arange(rec["mask_inter"].numel() // (S if kind == "inter" else 1))
        envs = (rows // (1 if kind == "inter" else S)) % B
        for m in range(G):
            mine = rows[(envs >= FIRST[m]) & (envs < FIRST[m + 1])]
            batch = ad.ppo_rows(rec, kind, mine, layout)
            with torch.no_grad():
                _, st = ad.ppo_loss_reference([(w.double(), b.double()) for w, b in ref.layers_of(nets[kind][m])], None, batch, kind, 0.2, 0.5, 0.01, False, acts[m])
            lp = (st["logp"] + 0.25 * torch.randn(st["logp"].shape, generator=g, dtype=torch.float64)).to(torch.float32)
            if kind == "inter":
                view[mine, 0] = lp
            else:
                view[mine // S, 1 + mine % S] = lp
    _RECORDS[key] = rec
    return rec


def beyond_record(case):
    return record(case, beyond_nets(case), [BEYOND[case][1]] * G, BEYOND[case][2])


def mixed_record():
    return record("mixed", mixed_nets(), [a for _, a in MIXED], MIXED_LAYOUT)


def order(rec, epochs, seed=4):
    from intent_radio_sched_multi_slice_amd import adapters as ad
    return ad.ppo_row_order(rec, FIRST, epochs, seed=seed)
