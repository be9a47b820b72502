"""What the tests of the PPO update of MIXED populations share (tests/test_ppo_mixed_cpu.py, tests/test_gpu_ppo_mixed.py): the two
cases, the members' nets, the uniform twin populations that a member is compared with bit for bit, one synthetic record per case whose
logp column is each member's own log-probability plus a perturbation (ratios on both sides of the clip), and the packed-gradient
helpers of the planted slips.  Built on tests/ppo_update_ref.py, which stays as it is."""
from __future__ import annotations

import numpy as np
import torch

from tests import ppo_update_ref as ref

S, US, T = ref.S, ref.US, ref.T          # both cases: the native shape, as ref.native_workload builds it
FIRST = ref.FIRST                        # members of 16, 32 and 48 inter rows: a partial tile, a tile, a tile and a half
MINIBATCH = ref.MINIBATCH
SEED = 6300                              # the nets' seed: tests/test_ppo_mixed_cpu.py guards that no gradient tensor of the twin is zero with it
RECORD_SEED = 17
# case -> (intra input layout, the members' actors as (hidden widths, activation)); member m's critic is actor (m + 1) % G's shape, so
# every member's actor and critic differ in depth
#   base  every width off the 32 grid, depths 1, 2 and 4
#   edge  [512, 512, 32] at the edge of the LDS plan (162 304 of 163 840 bytes, ref.SHAPES["A"]) beside the smallest net -- which then
#         runs inside a launch with the largest LDS allocation and extent -- and one whose LDS strides are no multiples of 64
CASES = {"base": ("mask_obs", [([24], "relu"), ([40, 24], "tanh"), ([8, 8, 8, 8], "tanh")]),
         "edge": ("obs", [([512, 512, 32], "tanh"), ([24], "relu"), ([33, 160, 7, 96], "relu")])}
# A shape that fits the edge case's extent (its first two layers pack into fewer floats than [50 -> 512]) and is beyond the LDS plan:
# the extent owner's widths behind one more input-side layer, 162 304 + 128 * ld(32) = 171 008 bytes
BEYOND = ([8, 512, 512, 32], "tanh")


def shapes(case, G=None):
    """[(actor widths, actor activation, critic widths, critic activation)] per member; ``G`` members cycle through the case's"""
    actors = CASES[case][1]
    n = len(actors)
    G = n if G is None else G
    return [actors[m % n] + actors[(m + 1) % n] for m in range(G)]


def layout(case):
    return CASES[case][0]


def member_seed(m):
    return SEED + 10 * m


def mixed_nets(case, G=None):
    """{role: [member's net]} of the mixed population"""
    per = [ref.make_role_nets(S, US, aw, aa, layout(case), member_seed(m), cw, ca) for m, (aw, aa, cw, ca) in enumerate(shapes(case, G))]
    return {r: [p[r] for p in per] for r in ref.ROLES}


def twin_nets(case, m, G=None):
    """{role: [net]} of the UNIFORM twin population of member ``m``: every member has m's shape and activations, position m holds m's own
    weights (the same seed), the others weights of their own"""
    sh = shapes(case, G)
    aw, aa, cw, ca = sh[m]
    per = [ref.make_role_nets(S, US, aw, aa, layout(case), member_seed(i) + (0 if i == m else 5), cw, ca) for i in range(len(sh))]
    return {r: [p[r] for p in per] for r in ref.ROLES}


_RECORDS = {}


def record(case, first=FIRST, G=None):
    """The case's synthetic record (host tensors, computed once and left unchanged): ref.synthetic_record with, for every member's rows,
    logp = the member's own nets' log-probability + 0.25 N(0, 1), rounded to float32"""
    from intent_radio_sched_multi_slice_amd import adapters as ad
    key = (case, tuple(first))
    if key in _RECORDS:
        return _RECORDS[key]
    B = first[-1]
    rec = ref.synthetic_record(B=B, seed=RECORD_SEED, layout=layout(case))
    nets, sh = mixed_nets(case, G), shapes(case, G)
    g = torch.Generator().manual_seed(5)
    view = rec["logp"].reshape(-1, S + 1)
    for kind in ("inter", "intra"):
        rows = torch.arange(rec["mask_inter"].numel() // (S if kind == "inter" else 1))
        envs = (rows // (1 if kind == "inter" else S)) % B
        for m in range(len(sh)):
            mine = rows[(envs >= first[m]) & (envs < first[m + 1])]
            batch = ad.ppo_rows(rec, kind, mine, layout(case))
            with torch.no_grad():
                _, st = ad.ppo_loss_reference([(w.double(), b.double()) for w, b in ref.layers_of(nets[kind][m])], None, batch, kind, 0.2, 0.5, 0.01, False, sh[m][1])
            lp = (st["logp"] + 0.25 * torch.randn(st["logp"].shape, generator=g, dtype=torch.float64)).to(torch.float32)
            if kind == "inter":
                view[mine, 0] = lp
            else:
                view[mine // S, 1 + mine % S] = lp
    _RECORDS[key] = rec
    return rec


def order(case, epochs, first=FIRST, G=None, seed=4):
    from intent_radio_sched_multi_slice_amd import adapters as ad
    return ad.ppo_row_order(record(case, first, G), first, epochs, seed=seed)


def twin_gradient(case, kind, m, dtype=torch.float64, nets=None, acts=None, first=FIRST):
    """``adapters.ppo_update_reference`` of member m and kind at the bound weights: one minibatch of all its rows, lr 0, no clipping.
    ``nets`` / ``acts``: another (actor layers, critic layers) / (actor activation, critic activation) than the member's -- a planted slip"""
    from intent_radio_sched_multi_slice_amd import adapters as ad
    a, c = ("inter", "v_inter") if kind == "inter" else ("intra", "v_intra")
    if nets is None:
        all_nets = mixed_nets(case)
        nets = (ref.layers_of(all_nets[a][m]), ref.layers_of(all_nets[c][m]))
    aw, aa, cw, ca = shapes(case)[m]
    aa, ca = (aa, ca) if acts is None else acts
    o = order(case, 1, first)
    f = o["first_" + kind]
    return ad.ppo_update_reference(record(case, first), kind, nets[0], nets[1], o["order_" + kind], int(f[m]), int(f[m + 1]), epochs=1, minibatch=ref.ALL,
                                   lr=0.0, grad_clip=0.0, act_actor=aa, act_critic=ca, layout=layout(case), dtype=dtype, clip=0.2, vf_coeff=0.5,
                                   ent_coeff=0.01, adv_norm=True)


def pack_grad(actor, critic):
    """The inverse of ref.unpack_grad: lists of (dW, db) -> the packed float64 block, actor then critic, widths padded to 32"""
    flat = []
    for w, b in list(actor) + list(critic):
        w, b = np.asarray(w, dtype=np.float64), np.asarray(b, dtype=np.float64)
        W = np.zeros((ref.pad32(w.shape[0]), ref.pad32(w.shape[1])))
        W[:w.shape[0], :w.shape[1]] = w
        bb = np.zeros(ref.pad32(w.shape[0]))
        bb[:b.shape[0]] = b
        flat += [W.reshape(-1), bb]
    return np.concatenate(flat)


def packed_floats(net):
    """Floats of the packed copy of a list of (W, b)"""
    return sum(ref.pad32(w.shape[0]) * ref.pad32(w.shape[1]) + ref.pad32(w.shape[0]) for w, b in net)


def unpack_at(flat, net, at):
    """The (dW, db) of ``net`` read from float ``at`` of a packed block, zeros beyond its end, no padding check: what a reader that
    starts at a wrong offset sees"""
    out = []
    flat = np.concatenate([flat, np.zeros(packed_floats(net) + at)])
    for w, b in net:
        N, K = w.shape
        np_, kp = ref.pad32(N), ref.pad32(K)
        W = flat[at:at + np_ * kp].reshape(np_, kp)
        at += np_ * kp
        out.append((W[:N, :K].copy(), flat[at:at + N].copy()))
        at += np_
    return out


def ratios(t64, t32, other):
    """{(net, layer, "W" / "b"): error of ``other`` against the float64 twin over the float32 yardstick's (floor 1e-6)}: what
    ref.check_against_twin bounds by 8 on the GPU.  All three: {"actor": [(dW, db)], "critic": [...]} of tensors or arrays"""
    out = {}
    for net in ("actor", "critic"):
        for li, (g64, g32, go) in enumerate(zip(t64[net], t32[net], other[net])):
            for name, x64, x32, xo in zip("Wb", g64, g32, go):
                x64, x32, xo = (np.asarray(x, dtype=np.float64) for x in (x64, x32, xo))
                n = np.linalg.norm(x64)
                out[net, li, name] = np.linalg.norm(xo - x64) / n / max(np.linalg.norm(x32 - x64) / n, 1e-6)
    return out
