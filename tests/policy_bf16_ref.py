"""A float64 statement of a RANENV_NET_BF16 policy net (include/ranenv.h: the numeric contract) with a rigorous error bound, and
integer-valued nets whose every evaluation is exact: the shared reference of tests/test_policy_bf16_cpu.py and
tests/test_gpu_policy_bf16.py.  ``adapters._mlp_forward(..., precision="bf16")`` is the normative float32 restatement; this module
is its high-precision twin, as tests/policy_ref.py is for the float32 nets.

The contract's rounding points -- W at bind, the input row, every hidden layer's activation -- are roundings to bf16, round to
nearest even.  ``mlp64_bf16`` applies them to its float64 values and carries policy_ref.mlp64's bound ``t`` through the layers:

    Linear     t = |W| t_in + 2 (K + 2) u a     mlp64's rule with the accumulation term doubled: products of two bf16 numbers are
                                                exact in float32, the matrix core's internal rounding is not documented, so two
                                                units per operation instead of one
    tanh/relu  mlp64's rules
    rounding   treated exactly.  The device rounds some float32 v with |v - h| <= t, the reference rounds h.  Rounding is monotone:
               the device's result lies between the roundings of the ends of [h - t, h + t] (widened by one float32 ulp, for the
               cast of the ends).  If both ends round to the reference's value the next layer's input bound is 0 -- device and
               reference hold the same number -- else it is the distance from the reference's value to the farther rounded end.

So most hidden values carry no error at all, a few carry one bf16 ulp (a flip at a rounding boundary), and the output bound says
how far such flips can move an output.  The bound does not depend on rounding luck.
"""
from __future__ import annotations

import numpy as np

from tests import policy_ref as pr

U32 = pr.U32


def bf16(x):
    """float32 -> bfloat16, round to nearest even, as float32 again: on the bits (add 0x7FFF + bit 16, drop the low half)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(x), x, r).astype(np.float32)


def bf16_trunc(x):
    """The planted slip: truncation instead of rounding."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def round_bound(h, t):
    """(r, bound): the reference's rounded value of float64 ``h`` and the bound on |device's rounded value - r| when the device
    rounds a float32 within ``t`` of ``h``."""
    h32 = h.astype(np.float32)
    lo = bf16(np.nextafter((h - t).astype(np.float32), np.float32(-np.inf))).astype(np.float64)
    hi = bf16(np.nextafter((h + t).astype(np.float32), np.float32(np.inf))).astype(np.float64)
    r = bf16(h32).astype(np.float64)
    exact = (t == 0.0) & (h32.astype(np.float64) == h)          # the device holds h itself: the same rounding
    return r, np.where(exact, 0.0, np.maximum(hi - r, r - lo))


def linear64(h, t, w, b):
    """One Linear in float64 on inputs h with bound t: (z, its bound) -- policy_ref.mlp64's rule, the accumulation term doubled."""
    w, b = pr._np(w), pr._np(b)
    aw = np.abs(w)
    z = h @ w.T + b
    a = (np.abs(h) + t) @ aw.T + np.abs(b)
    K = pr.pad32(w.shape[1])
    return z, t @ aw.T + 2 * (K + 2) * U32 * a + 2.0 ** -50 * a + K * 2.0 ** -125


def activation64(z, t, act):
    """policy_ref.mlp64's activation rules: (act(z), its bound)."""
    if act == "tanh":
        t = t / np.cosh(np.maximum(np.abs(z) - t, 0.0)) ** 2
        z = np.tanh(z)
        return z, t + pr.TANH_ULPS * 2.0 ** -23 * np.abs(z) + 2.0 ** -126
    if act == "relu":
        return np.maximum(z, 0.0), np.where(z < -t, 0.0, t)
    raise ValueError(act)


def mlp64_bf16(x, layers, act, t0=None):
    """The float64 forward of a bf16 net on float32 inputs ``x`` [R, K] with the contract's rounding points: (y [R, N], t [R, N]),
    the outputs and the bound on their distance to any evaluation the contract allows.  A ``PerSlice`` stack (a list subclass
    with attribute ``per_slice``) runs slice s's rows (row b * S + s) through net s."""
    if getattr(layers, "per_slice", False):
        S = len(layers)
        xs = pr._np(x).reshape(-1, S, np.shape(x)[-1])
        outs = [mlp64_bf16(xs[:, s], layers[s], act) for s in range(S)]
        y, t = np.stack([o[0] for o in outs], axis=1), np.stack([o[1] for o in outs], axis=1)
        return y.reshape(xs.shape[0] * S, -1), t.reshape(xs.shape[0] * S, -1)
    h = pr._np(x)
    h, t = round_bound(h, np.zeros_like(h) if t0 is None else pr._np(t0))
    for i, (w, b) in enumerate(layers):
        z, t = linear64(h, t, bf16(pr._np(w, np.float32)), pr._np(b, np.float32))
        if i == len(layers) - 1:
            return z, t
        z, t = activation64(z, t, act)
        h, t = round_bound(z, t)


class PerSlice(list):
    """The (W, b) stacks of S nets of one shape, entry s for slice index s (``mlp64_bf16`` runs them per slice)."""
    per_slice = True


# ---- a float32 restatement in numpy with planted slips (tests/test_policy_bf16_cpu.py) -------------------------------------------
SLIPS = ("truncate", "unrounded_weights", "unrounded_hidden", "rounded_output", "swapped_k", "rounded_bias")


def forward32(x, layers, act, slip=None):
    """The contract in float32 numpy; ``slip``: one of SLIPS, a planted mistake."""
    rnd = bf16_trunc if slip == "truncate" else bf16
    h = rnd(np.asarray(x, dtype=np.float32))
    for i, (w, b) in enumerate(layers):
        w, b = pr._np(w, np.float32), pr._np(b, np.float32)
        wq = w if slip == "unrounded_weights" else rnd(w)
        if slip == "swapped_k":                                # k and k + 1 of every 8-group swapped on the weights' side only
            K8 = wq.shape[1] // 8 * 8
            idx = np.arange(wq.shape[1])
            idx[:K8] = idx[:K8] ^ 1
            wq = wq[:, idx]
        if slip == "rounded_bias":
            b = rnd(b)
        z = (h.astype(np.float32) @ wq.T.astype(np.float32) + b).astype(np.float32)
        if i == len(layers) - 1:
            return rnd(z) if slip == "rounded_output" else z
        z = np.tanh(z).astype(np.float32) if act == "tanh" else np.maximum(z, np.float32(0))
        h = z if slip == "unrounded_hidden" else rnd(z)


# ---- integer-valued nets: every evaluation order gives the same bits ----------------------------------------------------------
OUT_SCALE = 2.0 ** -9


def exact_net(dims, seed, first_nnz=6, nnz=3):
    """A relu net as a list of float32 (W, b) on inputs in {0, 1}: hidden weights with ``first_nnz`` (first layer) / ``nnz``
    nonzeros per row out of {-1, +1} -- more where a layer has so few rows that its columns would not all be read: the columns
    are first dealt to the rows in turn, so every input column of every layer meets a nonzero weight --; integer biases in
    {0, 1, 2}; output weights scaled by 2^-9 and zero output bias.  Every hidden value is a small integer -- exact in bf16 --,
    every partial sum is exact in float32: any summation order reproduces the float64 value bit for bit, and a wrong k
    permutation, row map, padding or tail cannot."""
    rng = np.random.default_rng(seed)
    layers = []
    for i in range(len(dims) - 1):
        K, N = dims[i], dims[i + 1]
        last = i == len(dims) - 2
        n = min(max(first_nnz if i == 0 else nnz, -(-K // N)), K)
        w = np.zeros((N, K), dtype=np.float32)
        dealt = rng.permutation(K)
        for r in range(N):
            cols = dealt[r::N]                                  # this row's share of the columns, then random ones up to n
            rest = np.setdiff1d(np.arange(K), cols)
            cols = np.concatenate([cols, rng.choice(rest, n - len(cols), replace=False)]) if len(cols) < n else cols
            w[r, cols] = rng.choice([-1.0, 1.0], len(cols))
        if last:
            w *= np.float32(OUT_SCALE)
        b = np.zeros(N, dtype=np.float32) if last else rng.integers(0, 3, N).astype(np.float32)
        layers.append((w, b))
    return layers


def exact_forward(x, layers, hidden=None):
    """float64 relu forward of an exact net; ``hidden``: a list that receives every hidden layer's values."""
    h = pr._np(x)
    for i, (w, b) in enumerate(layers):
        h = h @ pr._np(w).T + pr._np(b)
        if i < len(layers) - 1:
            h = np.maximum(h, 0.0)
            if hidden is not None:
                hidden.append(h)
    return h


def exact_forward_ref(x, layers, act="relu", t0=None):
    """``exact_forward`` as a PolicyRef / HeadRef ``forward``: outputs with bound 0 (also for a PerSlice stack)."""
    assert act == "relu"
    if getattr(layers, "per_slice", False):
        S = len(layers)
        xs = pr._np(x).reshape(-1, S, np.shape(x)[-1])
        y = np.stack([exact_forward(xs[:, s], layers[s]) for s in range(S)], axis=1).reshape(xs.shape[0] * S, -1)
    else:
        y = exact_forward(x, layers)
    return y, np.zeros_like(y)


def exact_inputs(rng, B, S, Us):
    """obs_inter [B, 10S] and obs_intra [B, S, 2Us+9] of zeros and ones (float32)."""
    return rng.integers(0, 2, (B, 10 * S)).astype(np.float32), rng.integers(0, 2, (B, S, 2 * Us + 9)).astype(np.float32)


# ---- the cases both test modules share --------------------------------------------------------------------------------------------
ARCHS = {"33": [33], "64x64": [64, 64], "400x300": [400, 300], "40x72x40x72": [40, 72, 40, 72], "512x3": [512, 512, 512]}
B_TEST = 70                      # two full tiles of 32 rows and a tail of 6
SHAPES = {"S5": (5, 5), "S10": (10, 10)}     # (S, Us): inter input 50 -> 64, intra 19 -> 32 / mask_obs 24 -> 32; 100 -> 128, 29 -> 32


def intra_width(Us, layout):
    return 2 * Us + 9 + (Us if layout == "mask_obs" else 0)


def exact_case_nets(arch, S, Us, layout, seed, per_slice=False, head_out=None):
    """(inter actor [10S -> 2S], intra actor [-> 3] or a list of S of them, inter critic [-> 1], intra critic [-> 1]) of exact nets;
    ``head_out``: the inter actor's output width instead of 2S (a head actor)."""
    w, n_in = ARCHS[arch], intra_width(Us, layout)
    intra = ([exact_net([n_in] + w + [3], seed + 10 + s) for s in range(S)] if per_slice else exact_net([n_in] + w + [3], seed + 1))
    return (exact_net([10 * S] + w + [2 * S if head_out is None else head_out], seed), intra,
            exact_net([10 * S] + w + [1], seed + 2), exact_net([n_in] + w + [1], seed + 3))


# (name, S/Us key, hidden widths, activation, stochastic, gain of the intra net's initialisation).  The gain is what makes at least
# half of the rows' intra choices decidable under the logits' bound (asserted by tests/test_policy_bf16_cpu.py).  Scaling the logits
# does not: bound and margin scale together.  What does is the hidden rows' L1 norm: one flipped rounding upstream moves a
# pre-activation by up to |w| ulp, the worst case adds these up over the row, and at width 512 under uniform(+-1 / sqrt(fan_in)) that
# sum (about 11 per layer) outgrows the logits' spread within three layers (13 % of the rows decidable with tanh, 36 % with relu);
# at gain 0.3 it is about 3.4 and 99.9 % are.  The inter nets keep gain 1: their scores are compared within the bound either way.
RANDOM_CASES = [("64x64-tanh", "S5", [64, 64], "tanh", False, 1.0), ("64x64-relu", "S10", [64, 64], "relu", True, 1.0),
                ("512x3-tanh", "S10", [512, 512, 512], "tanh", True, 0.3), ("512x3-relu", "S5", [512, 512, 512], "relu", False, 0.3)]
RANDOM_IDS = [c[0] for c in RANDOM_CASES]
RANDOM_SEED = 0xB16


def random_case_nets(case):
    """(inter actor, intra actor) of a random case as torch modules (tests/gpu_common.make_net's initialisation)."""
    from tests.gpu_common import make_inter_net, make_net
    name, key, widths, act, st, gain = case
    S, Us = SHAPES[key]
    k = RANDOM_IDS.index(name)
    return make_inter_net(S, widths, act, 700 + k), make_net([intra_width(Us, "obs")] + list(widths) + [3], act, 800 + k, gain=gain)


def random_case_inputs(case, step=0):
    """The injected observations of a random case's TTI ``step``: policy_ref.injected_inputs under the case's own generator."""
    name, key = case[0], case[1]
    S, Us = SHAPES[key]
    rng = np.random.default_rng([RANDOM_SEED, RANDOM_IDS.index(name), step])
    return pr.injected_inputs(rng, B_TEST, S, Us)


# (architecture, S/Us key, intra input layout) of the exact GPU tests; case k's nets are exact_case_nets(..., seed=900 + 10 k)
EXACT_CASES = [("33", "S5", "obs"), ("64x64", "S5", "mask_obs"), ("400x300", "S10", "obs"), ("40x72x40x72", "S5", "mask_obs"),
               ("512x3", "S10", "obs")]
EXACT_IDS = [c[0] for c in EXACT_CASES]


def exact_case_seed(case):
    return 900 + 10 * EXACT_IDS.index(case[0])


def exact_case_inputs(case, step=0):
    """(obs_inter, obs_intra, mask_intra) of zeros and ones for an exact case's TTI ``step`` (the mask: what a CPU test feeds the
    mask_obs layout; on the device the env's own 0 / 1 mask stands there)."""
    S, Us = SHAPES[case[1]]
    rng = np.random.default_rng([RANDOM_SEED + 1, EXACT_IDS.index(case[0]), step])
    oi, oa = exact_inputs(rng, B_TEST, S, Us)
    return oi, oa, rng.integers(0, 2, (B_TEST, S, Us)).astype(np.int8)
