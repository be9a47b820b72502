"""The row lists on the device (ranenv_ppo_row_count / ranenv_ppo_row_order, include/ranenv.h "Row lists on the device"): what
tests/test_ppo_row_order_cpu.py and tests/test_gpu_ppo_row_order.py share.

1. A plain-Python restatement of the header's text: loops over Python ints, no numpy in the arithmetic, nothing vectorised.  It is
   the yardstick of the numpy twin ``adapters.ppo_row_order_reference`` on the CPU; the twin is the yardstick of the device.
2. The cases of the GPU test -- sizes, masks, populations, groupings, epochs, seeds -- and the one comparison it makes (``same``:
   tables equal, lists byte for byte), so that the CPU test can show that each planted slip of the twin fails that comparison on
   those cases.

CHUNK is the compaction's chunk (ROWS_CHUNK of csrc/ranenv_internal.h): at most 2048 cells of ONE unit.  Under the grouping by
members a chunk is a piece of a member's cells at one TTI ((envs of the member) x S contiguous cells), under the grouping by slices
a run of 2048 record rows t * B + b at one slice.  On the GPU test's handle (B 12, S 5) T * B * S = 60 T is a multiple of 4, so it
never lies nearer than 4 cells to a multiple of 2048: T 239 gives 7 x 2048 + 4 and T 273 gives 8 x 2048 - 4 cells, the nearest there
are.  The boundaries the kernels really have at that shape are the slices' runs of T * B = 12 T rows -- T 171: 2048 + 4 rows, T 341:
2 x 2048 - 4 rows -- and a member's cells at one TTI, which pass 2048 only on a wider batch (BIG: members of 2045, 2050 and 50 cells)."""
from __future__ import annotations

import numpy as np

CHUNK = 2048
TAG = 0x53485546
M32 = 0xFFFFFFFF
MEMBERS, SLICES = 0, 1


# ---- 1. the plain restatement ---------------------------------------------------------------------------------------------------------
def philox(c, k0, k1):
    c0, c1, c2, c3 = c
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return [c0, c1, c2, c3]


def fmix32(x):
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def permutation(n, seed, epoch, unit, kind, passes=None):
    """P(n, seed, epoch, unit, kind) as a list; ``passes``: a list that receives the walking passes of every position"""
    if n == 1:
        return [0]
    h = max(1, ((n - 1).bit_length() + 1) // 2)
    mask = (1 << h) - 1
    key = []
    for j in range(2):
        key += philox((epoch, unit, kind, TAG + j), seed & M32, (seed >> 32) & M32)
    out = []
    for i in range(n):
        x, walked = i, 0
        while True:
            left, right = x >> h, x & mask
            for r in range(8):
                left, right = right, left ^ (fmix32((right + key[r]) & M32) & mask)
            x, walked = (left << h) | right, walked + 1
            if x < n:
                break
        out.append(x)
        if passes is not None:
            passes.append(walked)
    return out


def row_order(mask, first_env, epochs, seed, grouping=MEMBERS):
    """The four tables of the header's text for ``mask`` [T][B][S] (nested sequences or an array): ({"inter": lists [epochs][N],
    "intra": ...}, {"inter": first, "intra": first}, {"inter": base lists per unit, "intra": ...})"""
    T, B, S = len(mask), len(mask[0]), len(mask[0][0])
    G = len(first_env) - 1
    bases = {"inter": [], "intra": []}
    if grouping == SLICES:
        assert G == 1
        bases["inter"].append([t * B + b for t in range(T) for b in range(B)])
        for s in range(S):
            bases["intra"].append([(t * B + b) * S + s for t in range(T) for b in range(B) if mask[t][b][s] != 0])
    else:
        for m in range(G):
            envs = range(first_env[m], first_env[m + 1])
            bases["inter"].append([t * B + b for t in range(T) for b in envs])
            bases["intra"].append([(t * B + b) * S + s for t in range(T) for b in envs for s in range(S) if mask[t][b][s] != 0])
    lists, firsts = {}, {}
    for kind, name in enumerate(("inter", "intra")):
        first = [0]
        for base in bases[name]:
            first.append(first[-1] + len(base))
        rows = []
        for k in range(epochs):
            row = []
            for u, base in enumerate(bases[name]):
                if base:
                    row += [base[j] for j in permutation(len(base), seed, k, u, kind)]
            rows.append(row)
        lists[name], firsts[name] = rows, first
    return lists, firsts, bases


# ---- 2. the GPU test's cases and its comparison ---------------------------------------------------------------------------------------
B, S = 12, 5
POPULATIONS = {"one": [0, 12], "three": [0, 5, 6, 12], "twelve": list(range(13))}
MASKS = ("ones", "zeros", "last_cell", "dead_slice", "bernoulli")
SEEDS = (0, 2 ** 33 + 5)
T_SHORT, T_PAST = 273, 239               # T * B * S = 8 x 2048 - 4 and 7 x 2048 + 4 cells
T_RUN_PAST, T_RUN_SHORT = 171, 341       # T * B = 2048 + 4 and 2 x 2048 - 4 rows: a slice's runs
BIG = dict(B=829, S=5, T=3, first_env=[0, 409, 819, 829])      # members of 2045, 2050 and 50 cells per TTI


def make_mask(kind, T, B=B, S=S, seed=0):
    """int8 [T, B, S] of zeros and ones"""
    rng = np.random.default_rng(1000 + seed)
    if kind == "ones":
        m = np.ones((T, B, S), dtype=np.int8)
    elif kind == "zeros":
        m = np.zeros((T, B, S), dtype=np.int8)
    elif kind == "last_cell":
        m = np.zeros((T, B, S), dtype=np.int8)
        m[-1, -1, -1] = 1
    elif kind == "dead_slice":               # an empty unit between full ones under SLICES
        m = np.ones((T, B, S), dtype=np.int8)
        m[:, :, 2] = 0
    elif kind == "bernoulli":
        m = (rng.random((T, B, S)) < 0.5).astype(np.int8)
    else:
        raise ValueError(kind)
    return m


def cases():
    """(name, T, mask kind, population name, per_slice, epochs, seed): every mask at T 1 and T 8 under every population and under
    the slices' grouping, epochs 1 and 3 and both seeds alternating so that each occurs under every grouping; the four boundary
    lengths on the Bernoulli mask, which has every unit partly live."""
    out, i = [], 0
    for T in (1, 8):
        for mask in MASKS:
            for g, (pop, per_slice) in enumerate((("one", False), ("three", False), ("twelve", False), ("one", True))):
                out.append((f"T{T}-{mask}-{pop}{'-slices' if per_slice else ''}", T, mask, pop, per_slice, (1, 3)[(i + g) % 2], SEEDS[((i + g) // 2) % 2]))
            i += 1
    for T in (T_SHORT, T_PAST, T_RUN_PAST, T_RUN_SHORT):
        for pop, per_slice in (("three", False), ("one", True)):
            out.append((f"T{T}-bernoulli-{pop}{'-slices' if per_slice else ''}", T, "bernoulli", pop, per_slice, 1 if T > 200 else 3, SEEDS[T % 2]))
    return out


def same(got, want):
    """The GPU test's comparison of two ``ppo_row_order`` dicts: None where they agree -- tables equal, lists of the same shape and
    bytes -- else a word on the first difference"""
    for kind in ("inter", "intra"):
        f_got, f_want, o_got, o_want = got["first_" + kind], want["first_" + kind], got["order_" + kind], want["order_" + kind]
        if (f_got is None) != (f_want is None) or (o_got is None) != (o_want is None):
            return f"{kind}: one side has no lists"
        if f_got is None:
            continue
        f_got, f_want = np.asarray(f_got), np.asarray(f_want)
        if f_got.dtype != np.int32 or f_got.shape != f_want.shape or not np.array_equal(f_got, f_want):
            return f"first_{kind}: {f_got.tolist()} != {f_want.tolist()}"
        o_got = o_got.cpu().numpy() if hasattr(o_got, "cpu") else np.asarray(o_got)
        o_want = np.asarray(o_want)
        if o_got.dtype != np.int32 or o_got.shape != o_want.shape:
            return f"order_{kind}: {o_got.dtype} {o_got.shape} != int32 {o_want.shape}"
        if o_got.tobytes() != o_want.tobytes():
            k, p = np.argwhere(o_got != o_want)[0]
            return f"order_{kind}[{k}, {p}]: {o_got[k, p]} != {o_want[k, p]}"
    return None
