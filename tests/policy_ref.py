"""A float64 statement of RANENV_POLICY_NETWORK with a rigorous error bound, for the tests of the policy kernel.

``adapters.ibsched_policy_actions`` is the normative float32 restatement; this module is its high-precision twin.  The forward
runs in float64 from the float32 (W, b) layers, and every output carries a bound ``t`` on the distance between the float64 value
and any float32 evaluation of the same net in any summation order (the device's MFMA GEMM, torch's CPU GEMM):

    magnitude  a_l = |W_l| m_{l-1} + |b_l|          m_0 = |x|,  m_l = |h_l| + t_l  (h_l the float64 activation)
    bound      t_l = |W_l| t_{l-1} + (K_l + 2) u a_l      u = 2^-24, K_l the padded input width of layer l
    tanh       scales t by its largest slope within z +- t, then adds TANH_ULPS float32 ulps of its result (the device's tanhf)
    relu       passes t through, or makes it 0 where z < -t (both sides then give exactly 0)
    clamp      passes t through, or makes it 0 where |v| > 1 + t (both sides then give exactly -1 or 1)

(the classical running-error bound of a float32 dot product of length K plus the bias add, with one more unit per product; the
inputs are float32 values, so t_0 = 0).  The bound does not depend on rounding luck, so a test built on it never flakes, and it
is orders of magnitude below the error of an indexing, padding or tile bug.

The epilogue -- sorted action mask, Box-Muller noise, clamp, argmax with the lowest index on ties, categorical draw -- is
computed in float64 from the reference outputs, with the rules of include/ranenv.h.  ``check_actions`` compares a device's
actions with it: scores within their bound, masked positions exactly -1, intra choices equal wherever the reference's margin
exceeds the logits' bound.
"""
from __future__ import annotations

import numpy as np

U32 = 2.0 ** -24          # unit roundoff of float32
TANH_ULPS = 4             # accuracy of the device's tanhf, with room to spare
NET_ROWS = 32             # rows of one policy workgroup (ranenv_internal.h)
POLICY_TAG = 0x504F4C00   # counter word c3 of the policy's Philox draws
HALF_LN_2PI = 0.9189385332046727


def pad32(n: int) -> int:
    return (int(n) + 31) // 32 * 32


def _np(x, dtype=np.float64):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=dtype)


def mlp64(x, layers, act: str, t0=None):
    """float64 forward of a (W, b) stack (hidden layers with ``act`` between them, none after the last) on float32-valued
    inputs ``x`` [R, K], or on inputs that carry a bound of their own: |device input - x| <= ``t0`` [R, K].  Returns
    (y [R, N], t [R, N]): outputs and their bound."""
    h = _np(x)
    t = np.zeros_like(h) if t0 is None else _np(t0)
    m = np.abs(h) + t
    for i, (w, b) in enumerate(layers):
        w, b = _np(w), _np(b)
        aw = np.abs(w)
        z = h @ w.T + b
        a = m @ aw.T + np.abs(b)
        K = pad32(w.shape[1])
        # (+ the float64 reference's own rounding, + products flushed below float32's normal range)
        t = t @ aw.T + (K + 2) * U32 * a + 2.0 ** -50 * a + K * 2.0 ** -125
        if i < len(layers) - 1:
            if act == "tanh":       # slope sech^2 at the point of the interval z +- t nearest to 0
                t = t / np.cosh(np.maximum(np.abs(z) - t, 0.0)) ** 2
                z = np.tanh(z)
                t = t + TANH_ULPS * 2.0 ** -23 * np.abs(z) + 2.0 ** -126
            elif act == "relu":     # below -t the device's value is negative too: both give exactly 0
                t = np.where(z < -t, 0.0, t)
                z = np.maximum(z, 0.0)
            else:
                raise ValueError(act)
        h = z
        m = np.abs(h) + t
    return h, t


def sorted_mask(mask_inter):
    """adapters.sorted_action_mask in numpy: position j of a row is active iff j >= S - (number of active slices)."""
    mk = _np(mask_inter, np.int64) != 0
    S = mk.shape[-1]
    return np.arange(S)[None, :] >= S - mk.sum(axis=-1, keepdims=True)


def philox_draws(env_ids, episode, step, S: int, seed: int, tag: int = POLICY_TAG):
    """A policy's Philox words (counter word c3 = ``tag`` + position) for [B] envs x S positions / slices: 4 arrays [B, S] of
    uint64 holding 32-bit words."""
    from intent_radio_sched_multi_slice_amd.adapters import philox4x32_10
    col = lambda a: np.asarray(_np(a, np.int64), dtype=np.int64).reshape(-1, 1) & 0xFFFFFFFF  # noqa: E731
    c3 = tag + np.arange(S, dtype=np.int64)[None, :]
    return philox4x32_10(col(env_ids), col(episode), col(step), c3, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)


def box_muller(draws):
    u1 = (draws[0].astype(np.float64) + 1.0) * 2.0 ** -32
    u2 = draws[1].astype(np.float64) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def gauss_noise(tag: int, env_ids, episode, step, S: int, seed: int):
    """z float64 [B, S]: the standard normal draws of the policy with Philox tag ``tag``."""
    return box_muller(philox_draws(env_ids, episode, step, S, seed, tag))


def intra_input(obs_intra, mask_intra, layout: str):
    """The intra net's input rows [B*S, K]: obs_intra, or [mask_intra, obs_intra] for the "mask_obs" layout."""
    oi = _np(obs_intra, np.float32)
    B, S = oi.shape[:2]
    x = oi.reshape(B * S, -1)
    if layout == "mask_obs":
        x = np.concatenate([_np(mask_intra, np.float32).reshape(B * S, -1), x], axis=1)
    elif layout != "obs":
        raise ValueError(layout)
    return x


def inter_epilogue(out, out_t, mask_inter, stochastic: bool, draws=None):
    """Scores [B, S] and their bound from the inter net's outputs [B, 2S] (mean | log_std) and bounds."""
    S = out.shape[1] // 2
    mean, ls, t_mean, t_ls = out[:, :S], out[:, S:], out_t[:, :S], out_t[:, S:]
    bound = t_mean.copy()
    if stochastic:
        z = box_muller(draws)
        sd = np.exp(ls)
        mean = mean + sd * z
        bound = bound + sd * np.abs(z) * np.expm1(t_ls) + 1e-12 * (1.0 + sd * np.abs(z))   # (double transcendental libraries)
    active = sorted_mask(mask_inter)
    scores = np.where(active, np.clip(mean, -1.0, 1.0), -1.0)
    bound = np.where(np.abs(mean) - bound > 1.0, 0.0, bound)      # clamped on both sides: exactly -1 or 1
    return scores, np.where(active, bound, 0.0), active


def intra_epilogue(lg, lg_t, stochastic: bool, draws=None):
    """Choices [B, S] uint8 and a mask of the rows whose choice is certain (margin above the logits' bound)."""
    if not stochastic:
        win = np.argmax(lg, axis=-1)[..., None]                  # (numpy: the first maximum, the kernel's tie rule)
        gap = np.take_along_axis(lg, win, -1) - lg
        need = np.take_along_axis(lg_t, win, -1) + lg_t
        safe = np.all((np.arange(3) == win) | (gap > need), axis=-1)     # the winner beats every other logit beyond both bounds
        return win[..., 0].astype(np.uint8), safe
    mx = lg.max(axis=-1, keepdims=True)
    e = np.exp(lg - mx)
    tot = e.sum(axis=-1)
    c0, c1 = e[..., 0] / tot, (e[..., 0] + e[..., 1]) / tot
    u = draws[2].astype(np.float64) * 2.0 ** -32
    ch = np.where(u < c0, 0, np.where(u < c1, 1, 2)).astype(np.uint8)
    T = lg_t.max(axis=-1)
    margin = np.expm1(2.0 * T) + 1e-12              # how far a cumulative probability moves under logit errors <= T
    safe = (np.abs(u - c0) > margin) & (np.abs(u - c1) > margin)
    return ch, safe


class PolicyRef:
    """The float64 reference of one TTI's actions.  ``inter`` / ``intra``: (layers, activation) as policy_net_layers
    returns them (intra None = no intra net).  ``env_ids`` / ``episode`` / ``step``: [B] Philox counters (stochastic)."""

    def __init__(self, obs_inter, mask_inter, inter, obs_intra=None, mask_intra=None, intra=None, stochastic=False, seed=0,
                 layout="obs", env_ids=None, episode=None, step=None, forward=None):
        forward = forward or mlp64
        x = _np(obs_inter, np.float32)
        B, S = x.shape[0], x.shape[1] // 10
        self.B, self.S, self.stochastic = B, S, bool(stochastic)
        draws = philox_draws(env_ids, episode, step, S, seed) if stochastic else None
        out, out_t = forward(x, *inter)
        self.out, self.out_t = out, out_t
        self.scores, self.score_bound, self.active = inter_epilogue(out, out_t, mask_inter, stochastic, draws)
        self.intra = self.intra_safe = self.logits = None
        if intra is not None:
            lg, lg_t = forward(intra_input(obs_intra, mask_intra, layout), *intra)
            self.logits, self.logit_bound = lg.reshape(B, S, 3), lg_t.reshape(B, S, 3)
            self.intra, self.intra_safe = intra_epilogue(self.logits, self.logit_bound, stochastic, draws)


def check_actions(ref: PolicyRef, scores, intra=None, rows=None, min_safe: float = 0.9):
    """Assert that device actions match the reference on env ``rows`` (default all).  Returns the number of (env, slice)
    intra rows compared (0 without an intra net)."""
    rows = np.arange(ref.B) if rows is None else np.asarray(rows)
    sc = _np(scores)[rows]
    want, bnd, act = ref.scores[rows], ref.score_bound[rows], ref.active[rows]
    assert np.all(sc[~act] == -1.0), "a masked position does not score exactly -1"
    err = np.abs(sc - want)
    bad = act & ~(err <= bnd)
    if bad.any():
        b, j = np.argwhere(bad)[0]
        raise AssertionError(f"{int(bad.sum())} scores outside the bound; first env {int(rows[b])} position {int(j)}: "
                             f"device {sc[b, j]!r} reference {want[b, j]!r} bound {bnd[b, j]:.3g}")
    if ref.intra is None:
        assert intra is None
        return 0
    ic = _np(intra, np.int64)[rows]
    safe = ref.intra_safe[rows]
    assert safe.mean() >= min_safe, f"only {safe.mean():.1%} of the intra rows are decidable"
    wrong = safe & (ic != ref.intra[rows])
    if wrong.any():
        b, s = np.argwhere(wrong)[0]
        raise AssertionError(f"{int(wrong.sum())} intra choices differ; first env {int(rows[b])} slice {int(s)}: "
                             f"device {int(ic[b, s])} reference {int(ref.intra[rows][b, s])} logits {ref.logits[rows][b, s]}")
    assert np.all((ic >= 0) & (ic <= 2))
    return int(safe.sum())


def injected_inputs(rng, B: int, S: int, Us: int):
    """Dense distinct observations on several scales (about 0.1, 1 and 5: tanh saturates, relu cuts), exact zeros and
    negative values included: float32 obs_inter [B, 10S] and obs_intra [B, S, 2Us+9]."""
    def draw(shape):
        scale = rng.choice([0.1, 1.0, 5.0], size=shape)
        v = rng.standard_normal(shape) * scale
        v[rng.random(shape) < 0.05] = 0.0
        return v.astype(np.float32)
    return draw((B, 10 * S)), draw((B, S, 2 * Us + 9))
