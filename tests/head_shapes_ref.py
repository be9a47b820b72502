"""The shape grid of the head / off-policy kernel family -- the head policies (policy_body<HEAD>), ranenv_head_kernel, the replay ring
and sampler, ranenv_sac_target_kernel -- stated once, with its fixtures and checks; tests/test_head_shapes_cpu.py and
tests/test_gpu_head_shapes.py run on it.

What the grid reaches that tests/head_policy_ref.SIZES and tests/sac_ref.CASES (S 5 and S 10, Us 10, widths on the 64 grid) do not:

    S   Us   U    the SAC target                         the head kernel            the sampler
    1   16   16   critic input 11 -> 32                  one wave, n = 16           a row of 5 words (fewer than the 16 lanes)
    3   16   40   33 -> 64                               one wave
    6    5   25   66 -> 96, the + 36 LDS stride          two waves
    8   12   60   88 -> 96; 32 S = 256: the last S at    two waves, n = 11, 12
                  which no thread owns a second pair
    16  16  256   176 -> 192, every thread two pairs     four waves, n = 16         a row of 80 words (five passes)

and nets whose widths leave the 32 grid (1, 7, 33, 100, 255, 480, 511), depths 1 to 4, both activations, the actor and the critics
differing -- a critic wider and deeper than its actor and the reverse, so that the kernels' LDS row stride comes from either side.

THE YARDSTICK.  The rigorous bounds of sac_ref / head_policy_ref hold for ANY float32 evaluation, so at wide nets they are loose: at
S 16 under [512, 512] nets the critics' sum in place of their minimum stays inside the target's bound on 41 of the 49 live rows.  ``yardstick`` is the
rule of ppo_update_ref.check_against_twin: per output tensor, over the rows of the call,
    e_dev = |device - ref|_2 / |ref|_2,   e_32 the same figure of the float32 torch restatement,   e_dev <= 8 max(e_32, 1e-6).

``restate`` is adapters.sac_targets_torch once more (bit for bit: test_head_shapes_cpu holds it to that) with a ``slip`` argument: the
mistakes of sac_ref.SLIPS and four that only the new shapes can see (SHAPE_SLIPS).
"""
from __future__ import annotations

import numpy as np
import torch

from tests import head_policy_ref as hr
from tests import policy_ref as pr
from tests import sac_ref as sr


def _size(S, Us, U):
    return dict(n_slices=S, n_ues=U, n_rbs=25, rbs_per_rbg=1, max_ues_slice=Us, min_slices=1, min_ues=1)


# the environment shapes (keywords of make_mult_slice_workload, as gpu_common.shaped_workload builds them)
ENV_SHAPES = {1: _size(1, 16, 16), 3: _size(3, 16, 40), 6: _size(6, 5, 25), 8: _size(8, 12, 60), 16: _size(16, 16, 256)}
# name -> (S, actor widths, actor activation, critic widths, critic activation)
CASES = {"S1_7x100_96": (1, [7, 100], "relu", [96], "tanh"),                        # depth 2 over depth 1; 11 -> 32
         "S3_96x160_33": (3, [96, 160], "relu", [33], "tanh"),                      # the actor wider and deeper: ldm is the actor's
         "S6_40x24_160x7x96": (6, [40, 24], "tanh", [160, 7, 96], "relu"),          # the critic wider and deeper: ldm is the critic's
         "S8_255_511x1": (8, [255], "tanh", [511, 1], "relu"),
         "S16_256x256_480x33": (16, [256, 256], "relu", [480, 33], "tanh"),
         "S16_64x4_100x7x255x32": (16, [64] * 4, "relu", [100, 7, 255, 32], "tanh"),  # depth 4 on both sides
         "S16_512x512": (16, [512, 512], "tanh", [512, 512], "relu")}
TAIL_CASES = ("S1_7x100_96", "S16_256x256_480x33")       # row tails: the S 1 case and an S 16 case
TAILS = (1, 31, 32, 33, 64, 65)
N_ROWS, GAMMA, ENT_COEF = sr.N_ROWS, sr.GAMMA, sr.ENT_COEF
SEED, DRAW = 77, 3
FACTOR, FLOOR = 8.0, 1e-6          # ppo_update_ref.check_against_twin's constants
NET_ROWS = 32                      # rows of a workgroup of the net kernels
SHAPE_SLIPS = ("second_pair_dropped", "logp_short", "terms_stride_16", "action_cols_pad32")
SLIPS = sr.SLIPS + SHAPE_SLIPS


def pad32(x):
    return (x + 31) // 32 * 32


def slip_applies(slip, S):
    """Whether ``slip`` changes anything at S slices: the second pair exists above 256 pairs, stride 16 is the right stride at S 16, and
    10 S is its own multiple of 32 at S 16."""
    return {"second_pair_dropped": NET_ROWS * S > 256, "terms_stride_16": S != 16, "action_cols_pad32": pad32(10 * S) != 10 * S}.get(slip, True)


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
def sac_nets(case, seed=31):
    """(actor, q1, q2) of a CASES entry, in sac_ref.sac_nets' manner for any S: the log_std half of the actor's output bias is
    LOG_STD_BIAS[0] (around the lower clamp) at positions 0, 4, 8, .., LOG_STD_BIAS[1] (above the upper clamp) at 1, 5, 9, .. and
    LOG_STD_BIAS[2] elsewhere, so a quarter of the positions each meets a clamp and the tanh saturates on a share that does not shrink with S.
    S 1 has one position: its log_std row is scaled up instead, so that the rows spread over both clamps."""
    S, aw, aact, qw, qact = CASES[case]
    actor = hr.mlp([10 * S] + aw + [2 * S], aact, seed, sr.OUT_SCALE)
    lo, hi, mid = sr.LOG_STD_BIAS
    with torch.no_grad():
        if S == 1:                     # log_std over the case's rows: mean -9, deviation 12
            raw = actor(torch.from_numpy(sac_inputs(case)[0]))[:, 1]
            k = 12.0 / float(raw.std())
            actor[-1].weight[1] *= k
            actor[-1].bias[1] = (actor[-1].bias[1] - raw.mean()) * k - 9.0
        else:
            j = torch.arange(S)
            actor[-1].bias[S:] += torch.where(j % 4 == 0, lo, torch.where(j % 4 == 1, hi, mid)).to(torch.float32)
    q1 = hr.mlp([11 * S] + qw + [1], qact, seed + 1)
    q2 = hr.mlp([11 * S] + qw + [1], qact, seed + 2)
    return actor, q1, q2


def sac_inputs(case, n=N_ROWS, seed=5):
    """sac_ref.sac_inputs at the case's S."""
    S = CASES[case][0]
    rng = np.random.default_rng(seed)
    shape = (n, 10 * S)
    obs = rng.standard_normal(shape) * rng.choice([0.05, 0.25, 1.0], size=shape) * sr.OBS_SCALE
    obs[rng.random(shape) < 0.05] = 0.0
    reward = (rng.standard_normal(n) * 2.0).astype(np.float32)
    done = (rng.random(n) < 1.0 / 3.0).astype(np.uint8)
    return obs.astype(np.float32), reward, done


def head_nets(case, dist, seed=21):
    """(actor, log_std or None, critic) for the head policy tests, head_policy_ref.head_nets on the case's widths: the actor of the
    case's actor shape, the value net of its critics' shape on the observation alone."""
    S, aw, aact, qw, qact = CASES[case]
    actor = hr.mlp([10 * S] + aw + [S if dist == "gauss_clip" else 2 * S], aact, seed, hr.OUT_SCALE)
    if dist == "gauss_tanh":
        with torch.no_grad():
            actor[-1].bias[S:] += 1.0
    g = torch.Generator().manual_seed(seed + 1)
    log_std = ((torch.rand(S, generator=g) * 2 - 1) * 1.5).to(torch.float32) if dist == "gauss_clip" else None
    critic = hr.mlp([10 * S] + qw + [1], qact, seed + 2)
    return actor, log_std, critic


_SHARED = {}


def sac_case(case):
    """The case's inputs, nets, noise, the float64 references of both modes and the float32 restatements: computed once per process,
    shared by every test, never modified."""
    if case not in _SHARED:
        from intent_radio_sched_multi_slice_amd import adapters
        obs, reward, done = sac_inputs(case)
        nets = sac_nets(case)
        S = CASES[case][0]
        z = sr.noise(N_ROWS, S, SEED, DRAW)
        ref = {True: sr.SacRef(obs, reward, done, *nets, GAMMA, ENT_COEF, z), False: sr.SacRef(obs, reward, done, *nets, GAMMA, ENT_COEF, None)}
        got = {st: adapters.sac_targets_torch(obs, reward, done, *nets, GAMMA, ENT_COEF, st, SEED, DRAW) for st in (True, False)}
        _SHARED[case] = dict(name=case, S=S, obs=obs, reward=reward, done=done, nets=nets, z=z, ref=ref, got=got)
    return _SHARED[case]


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------
SAC_OUTPUTS = ("next_action", "next_logp", "q", "target")


def rel_error(value, want):
    """|value - want|_2 / |want|_2 in float64 (inf when the difference is not finite)."""
    want = np.asarray(want, dtype=np.float64)
    n = float(np.linalg.norm(want))
    assert n > 0.0, "the reference is zero"
    with np.errstate(invalid="ignore", over="ignore"):
        d = float(np.linalg.norm(pr._np(value).astype(np.float64) - want))
    return d / n if np.isfinite(d) else float("inf")


def yardstick_ratios(dev, ref, f32, names=SAC_OUTPUTS, rows=None):
    """name -> (e_dev / max(e_32, FLOOR), e_dev, e_32) of the outputs ``names``: ``dev`` and ``f32`` dicts of arrays, ``ref`` an object
    with the float64 values as attributes (or a dict).  ``rows``: the first rows of ``ref`` / ``f32`` that ``dev`` holds."""
    out = {}
    for k in names:
        want = ref[k] if isinstance(ref, dict) else getattr(ref, k)
        mine = pr._np(f32[k])
        if rows is not None:
            want, mine = want[:rows], mine[:rows]
        e_dev, e_32 = rel_error(dev[k], want), rel_error(mine, want)
        out[k] = (e_dev / max(e_32, FLOOR), e_dev, e_32)
    return out


def check_yardstick(dev, ref, f32, what, names=SAC_OUTPUTS, rows=None):
    """Asserts e_dev <= FACTOR max(e_32, FLOOR) for every output; prints and returns the ratios."""
    ratios = yardstick_ratios(dev, ref, f32, names, rows)
    for k, (ratio, e_dev, e_32) in ratios.items():
        print(f"{what} {k}: device / yardstick {ratio:.3g} (device {e_dev:.3g}, float32 torch {e_32:.3g})")
    bad = {k: v for k, v in ratios.items() if not v[0] <= FACTOR}
    assert not bad, f"{what}: error beyond {FACTOR:g} x the float32 restatement's: " + ", ".join(
        f"{k} device {e:.3g} float32 torch {e32:.3g}" for k, (_, e, e32) in bad.items())
    return {k: v[0] for k, v in ratios.items()}


# ---- the restatement with slips -------------------------------------------------------------------------------------------------------
def restate(next_obs, reward, done, actor, q1, q2, gamma, ent_coef, stochastic=True, seed=0, draw=0, slip=None):
    """adapters.sac_targets_torch, with ``slip`` one of SLIPS planted the way the kernel would make it (None: none).  The workgroup's
    geometry matters to three of them: 32 rows, the flat pair index i = (row % 32) S + j, the terms of log pi at i."""
    from intent_radio_sched_multi_slice_amd import adapters
    from intent_radio_sched_multi_slice_amd.batched_env import policy_net_layers
    assert slip is None or slip in SLIPS, slip
    x = torch.as_tensor(next_obs).detach().to(torch.float32)
    n, S = x.shape[0], x.shape[1] // 10
    nets = [policy_net_layers(net, None, k, o) for net, k, o in ((actor, 10 * S, 2 * S), (q1, 11 * S, 1), (q2, 11 * S, 1))]
    fwd = lambda inp, k: adapters._mlp_forward(inp, nets[k][0], nets[k][1])  # noqa: E731
    out = fwd(x, 0).to(torch.float64)
    mu, ls = out[:, :S], out[:, S:]
    if slip != "unclamped_log_std":
        ls = ls.clamp(adapters.LOG_STD_MIN, adapters.LOG_STD_MAX)
    z = torch.from_numpy(adapters.sac_target_noise(n, S, seed, draw)) if stochastic else torch.zeros_like(mu)
    a = torch.tanh(mu + torch.exp(ls) * z)
    a32 = a.to(torch.float32)
    eps = 0.0 if slip == "no_epsilon" else 1e-6
    terms = (((-0.5 * z) * z - ls) - adapters.HALF_LN_2PI) - torch.log((1.0 - a * a) + eps)
    if slip == "terms_stride_16":      # row r of a workgroup reads the flat terms at 16 r + j (what lies behind the 32 S terms: zeros)
        read = torch.zeros_like(terms)
        for w0 in range(0, n, NET_ROWS):
            flat = torch.zeros(NET_ROWS * 16 + 16, dtype=torch.float64)
            blk = terms[w0:w0 + NET_ROWS]
            flat[:blk.numel()] = blk.reshape(-1)
            for r in range(blk.shape[0]):
                read[w0 + r] = flat[16 * r:16 * r + S]
        terms = read
    logp = torch.zeros(n, dtype=torch.float64)
    for j in range(S - 1 if slip == "logp_short" else S):
        logp = logp + terms[:, j]
    act = a32
    if slip == "second_pair_dropped":  # the pairs i >= 256 of a workgroup never reach the critics' rows
        i = (torch.arange(n) % NET_ROWS)[:, None] * S + torch.arange(S)[None, :]
        act = torch.where(i < 256, a32, torch.zeros_like(a32))
    if slip == "action_cols_pad32":    # the actions land at column pad32(10 S) + j; the critics read columns 10 S .. 11 S - 1
        shift = pad32(10 * S) - 10 * S
        act = torch.zeros_like(a32)
        if shift < S:
            act[:, shift:] = a32[:, :S - shift]
    xa = torch.cat([x, act], dim=1)
    q = torch.cat([fwd(xa, 1), fwd(xa, 2)], dim=1)
    q64 = q.to(torch.float64)
    qmin = q64.sum(dim=1) if slip == "sum_not_min" else torch.minimum(q64[:, 0], q64[:, 1])
    r = torch.as_tensor(reward).detach().to(torch.float32).to(torch.float64)
    nd = torch.where(torch.as_tensor(done).detach() != 0, 0.0, 1.0).to(torch.float64)
    if slip == "through_done":
        nd = torch.ones_like(nd)
    ent = 0.0 if slip == "no_entropy" else float(ent_coef)
    target = (r + nd * (float(gamma) * (qmin - ent * logp))).to(torch.float32)
    return {"target": target, "next_action": a32, "next_logp": logp.to(torch.float32), "q": q}


# ---- directed scenario tables for the head kernel -----------------------------------------------------------------------------------------
MEMBER_COUNTS = (0, 1, 7, 8, 9, 15, 16)        # UEs of a slice: the edges of np_sum16_lds' blocks of eight, none and all 16


def directed_counts(S, U, Us=16):
    """Per scenario, the UEs of each of the S slices: MEMBER_COUNTS dealt round the slices, rotated by one from scenario to scenario.
    S 1 leaves the 0 out: a scenario there has its one slice (the generators never make a scenario without a slice)."""
    pool = [c for c in MEMBER_COUNTS if c <= Us and (S > 1 or c > 0)]
    scenarios = [[pool[(i + s) % len(pool)] for s in range(S)] for i in range(len(pool))]
    assert all(sum(counts) <= U for counts in scenarios), (S, U)
    return scenarios


def directed_tables(S, U, Us=16, seed=5):
    """ScenarioTables whose scenario i has directed_counts(S, U)[i] UEs in its slices (a slice of 0 UEs is inactive), through
    set_from_reference as test_gpu_member_lines._directed builds them, unsorted (SchedTWC's enable_sort_slices=False)."""
    from intent_radio_sched_multi_slice_amd.scenario import SLICE_TEMPLATES, ScenarioTables, slice_template_dict
    rng = np.random.default_rng(seed + S)
    scen = directed_counts(S, U, Us)
    t = ScenarioTables.empty(len(scen), S, U, Us)
    for i, counts in enumerate(scen):
        ues = rng.choice(U, sum(counts), replace=False)
        bsa, sua = np.zeros((1, S)), np.zeros((S, U))
        req = {f"slice_{s}": {} for s in range(S)}
        used = 0
        for s, cnt in enumerate(counts):
            if cnt == 0:
                continue
            bsa[0, s] = 1
            req[f"slice_{s}"] = slice_template_dict((s + i) % len(SLICE_TEMPLATES))
            sua[s, ues[used:used + cnt]] = 1
            used += cnt
        t.set_from_reference(i, bsa, sua, req, False)
    return t, scen
