"""What the tests of the SAC update share (tests/test_sac_update_cpu.py, tests/test_gpu_sac_update.py): the cases, their nets, a synthetic
batch for the CPU, the packed-gradient layout, the comparison of a device step with the torch twin (``adapters.sac_update_reference``)
under the project's yardstick, the conditions the inputs must meet, and the GPU fixture: an env of the case's shape whose batch comes
out of a ring that a real ``collect_replay`` filled.

The cases (actor / critics) take their environment shapes from tests/head_shapes_ref.py (S 5: the native shape of head_policy_ref), so
the critics' input widths 11 S = 55, 11, 66, 176 hit the LDS strides those tests hit: 64 + 4, 32 + 36, 96 + 36, 192 + 4.

THE YARDSTICK is ppo_update_ref.check_against_twin's: per gradient tensor e_dev = |device - t64|_2 / |t64|_2 <= 8 max(e_32, 1e-6) with e_32
the same figure of the float32 twin; a statistic s: |dev - t64| <= 8 max(|t32 - t64|, 1e-6 max(1, |t64|)).
"""
from __future__ import annotations

import numpy as np
import torch

from tests import head_policy_ref as hr
from tests import head_shapes_ref as hs
from tests import policy_ref as pr
from tests import ppo_update_ref as pu
from tests import sac_ref as sr

# name -> (S, actor widths, actor activation, critic widths, critic activation)
CASES = {"base": (5, [24], "relu", [40, 24], "tanh"), "deg": (1, [7, 100], "relu", [96], "tanh"),
         "stride": (6, [40, 24], "tanh", [160, 7, 96], "relu"), "two_pair": (16, [64, 64], "relu", [64, 64], "relu")}
ENV_SHAPES = {5: hr.SIZES["S5U25"], 1: hs.ENV_SHAPES[1], 6: hs.ENV_SHAPES[6], 16: hs.ENV_SHAPES[16],
              3: hs.ENV_SHAPES[3], 8: hs.ENV_SHAPES[8], 10: hr.SIZES["S10U100"]}      # (3, 8, 10: tests/sac_update_shapes_ref.py's grid)
B, RING_SLOTS, ROWS = 12, 4, 96          # a ring of four TTIs of twelve envs; the longest batch: three tiles
NET_SEED, BATCH_SEED = 31, 5             # tests/test_sac_update_cpu.py holds the conditions on the inputs for these
SEED, DRAW = 77, 3
GAMMA, TAU, ENT_INIT = 0.99, 0.005, 0.2
Q_SCALE = 4.0                            # on the critics' output layers
S1_INPUT_GAIN = 32.0                     # S 1: on the actor's first layer, so that log_std varies over the rows by more than its float32 error
FACTOR, FLOOR = 8.0, 1e-6
TENSORS = ("actor", "q1", "q2")


def spec(case):
    """A case's tuple: ``case`` a name of CASES, or such a tuple itself (tests/sac_update_shapes_ref.py's grid)"""
    return CASES[case] if isinstance(case, str) else tuple(case)


def nets(case, seed=NET_SEED):
    """(actor, q1, q2) modules of a case, in head_shapes_ref.sac_nets' manner: the log_std half of the actor's output bias sits around
    the lower clamp at positions 0, 8, .., above the upper clamp at 1, 9, .., elsewhere at a small deviation -- more than half of the
    positions stay free; S 1 has one position, whose log_std row is scaled up over the synthetic batch instead (mean -9, deviation 12),
    so that the rows spread over both clamps.  The critics' output layers are scaled by Q_SCALE, so that their gradient is a fair share
    of the actor's.  The second critic's output bias is moved so that, over the synthetic batch under the actor's own actions (the
    actor pass's draws at first_row 0), each critic is the smaller one on about half of the rows and zero lies in the middle of the
    widest gap between two neighbouring values of Q1 - Q2 among the central quarter: no row comes near a tie."""
    S, aw, aact, qw, qact = spec(case)
    actor = hr.mlp([10 * S] + aw + [2 * S], aact, seed, sr.OUT_SCALE)
    lo, hi, mid = sr.LOG_STD_BIAS
    with torch.no_grad():
        if S == 1:
            actor[0].weight *= S1_INPUT_GAIN
            raw = actor(torch.from_numpy(_observations(case, ROWS, BATCH_SEED)))[:, 1]
            k = 12.0 / float(raw.std())
            actor[-1].weight[1] *= k
            actor[-1].bias[1] = (actor[-1].bias[1] - raw.mean()) * k - 9.0
        else:
            j = torch.arange(S)
            actor[-1].bias[S:] += torch.where(j % 8 == 0, lo, torch.where(j % 8 == 1, hi, mid)).to(torch.float32)
    q1, q2 = hr.mlp([11 * S] + qw + [1], qact, seed + 1, Q_SCALE), hr.mlp([11 * S] + qw + [1], qact, seed + 2, Q_SCALE)
    with torch.no_grad():
        from intent_radio_sched_multi_slice_amd.adapters import sac_actor_noise
        obs = torch.from_numpy(_observations(case, ROWS, BATCH_SEED))
        out = actor(obs).double()
        a = torch.tanh(out[:, :S] + torch.exp(out[:, S:].clamp(-20.0, 2.0)) * torch.from_numpy(sac_actor_noise(ROWS, S, SEED, DRAW, 0)))
        x = torch.cat([obs, a.float()], dim=1)
        d = torch.sort((q1(x) - q2(x))[:, 0].double()).values[3 * ROWS // 8:ROWS - 3 * ROWS // 8]
        k = int(torch.argmax(d[1:] - d[:-1]))
        q2[-1].bias += float(0.5 * (d[k] + d[k + 1]))
    return actor, q1, q2


def layers(net):
    """A module's (W, b) list as detached float32 CPU tensors"""
    return [(m.weight.detach().clone(), m.bias.detach().clone()) for m in net if isinstance(m, torch.nn.Linear)]


def case_layers(case, seed=NET_SEED):
    return tuple(layers(n) for n in nets(case, seed))


def _observations(case, n, seed):
    S = spec(case)[0]
    rng = np.random.default_rng(seed)
    shape = (n, 10 * S)
    obs = rng.standard_normal(shape) * rng.choice([0.05, 0.25, 1.0], size=shape) * sr.OBS_SCALE
    obs[rng.random(shape) < 0.05] = 0.0
    return obs.astype(np.float32)


def synthetic_batch(case, n=ROWS, seed=BATCH_SEED):
    """A batch shaped as ``replay_sample`` returns it, on the CPU: sac_ref.sac_inputs' observations, actions inside (-1, 1) with some on
    the boundary, rewards of both signs, a third of the rows terminal."""
    S = spec(case)[0]
    rng = np.random.default_rng(seed + 1000)
    action = np.tanh(rng.standard_normal((n, S)) * 1.5).astype(np.float32)
    action[rng.random((n, S)) < 0.05] = 1.0
    return {"obs": torch.from_numpy(_observations(case, n, seed)), "next_obs": torch.from_numpy(_observations(case, n, seed + 1)),
            "action": torch.from_numpy(action), "reward": torch.from_numpy((rng.standard_normal(n) * 2.0).astype(np.float32)),
            "done": torch.from_numpy((rng.random(n) < 1.0 / 3.0).astype(np.uint8))}


def head(batch, n):
    return {k: v[:n] for k, v in batch.items()}


def twin(case, batch, nets_, lec, dtype=torch.float64, **kw):
    """adapters.sac_update_reference on a case: ``nets_`` = (actor, q1, q2, q1_target, q2_target) layer lists"""
    from intent_radio_sched_multi_slice_amd.adapters import sac_update_reference
    _, _, aact, _, qact = spec(case)
    args = dict(gamma=GAMMA, tau=TAU, seed=SEED, draw=DRAW, act_actor=aact, act_critic=qact)
    args.update(kw)
    return sac_update_reference({k: torch.as_tensor(v).cpu() for k, v in batch.items()}, *nets_, lec, dtype=dtype, **args)


def packed_floats(net_layers):
    return sum(pu.pad32(w.shape[0]) * pu.pad32(w.shape[1]) + pu.pad32(w.shape[0]) for w, _ in net_layers)


def unpack_grad(flat, actor, critic, dtype=np.float64):
    """dev_grad [actor | q1 | q2 | log_ent_coef] in the packed layouts as {"actor", "q1", "q2": [(dW, db)], "log_ent_coef": float}; the
    padding must be exact zeros (ppo_update_ref.unpack_grad asserts it)."""
    flat = np.asarray(flat)
    af, qf = packed_floats(actor), packed_floats(critic)
    assert flat.shape == (af + 2 * qf + 1,), (flat.shape, af, qf)
    out, at = {}, 0
    for name, net, f in (("actor", actor, af), ("q1", critic, qf), ("q2", critic, qf)):
        out[name] = pu.unpack_grad(flat[at:at + f], net, [], dtype)["actor"]
        at += f
    out["log_ent_coef"] = float(flat[at])
    return out


def grad_ratios(dev, t64, t32, names=TENSORS + ("log_ent_coef",)):
    """{(tensor, layer, "W" | "b"): (e_dev / max(e_32, FLOOR), e_dev, e_32)} of the gradients ``names``; a twin gradient of zero fails"""
    out = {}
    for name in names:
        if name == "log_ent_coef":
            x64, x32, xd = float(t64[name]), float(t32[name]), float(dev[name])
            assert x64 != 0.0, "the twin's log_ent_coef gradient is zero"
            e_dev, e_32 = abs(xd - x64) / abs(x64), abs(x32 - x64) / abs(x64)
            out[(name, 0, "")] = (e_dev / max(e_32, FLOOR), e_dev, e_32)
            continue
        for li, (g64, g32, gd) in enumerate(zip(t64[name], t32[name], dev[name])):
            for which, x64, x32, xd in zip("Wb", g64, g32, gd):
                x64, x32, xd = (np.asarray(x, dtype=np.float64) for x in (x64, x32, xd))
                n64 = np.linalg.norm(x64)
                assert n64 > 0.0, f"{name} layer {li} {which}: the twin's gradient is zero"
                e_dev, e_32 = np.linalg.norm(xd - x64) / n64, np.linalg.norm(x32 - x64) / n64
                out[(name, li, which)] = (e_dev / max(e_32, FLOOR), e_dev, e_32)
    return out


def check_grads(dev, t64, t32, what, names=TENSORS + ("log_ent_coef",)):
    """Asserts the yardstick on every gradient tensor; prints and returns the worst ratio"""
    ratios = grad_ratios(dev, t64, t32, names)
    worst = max(r[0] for r in ratios.values())
    bad = {k: v for k, v in ratios.items() if not v[0] <= FACTOR}
    print(f"{what}: worst gradient error, device / float32 torch yardstick: {worst:.3g}")
    assert not bad, f"{what}: " + ", ".join(f"{k}: device {e:.3g}, float32 torch {e32:.3g}" for k, (_, e, e32) in bad.items())
    return worst


def check_stats(dev, s64, s32, what):
    """|dev - t64| <= 8 max(|t32 - t64|, 1e-6 max(1, |t64|)) for the eight statistics of one step (arrays [8])"""
    from intent_radio_sched_multi_slice_amd import _lib
    bad = []
    for i, name in enumerate(_lib.SAC_STATS):
        err, allowed = abs(dev[i] - s64[i]), FACTOR * max(abs(s32[i] - s64[i]), FLOOR * max(1.0, abs(s64[i])))
        print(f"{what} {name}: device {dev[i]:.9g} twin {s64[i]:.9g} (error {err:.3g}, allowed {allowed:.3g})")
        if not err <= allowed:
            bad.append(f"{name}: device {dev[i]:.9g}, twin {s64[i]:.9g}, allowed {allowed:.3g}")
    assert not bad, f"{what}: " + "; ".join(bad)


def conditions(case, batch, nets_, lec, first_row=0):
    """The figures the tests' inputs are held to, on one minibatch = the whole ``batch``: the critics' separation against sac_ref's
    rigorous float32 bounds on [obs | a32], the share of rows on which each critic is the smaller, and the clamp census of log_std."""
    from intent_radio_sched_multi_slice_amd.adapters import sac_actor_noise
    S, _, aact, _, qact = spec(case)
    actor, q1, q2 = pu.as_sequential(nets_[0], aact), pu.as_sequential(nets_[1], qact), pu.as_sequential(nets_[2], qact)      # (modules: they carry the activation)
    obs = torch.as_tensor(batch["obs"]).detach().cpu().numpy().astype(np.float32)
    n = obs.shape[0]
    z = sac_actor_noise(n, S, SEED, DRAW, first_row)
    ref = sr.SacRef(obs, np.zeros(n, np.float32), np.zeros(n, np.uint8), actor, q1, q2, GAMMA, float(np.exp(float(lec))), z)
    gap, bound = np.abs(ref.q[:, 0] - ref.q[:, 1]), ref.q_bound[:, 0] + ref.q_bound[:, 1]
    raw = ref.log_std_raw
    return {"separated": bool((gap > bound).all()), "q1_smaller": float((ref.q[:, 0] < ref.q[:, 1]).mean()), "q2_smaller": float((ref.q[:, 1] < ref.q[:, 0]).mean()),
            "clamped_low": int((raw < -20.0).sum()), "clamped_high": int((raw > 2.0).sum()), "free": float(((raw >= -20.0) & (raw <= 2.0)).mean()),
            "min_gap_over_bound": float((gap / bound).min())}


# ---- the GPU side ---------------------------------------------------------------------------------------------------------------------
def make_env(case, slabs=32, ent_coef="auto_%g" % ENT_INIT, bind=True, seed=NET_SEED):
    """A reset env of the case's shape under the case's actor ("gauss_tanh", stochastic) and critics, a ring of RING_SLOTS TTIs filled
    by one real ``collect_replay``, and -- ``bind`` -- the SAC binding.  Returns (env, (actor, q1, q2) layer lists)."""
    S = spec(case)[0]
    _, env, _ = hr.make_env(ENV_SHAPES[S], "64x64", "gauss_tanh", B, bind=False)
    actor, q1, q2 = nets(case, seed)
    env.set_head_policy_network(actor, "gauss_tanh", stochastic=True, seed=1)
    env.set_sac_critics(q1, q2)
    env.reset()
    env.bind_replay(RING_SLOTS)
    env.collect_replay(RING_SLOTS)
    if bind:
        env.sac_bind(ent_coef=ent_coef, slabs=slabs)
    return env, (layers(actor), layers(q1), layers(q2))


def sample(env, n, seed=9, draw=1):
    """``n`` transitions of the ring as tensors of the caller's own (``replay_sample`` reuses its buffers)"""
    return {k: v.clone() for k, v in env.replay_sample(n, seed=seed, draw=draw).items() if k != "index"}


def device_nets(env, names=("actor", "q1", "q2", "q1_target", "q2_target")):
    """The binding's nets read back: {name: [(W, b) on the host]}"""
    return {k: [(w.cpu(), b.cpu()) for w, b in env.sac_net_weights(k)] for k in names}


def device_state(env):
    """The whole trainable state as host bytes: the five nets, the moments and counters, the scalar"""
    out = {}
    for k, net in device_nets(env).items():
        for i, (w, b) in enumerate(net):
            out[f"{k}/w{i}"], out[f"{k}/b{i}"] = w.numpy().copy(), b.numpy().copy()
    for k in ("actor", "q1", "q2", "log_ent_coef"):
        for name, v in env.sac_state(k).items():
            out[f"{k}/{name}"] = v.cpu().numpy().copy()
    out["log_ent_coef"] = env.sac_log_ent_coef().cpu().numpy().copy()
    return out
