"""The SAC update without a GPU: the torch twin (adapters.sac_update_reference) against a plain torch module loop with three
torch.optim.Adam -- the step of examples/train_sac_on_device.py reordered to SB3's --, the conditions the shared test inputs must meet,
planted slips against the yardstick, the actor pass's noise rule on one row with Python integers, the state-dict round trip, and the
new exports of the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from intent_radio_sched_multi_slice_amd import _lib, adapters
from tests import ppo_update_ref as pu
from tests import sac_update_ref as su

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("ranenv_sac_bind", "ranenv_sac_update", "ranenv_sac_layout", "ranenv_sac_lds_bytes", "ranenv_sac_state",
               "ranenv_get_sac_net_weights", "ranenv_get_sac_log_ent_coef")
LEC = float(np.float32(np.log(su.ENT_INIT)))
_SHARED = {}


def shared(case):
    """The case's synthetic batch, nets and the twins of one step at lr 0 on all ROWS rows (computed once, never modified)."""
    if case not in _SHARED:
        batch = su.synthetic_batch(case)
        actor, q1, q2 = su.case_layers(case)
        nets_ = (actor, q1, q2, q1, q2)
        kw = dict(steps=1, minibatch=su.ROWS, lr=0.0)
        _SHARED[case] = dict(batch=batch, nets=nets_, t64=su.twin(case, batch, nets_, LEC, **kw), t32=su.twin(case, batch, nets_, LEC, torch.float32, **kw))
    return _SHARED[case]


@pytest.mark.parametrize("case", sorted(su.CASES))
def test_conditions_on_the_test_inputs(case):
    c = shared(case)
    for n in (su.ROWS, 65, 33):          # the batches the GPU tests cut from these rows
        got = su.conditions(case, su.head(c["batch"], n), c["nets"], LEC)
        print(case, n, got)
        assert got["separated"], got      # no float32 evaluation can pick the other critic
        assert got["q1_smaller"] >= 0.25 and got["q2_smaller"] >= 0.25, got
        assert got["clamped_low"] >= 1 and got["clamped_high"] >= 1 and got["free"] >= 0.5, got
    su.grad_ratios(c["t64"]["grad"], c["t64"]["grad"], c["t32"]["grad"])      # (asserts: no twin gradient tensor is zero)


@pytest.mark.parametrize("case", ("base", "stride"))
def test_twin_agrees_with_a_plain_torch_module_loop(case):
    """Three steps of SB3's order -- coefficient read, critic step, actor step under the new critics, coefficient step, polyak -- with
    torch modules and torch.optim.Adam; the twin's nets, scalar and statistics at 1e-9."""
    S, _, aact, _, qact = su.CASES[case]
    batch, n, steps, lr = su.synthetic_batch(case), 32, 3, 1e-3
    al, q1l, q2l = su.case_layers(case)
    t = su.twin(case, batch, (al, q1l, q2l, q1l, q2l), LEC, steps=steps, minibatch=n, lr=lr)
    f64 = lambda ls, act: pu.as_sequential(ls, act).double()  # noqa: E731
    actor, q1, q2, q1t, q2t = f64(al, aact), f64(q1l, qact), f64(q2l, qact), f64(q1l, qact), f64(q2l, qact)
    lec = torch.nn.Parameter(torch.tensor(LEC, dtype=torch.float64))
    opt_q = torch.optim.Adam(list(q1.parameters()) + list(q2.parameters()), lr=lr, eps=1e-8)
    opt_pi, opt_a = torch.optim.Adam(actor.parameters(), lr=lr, eps=1e-8), torch.optim.Adam([lec], lr=lr, eps=1e-8)

    def act_of(obs, z):
        out = actor(obs)
        mu, ls = out[:, :S], out[:, S:].clamp(-20.0, 2.0)
        g = mu + torch.exp(ls) * z
        a = torch.tanh(g)
        # (the Gaussian's log-probability of g = mu + sigma z written in z: Normal(mu, sigma).log_prob(g) forms (g - mu) / sigma, which at
        #  sigma = exp(-20) loses nine digits to cancellation -- and Adam's first steps turn that into 1e-6 of a weight)
        logp = (-0.5 * z * z - ls - 0.5 * np.log(2.0 * np.pi)).sum(-1) - torch.log(1 - a ** 2 + 1e-6).sum(-1)
        return a, logp

    for g in range(steps):
        r = slice(g * n, (g + 1) * n)
        obs, nxt, act = batch["obs"][r].double(), batch["next_obs"][r].double(), batch["action"][r].double()
        rew, nd = batch["reward"][r].double(), (batch["done"][r] == 0).double()
        z_t = torch.from_numpy(adapters.sac_target_noise((g + 1) * n, S, su.SEED, su.DRAW)[g * n:])
        z_a = torch.from_numpy(adapters.sac_actor_noise(n, S, su.SEED, su.DRAW, g * n))
        alpha = torch.exp(lec.detach())
        with torch.no_grad():
            a_t, lp_t = act_of(nxt, z_t)
            xa = torch.cat([nxt, a_t.float().double()], dim=1)
            y = (rew + nd * su.GAMMA * (torch.minimum(q1t(xa), q2t(xa))[:, 0] - alpha * lp_t)).float().double()
        x = torch.cat([obs, act], dim=1)
        loss_q = 0.5 * (torch.nn.functional.mse_loss(q1(x)[:, 0], y) + torch.nn.functional.mse_loss(q2(x)[:, 0], y))
        opt_q.zero_grad()
        loss_q.backward()
        opt_q.step()
        a, lp = act_of(obs, z_a)
        xa = torch.cat([obs, a + (a.float().double() - a).detach()], dim=1)
        loss_pi = (alpha * lp - torch.minimum(q1(xa), q2(xa))[:, 0]).mean()
        opt_pi.zero_grad()
        loss_pi.backward()
        opt_pi.step()
        loss_a = -(lec * (lp.detach() + (-float(S)))).mean()
        opt_a.zero_grad()
        loss_a.backward()
        opt_a.step()
        with torch.no_grad():
            for tg, q in ((q1t, q1), (q2t, q2)):
                for pt, p in zip(tg.parameters(), q.parameters()):
                    pt.mul_(1.0 - su.TAU).add_(su.TAU * p)
        want = [float(x.detach()) for x in (loss_q, loss_pi, loss_a, alpha, lp.mean())]
        assert np.allclose(t["stats"][g, :5], want, rtol=1e-9, atol=1e-9), (g, t["stats"][g], want)
    for name, mod in (("actor", actor), ("q1", q1), ("q2", q2), ("q1_target", q1t), ("q2_target", q2t)):
        for (w, b), lin in zip(t[name], [m for m in mod if isinstance(m, torch.nn.Linear)]):
            assert torch.allclose(w, lin.weight, rtol=1e-9, atol=1e-9) and torch.allclose(b, lin.bias, rtol=1e-9, atol=1e-9), name
    assert abs(float(t["log_ent_coef"]) - float(lec.detach())) <= 1e-9


# slip -> (the gradient tensors or state it must move, the cases it applies to)
GRAD_SLIPS = {"larger_critic": ("actor",), "clamped_gradient": ("actor",), "target_noise_for_actor": ("actor", "log_ent_coef"),
              "short_logp": ("actor", "log_ent_coef"), "action_columns_pad32": ("actor",)}


# (at S 16 the action columns start at 160 = pad32(160): that slip changes nothing there)
SLIP_CASES = [(c, s) for c in sorted(su.CASES) for s in sorted(GRAD_SLIPS)
              if not (s == "action_columns_pad32" and pu.pad32(10 * su.CASES[c][0]) == 10 * su.CASES[c][0])]


@pytest.mark.parametrize("case,slip", SLIP_CASES)
def test_planted_gradient_slips_leave_the_yardstick(case, slip):
    """Each slip, planted into the float64 twin, puts its worst gradient tensor at least 1000 x the yardstick away"""
    S = su.CASES[case][0]
    if slip == "short_logp" and S == 1:
        names = ("log_ent_coef",)        # (no position is left: the actor keeps only the critics' gradient, which this slip does not touch)
    else:
        names = GRAD_SLIPS[slip]
    c = shared(case)
    bad = su.twin(case, c["batch"], c["nets"], LEC, steps=1, minibatch=su.ROWS, lr=0.0, slip=slip)
    ratios = su.grad_ratios(bad["grad"], c["t64"]["grad"], c["t32"]["grad"], names)
    worst = max(r[0] for r in ratios.values())
    print(case, slip, f"worst ratio {worst:.3g}")
    assert worst >= 1000.0 * su.FACTOR, (case, slip, worst)


@pytest.mark.parametrize("case", sorted(su.CASES))
def test_stale_critics_and_late_coefficient_leave_the_yardstick(case):
    """The actor gradient of one step under the critics of the step's START (lr 1e-2), and under the coefficient taken AFTER its own
    update (lr 1e-1: the coefficient moves by a tenth), each at least 1000 x the yardstick from the twin's."""
    c = shared(case)
    for slip, lr in (("stale_critics", 1e-2), ("coef_after_update", 1e-1)):
        kw = dict(steps=1, minibatch=su.ROWS, lr=lr)
        t64, t32 = su.twin(case, c["batch"], c["nets"], LEC, **kw), su.twin(case, c["batch"], c["nets"], LEC, torch.float32, **kw)
        bad = su.twin(case, c["batch"], c["nets"], LEC, slip=slip, **kw)
        worst = max(r[0] for r in su.grad_ratios(bad["grad"], t64["grad"], t32["grad"], ("actor",)).values())
        print(case, slip, f"worst ratio {worst:.3g}")
        assert worst >= 1000.0 * su.FACTOR, (case, slip, worst)


@pytest.mark.parametrize("case", sorted(su.CASES))
def test_polyak_on_the_live_critics_is_seen(case):
    """The targets are bit for bit the numpy rule on the new critics: a polyak step written into the live critics leaves every target
    tensor where it was, thousands of float32 ulp from where the rule puts it."""
    from tests.gpu_common import _ordered
    c = shared(case)
    kw = dict(steps=1, minibatch=su.ROWS, lr=1e-2)
    good, bad = su.twin(case, c["batch"], c["nets"], LEC, **kw), su.twin(case, c["batch"], c["nets"], LEC, slip="polyak_live", **kw)
    for k, start in (("q1_target", c["nets"][3]), ("q2_target", c["nets"][4])):
        for (w, _), (bw, _), (w0, _) in zip(good[k], bad[k], start):
            assert torch.equal(bw.float(), w0)
            d = np.abs(_ordered(w.float().numpy()) - _ordered(bw.float().numpy()))
            moved = d > 0                  # (a dead ReLU unit's weights have no gradient: neither the critic nor its target moves there)
            assert moved.any() and np.median(d[moved]) >= 1000, (k, float(np.median(d[moved])))


def test_actor_noise_rule_on_one_row():
    """Row k of a call is the global row first_row + k; counter (i lo, i hi, draw lo, SAC_ACTOR_TAG + j), key seed; Box-Muller."""
    S, seed, draw, first = 6, (5 << 32) | 9, 4, (1 << 32) + 7
    z = adapters.sac_actor_noise(3, S, seed, draw, first)
    i, j = first + 2, 4
    o = adapters.philox4x32_10(i & 0xFFFFFFFF, i >> 32, draw, adapters.SAC_ACTOR_TAG + j, 9, 5)
    u1, u2 = (int(o[0]) + 1.0) * 2.0 ** -32, int(o[1]) * 2.0 ** -32
    assert z[2, j] == np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)
    assert adapters.SAC_ACTOR_TAG == _lib.SAC_ACTOR_TAG and not (adapters.SAC_TAG <= adapters.SAC_ACTOR_TAG < adapters.SAC_TAG + 16)
    assert np.array_equal(adapters.sac_actor_noise(5, S, seed, draw, 0)[2:], adapters.sac_actor_noise(3, S, seed, draw, 2))
    assert not np.array_equal(adapters.sac_actor_noise(3, S, seed, draw, 0), adapters.sac_target_noise(3, S, seed, draw))


def test_state_dict_round_trip():
    actor, q1, q2 = su.case_layers("base")
    q1t, q2t = su.case_layers("base", seed=77)[1:]
    sd = adapters.sb3_sac_state_dict(actor, q1, q2, q1t, q2t, log_ent_coef=torch.tensor([LEC]))
    for (w, b), (w2, b2) in zip(actor, adapters.sb3_sac_actor_layers(sd)):
        assert torch.equal(w, w2) and torch.equal(b, b2)
    for prefix, want in (("critic", (q1, q2)), ("critic_target", (q1t, q2t))):
        for net, got in zip(want, adapters.sb3_sac_critic_layers(sd, prefix)):
            assert all(torch.equal(w, w2) and torch.equal(b, b2) for (w, b), (w2, b2) in zip(net, got))
    assert sd["actor.mu.weight"].shape == (5, 24) and sd["critic.qf1.2.weight"].shape == (24, 40) and float(sd["log_ent_coef"]) == LEC


def test_lds_plan_by_shape():
    """5120 + 128 x the larger net's strides; SB3's [256, 256] fits at every S <= 16; beyond the plan the figure says so"""
    from intent_radio_sched_multi_slice_amd.batched_env import sac_lds_bytes
    need = lambda dims: 128 * sum(pu.net_ld(pu.pad32(w)) for w in dims)  # noqa: E731
    for S in (1, 5, 10, 16):
        a, q = [10 * S, 256, 256, 2 * S], [11 * S, 256, 256, 1]
        assert sac_lds_bytes(a, q) == 5120 + max(need(a), need(q)) <= pu.LDS_MAX
    assert sac_lds_bytes([50, 24, 10], [55, 160, 7, 96, 1]) == 5120 + need([55, 160, 7, 96, 1])
    assert sac_lds_bytes([160, 512, 512, 32], [176, 512, 512, 1]) > pu.LDS_MAX


def test_header_binding_and_library_agree_on_the_new_exports():
    from intent_radio_sched_multi_slice_amd.csrc import build as hip_build
    with open(os.path.join(REPO, "include", "ranenv.h")) as f:
        hdr = f.read()
    assert re.search(r"#define\s+RANENV_ABI_VERSION\s+10\b", hdr) and _lib.ABI_VERSION == 10
    lib = ctypes.CDLL(hip_build.build())
    for name in NEW_EXPORTS:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name
        assert name in _lib.FUNCTIONS and hasattr(lib, name), name
    assert len(_lib.SAC_STATS) == int(re.search(r"#define\s+RANENV_SAC_STATS\s+(\d+)", hdr).group(1)) == 8
    assert re.search(r"0x53415000", hdr) and adapters.SAC_ACTOR_TAG == 0x53415000
    assert lib.ranenv_abi_version() == 10
    assert "ranenv_sac.hip" in hip_build.SOURCES and any(u[1] == "ranenv_sac.hip" for u in hip_build.UNITS)
