"""The PPO update of the head policies, on the CPU: the six new entries of the C ABI and their binding, the float64 twin
(adapters.ppo_head_update_reference) against a plain torch module, the health of the twin on the cases tests/test_gpu_ppo_head.py runs
(no zero gradient tensor, clip fractions strictly inside (0.1, 0.9)), the SB3 state-dict round trip, the row order, and planted slips of
the kind the head kernel can make -- each leaves the bound the GPU file puts on its tensors by a factor above 1000."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import ppo_head_ref as hd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = {"ranenv_ppo_bind_head": 2, "ranenv_ppo_update_head": 10, "ranenv_ppo_head_layout": 4, "ranenv_ppo_head_state": 6,
               "ranenv_get_head_net_weights": 4, "ranenv_get_head_log_std": 3}
E_INVALID = -1


def test_the_c_abi_declares_the_new_entries_and_the_binding_matches():
    from intent_radio_sched_multi_slice_amd import _lib
    header = open(os.path.join(REPO, "include", "ranenv.h")).read()
    lib = _lib.load()
    for name, n_args in NEW_EXPORTS.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == n_args, name
        assert name in _lib.EXPORTS and len(_lib.FUNCTIONS[name][1]) == n_args and hasattr(lib, name), name
    assert "#define RANENV_ABI_VERSION 10" in header and _lib.ABI_VERSION == 10 and lib.ranenv_abi_version() == 10
    calls = (lambda: lib.ranenv_ppo_bind_head(None, None), lambda: lib.ranenv_ppo_update_head(None, 1, None, None, None, 0, 0, None, None, None),
             lambda: lib.ranenv_ppo_head_layout(None, None, None, None), lambda: lib.ranenv_ppo_head_state(None, 0, None, None, None, None),
             lambda: lib.ranenv_get_head_net_weights(None, 0, None, None), lambda: lib.ranenv_get_head_log_std(None, None, None))
    for call in calls:
        assert call() == E_INVALID and b"null" in lib.ranenv_last_error(None)


class _Policy(torch.nn.Module):
    """SB3's ActorCriticPolicy in its plainest form: two MLPs and a log_std parameter"""

    def __init__(self, case):
        super().__init__()
        from tests import ppo_update_ref as ref
        actor, log_std, critic = hd.layers(case)
        self.actor = ref.as_sequential(actor, hd.CASES[case][2]).double()
        self.critic = ref.as_sequential(critic, hd.CASES[case][4]).double()
        self.log_std = torch.nn.Parameter(log_std.double().clone())


@pytest.mark.parametrize("case", list(hd.CASES))
def test_the_twin_is_sb3s_train_loop_in_plain_torch(case):
    """Two epochs of minibatch 12: the twin's weights, log_std and statistics against a torch module trained with Normal, Adam(eps=1e-5)
    and clip_grad_norm_, within 1e-9; the twin's clip fraction lies strictly inside (0.1, 0.9) on every minibatch"""
    rec, order = hd.synthetic_record(case), hd.row_order(2)
    hp = dict(clip=0.2, vf_coeff=0.5, ent_coeff=0.01, lr=3e-4, grad_clip=0.5)
    t = hd.twin(case, rec, order, epochs=2, minibatch=hd.MINIBATCH, adv_norm=True, **hp)
    assert len(t["clip_fracs"]) == 16 and all(0.1 < f < 0.9 for f in t["clip_fracs"]), t["clip_fracs"]
    pol, S = _Policy(case), hd.CASES[case][0]
    opt = torch.optim.Adam(pol.parameters(), lr=hp["lr"], eps=1e-5)
    obs, act = rec["obs_head"].reshape(hd.N, 10 * S).double(), rec["action"].reshape(hd.N, S)
    lp_old, adv_all, vtarg = (rec[k].reshape(-1).double() for k in ("logp", "adv", "vtarg"))
    for ep in range(2):
        for c0 in range(0, hd.N, hd.MINIBATCH):
            rows = order[ep, c0:c0 + hd.MINIBATCH].long()
            dist = torch.distributions.Normal(pol.actor(obs[rows]), torch.exp(pol.log_std))
            lp, adv = dist.log_prob(act[rows]).sum(dim=1), adv_all[rows]
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
            ratio = torch.exp(lp - lp_old[rows])
            loss = (-torch.min(ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv).mean()
                    + hp["vf_coeff"] * torch.nn.functional.mse_loss(pol.critic(obs[rows])[:, 0], vtarg[rows]) - hp["ent_coeff"] * dist.entropy().sum(dim=1).mean())
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(pol.parameters(), hp["grad_clip"])
            opt.step()
    lin = lambda net: [m for m in net if isinstance(m, torch.nn.Linear)]  # noqa: E731
    for name, net in (("actor", pol.actor), ("critic", pol.critic)):
        for (w, b), m in zip(t[name], lin(net)):
            assert torch.allclose(w, m.weight.detach(), rtol=0, atol=1e-9) and torch.allclose(b, m.bias.detach(), rtol=0, atol=1e-9), name
    assert torch.allclose(t["log_std"], pol.log_std.detach(), rtol=0, atol=1e-9)
    assert not torch.equal(t["log_std"], hd.layers(case)[1].double())


@pytest.mark.parametrize("case", list(hd.CASES))
def test_no_gradient_tensor_of_the_twin_is_zero(case):
    rec = hd.synthetic_record(case)
    t = hd.twin(case, rec, hd.row_order(1), epochs=1, minibatch=hd.ALL, lr=0.0, grad_clip=0.0, **hd.HP)
    for k, x in hd.tensors(t["grad"]).items():
        assert np.linalg.norm(x) > 0.0 and np.all(np.isfinite(x)), f"{case}: {k}"
    assert 0.1 < t["clip_fracs"][0] < 0.9
    for nb in (1, 31, 32, 33, 65):       # the row tails of the GPU file, advantages as given
        t = hd.twin(case, rec, hd.row_order(1)[:, :nb].contiguous(), epochs=1, minibatch=hd.ALL, lr=0.0, grad_clip=0.0, **dict(hd.HP, adv_norm=False))
        assert all(np.linalg.norm(x) > 0.0 for x in hd.tensors(t["grad"]).values()), (case, nb)


def test_the_state_dict_round_trip_is_exact():
    from intent_radio_sched_multi_slice_amd.adapters import sb3_ppo_layers, sb3_ppo_state_dict
    for case in hd.CASES:
        actor, log_std, critic = hd.layers(case)
        sd = sb3_ppo_state_dict(actor, log_std, critic)
        assert "log_std" in sd and "action_net.weight" in sd and "value_net.bias" in sd and "mlp_extractor.policy_net.0.weight" in sd
        a2, ls2, c2 = sb3_ppo_layers(sd)
        assert torch.equal(ls2, log_std) and len(a2) == len(actor) and len(c2) == len(critic)
        for got, want in ((a2, actor), (c2, critic)):
            for (w, b), (w0, b0) in zip(got, want):
                assert torch.equal(w, w0) and torch.equal(b, b0)
        again = sb3_ppo_state_dict(a2, ls2, c2)
        assert again.keys() == sd.keys() and all(torch.equal(again[k], sd[k]) for k in sd)
    with pytest.raises(ValueError):
        sb3_ppo_state_dict(actor[:1], log_std, critic)


def test_the_row_order_is_a_permutation_per_epoch():
    from intent_radio_sched_multi_slice_amd.adapters import ppo_head_row_order
    rng = np.random.default_rng(11)
    for _ in range(200):
        T, B, epochs, seed = int(rng.integers(1, 9)), int(rng.integers(1, 14)), int(rng.integers(1, 5)), int(rng.integers(0, 2 ** 31))
        rec = {"logp": torch.zeros((T, B))}
        o = ppo_head_row_order(rec, epochs, seed)
        assert o.dtype == torch.int32 and tuple(o.shape) == (epochs, T * B) and o.is_contiguous()
        assert torch.equal(torch.sort(o, dim=1).values, torch.arange(T * B, dtype=torch.int32).expand(epochs, -1))
        assert torch.equal(o, ppo_head_row_order(rec, epochs, seed))
    big = ppo_head_row_order({"logp": torch.zeros((8, 12))}, 3, 1)
    assert not torch.equal(big[0], big[1]) and not torch.equal(big, ppo_head_row_order({"logp": torch.zeros((8, 12))}, 3, 2))


# Two minibatches of 48 rows with a step of 1e-2 between them, clipped hard (grad_clip 0.05: the joint norm is far above it), entropy
# bonus 0.01: the tensors compared are the second minibatch's gradient and the trained weights, log_std and Adam's m behind it.
SLIP_HP = dict(epochs=1, minibatch=48, lr=1e-2, clip=0.2, vf_coeff=0.5, ent_coeff=0.01, grad_clip=0.05, adv_norm=True)


def _slip_tensors(t):
    out = {"grad " + k: v for k, v in hd.tensors(t["grad"]).items()}
    out.update({"weight " + k: v for k, v in hd.tensors({"actor": t["actor"], "critic": t["critic"], "log_std": t["log_std"]}).items()})
    na, nc = 2 * len(t["actor"]), 2 * len(t["critic"])
    m = [x.numpy().astype(np.float64) for x in t["state"]["m"]]
    pairs = lambda flat: [(flat[2 * i], flat[2 * i + 1]) for i in range(len(flat) // 2)]  # noqa: E731
    out.update({"m " + k: v for k, v in hd.tensors({"actor": pairs(m[:na]), "critic": pairs(m[na:na + nc]), "log_std": m[-1]}).items()})
    return out


@pytest.mark.parametrize("case", list(hd.CASES))
def test_planted_slips_leave_the_bound_by_a_factor_above_1000(case):
    """Each slip of ppo_head_ref.SLIPS in the float32 restatement puts some tensor's ratio to the yardstick above 1000 (the GPU file
    allows 8), on every case -- S 1 included: with one position a logp over S - 1 positions is a constant 0, the masked term replaces the
    only term, and the stride S + 1 = 2 still reads another row's cell, so none of the slips hides there."""
    rec, order = hd.synthetic_record(case), hd.row_order(1)
    t64 = _slip_tensors(hd.twin(case, rec, order, **SLIP_HP))
    t32 = _slip_tensors(hd.twin(case, rec, order, dtype=torch.float32, **SLIP_HP))
    clean = hd.ratios(t32, t64, t32)
    assert max(v[0] for v in clean.values()) <= 1.0 + 1e-12
    for slip in hd.SLIPS:
        got = _slip_tensors(hd.twin(case, rec, order, dtype=torch.float32, slip=slip, **SLIP_HP))
        r = hd.ratios(got, t64, t32)
        k, worst = max(((k, v[0]) for k, v in r.items()), key=lambda kv: kv[1])
        print(f"{case} {slip}: worst ratio {worst:.3g} at {k}")
        assert worst > 1000.0, f"{case}: the slip {slip} stays within {worst:.3g} x the yardstick (worst tensor {k})"
