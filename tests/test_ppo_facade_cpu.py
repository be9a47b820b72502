"""The two handle-free helpers behind ``ppo_update`` / ``ppo_update_per_slice`` / ``ppo_update_head`` (batched_env.ppo_hparams,
batched_env.ppo_order_firsts) at their edges, without a GPU.  Every property is a check that takes the helper, so that the planted
slips at the end -- wrong helpers, each wrong in one way -- can be shown to fail the check that states the property."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from intent_radio_sched_multi_slice_amd import batched_env as be
from intent_radio_sched_multi_slice_amd._lib import RanEnvError

HP = dict(epochs=3, minibatch=16, lr=3e-4, clip=0.2, vf_coeff=0.5, ent_coeff=0.01, grad_clip=0.5, adv_norm="minibatch", betas=(0.9, 0.999), eps=1e-8)
FIELDS = ("lr", "clip", "vf_coeff", "ent_coeff", "grad_clip", "beta1", "beta2", "eps", "minibatch", "epochs", "adv_norm")


def _fields(hp):
    return [tuple(getattr(hp[m], f) for f in FIELDS) for m in range(len(hp))]


def _order(first, epochs, dtype=torch.int32):
    """An order dict of one kind, "inter": ``epochs`` rows of first[-1] record rows each."""
    return {"order_inter": torch.zeros((epochs, int(first[-1])), dtype=dtype), "first_inter": np.asarray(first)}


# ---- ppo_hparams ----------------------------------------------------------------------------------------------------------------
def check_scalar_is_the_sequence(hparams):
    G = 3
    one, e1, m1 = hparams(G, **HP)
    seq = {k: ([v] * G if k != "betas" else v) for k, v in HP.items()}
    many, e2, m2 = hparams(G, **seq)
    assert _fields(one) == _fields(many) and len(one) == G
    assert _fields(one)[0] == (3e-4, 0.2, 0.5, 0.01, 0.5, 0.9, 0.999, 1e-8, 16, 3, 1)
    assert e1.dtype == np.int64 and m1.dtype == np.int64 and e1.tolist() == e2.tolist() == [3] * G and m1.tolist() == m2.tolist() == [16] * G
    # ... and a sequence is per member: member 1's own values land in member 1's entry
    hp, e, _ = hparams(G, **{**HP, "lr": [1e-3, 2e-3, 3e-3], "epochs": [1, 4, 2], "adv_norm": ["minibatch", None, "none"]})
    assert [hp[m].lr for m in range(G)] == [1e-3, 2e-3, 3e-3] and e.tolist() == [1, 4, 2] and [hp[m].adv_norm for m in range(G)] == [1, 0, 0]


def check_wrong_length_names_the_member_count(hparams):
    with pytest.raises(ValueError, match=r"clip: 2 values given, one per member is 3"):
        hparams(3, **{**HP, "clip": [0.1, 0.2]})
    with pytest.raises(ValueError, match=r"epochs: 4 values given, one per member is 1"):
        hparams(1, **{**HP, "epochs": [1, 2, 3, 4]})
    with pytest.raises(ValueError, match="one for all or one per member"):
        hparams(3, **{**HP, "adv_norm": ["minibatch", None]})


def check_grad_clip_none_is_zero(hparams):
    assert hparams(2, **{**HP, "grad_clip": None})[0][1].grad_clip == 0.0
    assert hparams(1, **{**HP, "grad_clip": 0.25})[0][0].grad_clip == 0.25


def check_adv_norm_words(hparams):
    assert [hparams(1, **{**HP, "adv_norm": w})[0][0].adv_norm for w in ("minibatch", "none", None)] == [1, 0, 0]
    for bad in ("batch", "Minibatch", ""):
        with pytest.raises(ValueError, match='adv_norm is "minibatch" or None'):
            hparams(1, **{**HP, "adv_norm": bad})


# ---- ppo_order_firsts -----------------------------------------------------------------------------------------------------------
CAPS = (96, 12)         # small caps: rows x epochs, optimiser steps


def check_row_epochs_cap_edge(firsts):
    # 32 rows x 3 epochs == 96 passes (minibatch 32: 3 steps), one row more is refused with the method's name and the kind
    out = firsts(_order([0, 32], 3), {"inter": 1}, 3, 32, CAPS, "ppo_update")
    assert out["inter"].dtype == np.int32 and out["inter"].tolist() == [0, 32]
    with pytest.raises(RanEnvError, match=r"ppo_update: a member has more than 96 rows x epochs \(inter\)"):
        firsts(_order([0, 33], 3), {"inter": 1}, 3, 33, CAPS, "ppo_update")
    # per member: member 1's own rows x its own epochs decide (20 x 5 = 100 > 96), not the largest of each (40 x 5)
    firsts(_order([0, 40, 59], 5), {"inter": 2}, [2, 5], 64, CAPS)
    with pytest.raises(RanEnvError, match="rows x epochs"):
        firsts(_order([0, 40, 60], 5), {"inter": 2}, [2, 5], 64, CAPS)
    with pytest.raises(RanEnvError, match=r"ppo_update_per_slice: a policy has more than 96 rows x epochs \(inter\)"):
        firsts(_order([0, 33], 3), {"inter": 1}, 3, 33, CAPS, "ppo_update_per_slice", per_slice=True)


def check_steps_use_the_ceiling(firsts):
    # rows = minibatch + 1 is 2 steps per epoch: 6 epochs are exactly the cap of 12, 7 epochs 14
    firsts(_order([0, 9], 6), {"inter": 1}, 6, 8, CAPS)
    with pytest.raises(RanEnvError, match=r"a member has more than 12 optimiser steps \(inter: 14\)"):
        firsts(_order([0, 9], 7), {"inter": 1}, 7, 8, CAPS)
    firsts(_order([0, 8], 12), {"inter": 1}, 12, 8, CAPS)          # rows = minibatch: 1 step per epoch


def check_shape_refusals(firsts):
    with pytest.raises(ValueError, match=r"order_inter: int32 \[>= 2 epochs, first_inter\[-1\]\] with first_inter of 3 entries$"):
        firsts(_order([0, 8], 2), {"inter": 2}, 2, 8, CAPS)                              # a first of the wrong size
    o = _order([0, 8], 2)
    o["order_inter"] = torch.zeros((8, 2), dtype=torch.int32).t()                        # [2, 8], not contiguous
    with pytest.raises(ValueError, match="order_inter: int32"):
        firsts(o, {"inter": 1}, 2, 8, CAPS)
    with pytest.raises(ValueError, match="order_inter: int32"):
        firsts(_order([0, 8], 2, dtype=torch.int64), {"inter": 1}, 2, 8, CAPS)           # an int64 order
    with pytest.raises(ValueError, match="order_inter: int32"):
        firsts(_order([0, 8], 1), {"inter": 1}, 2, 8, CAPS)                              # fewer rows than epochs
    with pytest.raises(ValueError, match="order needs order_inter / first_inter"):
        firsts({}, {"inter": 1}, 2, 8, CAPS)
    # first[0] == 0 is the per-slice method's check alone, as before the fold (the library refuses the member lists')
    one = {"order_inter": torch.zeros((2, 8), dtype=torch.int32), "first_inter": np.array([1, 8])}
    firsts(one, {"inter": 1}, 2, 8, CAPS)
    with pytest.raises(ValueError, match=r"with first_inter of 2 entries from 0$"):
        firsts(one, {"inter": 1}, 2, 8, CAPS, "ppo_update_per_slice", per_slice=True)
    both = {**_order([0, 8], 2), "order_intra": torch.zeros((2, 6), dtype=torch.int32), "first_intra": np.array([0, 2, 6])}
    assert sorted(firsts(both, {"inter": 1, "intra": 2}, 2, 8, CAPS, per_slice=True)) == ["inter", "intra"]
    with pytest.raises(ValueError, match=r"order_intra: .* of 4 entries from 0 \(adapters.ppo_row_order\(..., per_slice=True\)\)$"):
        firsts(both, {"inter": 1, "intra": 3}, 2, 8, CAPS, per_slice=True)


def check_force_lifts_the_caps_alone(firsts):
    assert firsts(_order([0, 33], 3), {"inter": 1}, 3, 33, CAPS, force=True)["inter"].tolist() == [0, 33]
    firsts(_order([0, 9], 7), {"inter": 1}, 7, 8, CAPS, force=True)
    with pytest.raises(ValueError, match="order_inter: int32"):
        firsts(_order([0, 8], 2, dtype=torch.int64), {"inter": 1}, 2, 8, CAPS, force=True)
    with pytest.raises(ValueError, match="order_inter: int32"):
        firsts(_order([0, 8], 2), {"inter": 2}, 2, 8, CAPS, force=True)
    with pytest.raises(ValueError, match="order needs order_inter"):
        firsts({}, {"inter": 1}, 2, 8, CAPS, force=True)


HPARAM_CHECKS = (check_scalar_is_the_sequence, check_wrong_length_names_the_member_count, check_grad_clip_none_is_zero, check_adv_norm_words)
ORDER_CHECKS = (check_row_epochs_cap_edge, check_steps_use_the_ceiling, check_shape_refusals, check_force_lifts_the_caps_alone)


@pytest.mark.parametrize("check", HPARAM_CHECKS, ids=lambda c: c.__name__)
def test_ppo_hparams(check):
    check(be.ppo_hparams)


@pytest.mark.parametrize("check", ORDER_CHECKS, ids=lambda c: c.__name__)
def test_ppo_order_firsts(check):
    check(be.ppo_order_firsts)


def test_the_default_caps_are_the_class_attributes():
    assert (be.BatchedRanEnv.PPO_ROW_EPOCHS_CAP, be.BatchedRanEnv.PPO_STEPS_CAP) == (be.PPO_ROW_EPOCHS_CAP, be.PPO_STEPS_CAP) == (1 << 20, 1 << 13)
    with pytest.raises(RanEnvError, match=f"more than {1 << 13} optimiser steps"):
        be.ppo_order_firsts(_order([0, (1 << 13) + 1], 1), {"inter": 1}, 1, 1)


# ---- planted slips: a helper wrong in one way fails the check that states the property -------------------------------------------
def _hparams_slip(slip):
    def wrong(G, epochs, minibatch, lr, clip, vf_coeff, ent_coeff, grad_clip, adv_norm, betas, eps):
        kw = dict(epochs=epochs, minibatch=minibatch, lr=lr, clip=clip, vf_coeff=vf_coeff, ent_coeff=ent_coeff, grad_clip=grad_clip,
                  adv_norm=adv_norm, betas=betas, eps=eps)
        if slip == "first_value_for_all":           # a sequence is taken for its first value
            kw = {k: (v[0] if k != "betas" and np.ndim(v) > 0 else v) for k, v in kw.items()}
        if slip == "short_sequence_padded":         # a sequence of the wrong length is filled up with its last value
            kw = {k: (list(v) + [v[-1]] * G)[:G] if k != "betas" and np.ndim(v) > 0 else v for k, v in kw.items()}
        if slip == "no_clip_is_the_default" and grad_clip is None:
            kw["grad_clip"] = 0.5
        if slip == "none_word_normalises" and adv_norm == "none":
            kw["adv_norm"] = "minibatch"
        if slip == "any_word_is_none" and isinstance(adv_norm, str) and adv_norm != "minibatch":
            kw["adv_norm"] = None
        return be.ppo_hparams(G, **kw)
    return wrong


def _order_slip(slip):
    def wrong(order, units, epochs, minibatch, caps=(be.PPO_ROW_EPOCHS_CAP, be.PPO_STEPS_CAP), method="ppo_update", per_slice=False, force=False):
        if slip == "cap_is_exclusive":              # rows x epochs == cap refused
            caps = (caps[0] - 1, caps[1])
        if slip == "largest_of_each":               # the largest member's rows x the largest epochs
            epochs = int(np.max(epochs))
        if slip == "steps_floor":                   # floor(rows / minibatch): the last, short minibatch is not counted
            first = np.asarray(order.get("first_inter", [0, 0]))
            if not force and first.size >= 2 and int((np.diff(first) // np.maximum(minibatch, 1) * epochs).max()) <= caps[1]:
                caps = (caps[0], 1 << 30)
        if slip == "force_lifts_everything" and force:
            return {k[6:]: np.asarray(v, dtype=np.int32) for k, v in order.items() if k.startswith("first_")}
        if slip == "dtype_unchecked":
            order = {k: (v.to(torch.int32) if k.startswith("order_") else v) for k, v in order.items()}
        if slip == "contiguity_unchecked":
            order = {k: (v.contiguous() if k.startswith("order_") else v) for k, v in order.items()}
        if slip == "first_size_unchecked":
            units = {k[6:]: np.asarray(v).size - 1 for k, v in order.items() if k.startswith("first_")}
        if slip == "from_zero_everywhere":
            per_slice = True
        return be.ppo_order_firsts(order, units, epochs, minibatch, caps, method, per_slice, force)
    return wrong


@pytest.mark.parametrize("slip, check", [
    ("first_value_for_all", check_scalar_is_the_sequence), ("short_sequence_padded", check_wrong_length_names_the_member_count),
    ("no_clip_is_the_default", check_grad_clip_none_is_zero), ("none_word_normalises", check_adv_norm_words), ("any_word_is_none", check_adv_norm_words)])
def test_a_planted_slip_in_the_hparams_fails_its_check(slip, check):
    with pytest.raises(BaseException) as e:
        check(_hparams_slip(slip))
    assert e.type is AssertionError or e.type.__name__ == "Failed", (slip, e.type)      # (Failed: pytest.raises saw no exception)


@pytest.mark.parametrize("slip, check", [
    ("cap_is_exclusive", check_row_epochs_cap_edge), ("largest_of_each", check_row_epochs_cap_edge), ("steps_floor", check_steps_use_the_ceiling),
    ("force_lifts_everything", check_force_lifts_the_caps_alone), ("dtype_unchecked", check_shape_refusals),
    ("contiguity_unchecked", check_shape_refusals), ("first_size_unchecked", check_shape_refusals), ("from_zero_everywhere", check_shape_refusals)])
def test_a_planted_slip_in_the_order_check_fails_its_check(slip, check):
    with pytest.raises(BaseException) as e:
        check(_order_slip(slip))
    assert e.type is AssertionError or e.type.__name__ == "Failed" or e.type in (ValueError, RanEnvError), (slip, e.type)
