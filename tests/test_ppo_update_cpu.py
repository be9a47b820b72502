"""The float64 twin of the PPO update (adapters.ppo_update_reference and its parts) on the CPU: its loss against the example's
``ppo_loss``, its clip + Adam against ``torch.optim.Adam`` + ``clip_grad_norm_``, ``ppo_row_order``'s permutations, the packed
gradient layout, and planted slips: each moves the compared quantity beyond the tolerance tests/test_gpu_ppo_update.py uses on the
GPU (gradient: 8x the float32 yardstick, at least 8e-6 relative; Adam: 4 float32 ulp), so those tolerances bite."""
from __future__ import annotations

import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from intent_radio_sched_multi_slice_amd import adapters as ad
from tests import ppo_update_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = "tanh40x24"
HP = dict(clip=0.2, vf_coeff=0.5, ent_coeff=0.01, adv_norm=True)


@pytest.fixture(scope="module")
def setup():
    """A synthetic record whose logp column IS the nets' log-probability plus a perturbation (ratios around 1, some clipped), the
    members' nets, the row lists and member 1's float64 / float32 reference gradients of one minibatch of all rows, computed once."""
    rec = ref.synthetic_record(seed=11)
    nets = ref.member_nets(CASE, 3)
    order = ad.ppo_row_order(rec, ref.FIRST, 2, seed=4)
    g = torch.Generator().manual_seed(5)
    for kind, a in (("inter", "inter"), ("intra", "intra")):
        rows = torch.arange(rec["mask_inter"].numel() // (ref.S if kind == "inter" else 1))
        for m in range(3):
            batch = ad.ppo_rows(rec, kind, rows, ref.CASES[CASE][2])
            with torch.no_grad():
                _, st = ad.ppo_loss_reference([(w.double(), b.double()) for w, b in ref.layers_of(nets[a][m])], None, batch, kind, 0.2, 0.5, 0.01, False)
            lp = (st["logp"] + 0.25 * torch.randn(st["logp"].shape, generator=g, dtype=torch.float64)).to(torch.float32)
            view = rec["logp"].reshape(-1, ref.S + 1)
            envs = (rows // (1 if kind == "inter" else ref.S)) % 12
            mine = (envs >= ref.FIRST[m]) & (envs < ref.FIRST[m + 1])
            if kind == "inter":
                view[rows[mine], 0] = lp[mine]
            else:
                view[rows[mine] // ref.S, 1 + rows[mine] % ref.S] = lp[mine]
    out = {"rec": rec, "nets": nets, "order": order}
    for kind in ("inter", "intra"):
        out[kind] = {d: _reference(out, kind, dtype=d) for d in (torch.float64, torch.float32)}
    return out


def _reference(setup, kind, m=1, dtype=torch.float64, slip=None, **kw):
    a, c = ("inter", "v_inter") if kind == "inter" else ("intra", "v_intra")
    f = setup["order"]["first_" + kind]
    args = dict(epochs=1, minibatch=1 << 20, lr=0.0, grad_clip=0.0, act_actor="tanh", act_critic="tanh", layout=ref.CASES[CASE][2], **HP)
    args.update(kw)
    return ad.ppo_update_reference(setup["rec"], kind, ref.layers_of(setup["nets"][a][m]), ref.layers_of(setup["nets"][c][m]), setup["order"]["order_" + kind],
                                   int(f[m]), int(f[m + 1]), dtype=dtype, slip=slip, **args)


def _worst_ratio(setup, kind, other, m=1):
    """max over the layer tensors of ||g_other - g64|| / ||g64|| over max(||g32 - g64|| / ||g64||, 1e-6): what the GPU test bounds by 8"""
    worst = 0.0
    refs = setup[kind] if m == 1 else {d: _reference(setup, kind, m=m, dtype=d) for d in (torch.float64, torch.float32)}
    for net in ("actor", "critic"):
        for g64, g32, go in zip(refs[torch.float64]["grad"][net], refs[torch.float32]["grad"][net], other["grad"][net]):
            for x64, x32, xo in zip(g64, g32, go):
                n = float(x64.norm())
                worst = max(worst, float((xo.double() - x64).norm()) / n / max(float((x32.double() - x64).norm()) / n, 1e-6))
    return worst


def test_the_twins_loss_is_the_examples_ppo_loss():
    spec = importlib.util.spec_from_file_location("train_ppo_on_device", os.path.join(REPO, "examples", "train_ppo_on_device.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    g = torch.Generator().manual_seed(2)
    for kind in ("inter", "intra"):
        rec = ref.synthetic_record(seed=21)
        nets = ref.member_nets(CASE, 1)
        a, c = ("inter", "v_inter") if kind == "inter" else ("intra", "v_intra")
        rows = torch.randperm(60, generator=g)[:37]
        batch = ad.ppo_rows(rec, kind, rows, ref.CASES[CASE][2])
        actor = [(w.double(), b.double()) for w, b in ref.layers_of(nets[a][0])]
        critic = [(w.double(), b.double()) for w, b in ref.layers_of(nets[c][0])]
        _, st0 = ad.ppo_loss_reference(actor, critic, batch, kind, ex.CLIP, ex.VF_COEFF, ex.ENT_COEFF, True)
        batch["logp"] = st0["logp"].detach() + 0.3 * torch.randn(37, generator=g, dtype=torch.float64)      # ratios on both sides of the clip
        loss, st = ad.ppo_loss_reference(actor, critic, batch, kind, ex.CLIP, ex.VF_COEFF, ex.ENT_COEFF, True)
        x = batch["x"]
        for i, (w, b) in enumerate(critic):
            x = x @ w.T + b
            x = torch.tanh(x) if i < len(critic) - 1 else x
        ent = st["entropy"] * torch.ones(37, dtype=torch.float64)      # (the example takes per-row entropies; their mean is the twin's)
        want = ex.ppo_loss(st["logp"], batch["logp"], ent, x[:, 0], batch["adv"], batch["vtarg"])
        assert 0.0 < float(st["clip_frac"]) < 1.0
        assert abs(float(loss) - float(want)) <= 1e-12 * max(1.0, abs(float(want))), (kind, float(loss), float(want))


def test_the_twins_inter_log_probability_is_the_masked_gaussians():
    """... as adapters.masked_gaussian_params + torch.distributions.Normal give it in float64 (masked positions: Normal(-1, 1e-9) at
    exactly -1), to 1e-9: a masked term evaluated in float32 (an integer count times a Python float promotes to the default dtype)
    would be 2.9e-7 off per masked position."""
    rec = ref.synthetic_record(seed=3)
    nets = ref.member_nets(CASE, 1)
    batch = ad.ppo_rows(rec, "inter", torch.arange(40), "obs")
    actor = [(w.double(), b.double()) for w, b in ref.layers_of(nets["inter"][0])]
    _, st = ad.ppo_loss_reference(actor, None, batch, "inter", 0.2, 0.5, 0.0, False)
    x = batch["x"]
    for i, (w, b) in enumerate(actor):
        x = x @ w.T + b
        x = torch.tanh(x) if i < len(actor) - 1 else x
    mean, std = ad.masked_gaussian_params(x[:, :ref.S], x[:, ref.S:], batch["active"].to(torch.float64))
    want = torch.distributions.Normal(mean, std).log_prob(batch["action"]).sum(dim=1)
    assert st["logp"].dtype == torch.float64 and torch.allclose(st["logp"], want, rtol=1e-12, atol=1e-9), float((st["logp"] - want).abs().max())
    assert not bool(batch["active"].all()) and bool((batch["action"][~batch["active"]] == -1.0).all())


def test_the_twins_clip_and_adam_are_torchs_over_five_steps():
    g = torch.Generator().manual_seed(9)
    params = [torch.randn(s, generator=g, dtype=torch.float64) for s in ((7, 5), (7,), (3, 7), (3,))]
    mine = [p.clone() for p in params]
    theirs = [p.clone().requires_grad_(True) for p in params]
    opt = torch.optim.Adam(theirs, lr=3e-3, betas=(0.9, 0.999), eps=1e-8)
    state = {}
    for step in range(5):
        grads = [torch.randn(p.shape, generator=g, dtype=torch.float64) * (3.0 if step % 2 else 0.01) for p in params]
        for p, gr in zip(theirs, grads):
            p.grad = gr.clone()
        norm_t = torch.nn.utils.clip_grad_norm_(theirs, 0.5)
        opt.step()
        norm = ad.ppo_adam_reference(mine, [gr.clone() for gr in grads], state, 3e-3, 0.5)
        assert abs(norm - float(norm_t)) <= 1e-12 * norm
        for a, b in zip(mine, theirs):
            assert torch.allclose(a, b.detach(), rtol=1e-12, atol=1e-14), step
    assert state["t"] == 5


def test_row_order_gives_every_member_a_permutation_of_its_live_rows():
    rng = np.random.default_rng(0)
    for draw in range(200):
        B, T, S = int(rng.integers(2, 14)), int(rng.integers(1, 6)), int(rng.integers(1, 6))
        G = int(rng.integers(1, min(B, 5) + 1))
        first = np.concatenate([[0], np.sort(rng.choice(np.arange(1, B), G - 1, replace=False)), [B]]).astype(np.int64)
        mask = torch.as_tensor(rng.integers(0, 2, (T, B, S)).astype(np.int8))
        E = int(rng.integers(1, 4))
        o = ad.ppo_row_order({"mask_inter": mask}, first, E, seed=draw)
        for kind, rows_of in (("inter", lambda m: [t * B + b for t in range(T) for b in range(first[m], first[m + 1])]),
                              ("intra", lambda m: [(t * B + b) * S + s for t in range(T) for b in range(first[m], first[m + 1]) for s in range(S)
                                                   if mask[t, b, s] != 0])):
            order, f = o["order_" + kind].numpy(), o["first_" + kind]
            assert order.dtype == np.int32 and order.shape == (E, f[-1]) and f[0] == 0 and len(f) == G + 1
            for m in range(G):
                want = sorted(rows_of(m))
                for e in range(E):
                    assert sorted(order[e, f[m]:f[m + 1]].tolist()) == want, (draw, kind, m, e)
    o1, o2 = ad.ppo_row_order({"mask_inter": mask}, first, 3, seed=7), ad.ppo_row_order({"mask_inter": mask}, first, 3, seed=7)
    assert torch.equal(o1["order_inter"], o2["order_inter"]) and torch.equal(o1["order_intra"], o2["order_intra"])
    big = ad.ppo_row_order({"mask_inter": torch.ones((8, 12, 5), dtype=torch.int8)}, ref.FIRST, 2, seed=1)["order_inter"]
    assert not torch.equal(big[0], big[1]) and not torch.equal(big[0], torch.sort(big[0])[0])


def test_the_packed_gradient_layout_round_trips():
    nets = ref.member_nets("relu24", 1)
    actor, critic = [(w.numpy(), b.numpy()) for w, b in ref.layers_of(nets["intra"][0])], [(w.numpy(), b.numpy()) for w, b in ref.layers_of(nets["v_intra"][0])]
    flat = []
    for w, b in actor + critic:
        W = np.zeros((ref.pad32(w.shape[0]), ref.pad32(w.shape[1])), dtype=np.float32)
        W[:w.shape[0], :w.shape[1]] = w
        bb = np.zeros(ref.pad32(w.shape[0]), dtype=np.float32)
        bb[:b.shape[0]] = b
        flat += [W.reshape(-1), bb]
    flat = np.concatenate(flat + [np.zeros(5, dtype=np.float32)])
    got = ref.unpack_grad(flat, actor, critic, dtype=np.float32)
    for (w, b), (gw, gb) in zip(actor + critic, got["actor"] + got["critic"]):
        assert np.array_equal(w, gw) and np.array_equal(b, gb)
    flat[ref.pad32(actor[0][0].shape[1]) - 1] = 1.0
    with pytest.raises(AssertionError):
        ref.unpack_grad(flat, actor, critic)


def test_the_float32_yardstick_itself_is_far_inside_the_bound(setup):
    for kind in ("inter", "intra"):
        assert _worst_ratio(setup, kind, setup[kind][torch.float32]) <= 1.0 + 1e-9


@pytest.mark.parametrize("slip", ["unclipped", "entropy_sign", "mean_over_32", "masked_gradient", "no_activation_derivative"])
def test_a_planted_slip_in_the_gradient_leaves_the_gpu_tolerance(setup, slip):
    """Each slip moves some layer tensor's gradient beyond 8x the float32 yardstick (the GPU gradient test's bound)."""
    kinds = ("inter",) if slip == "masked_gradient" else ("inter", "intra")
    m = 2 if slip == "mean_over_32" else 1      # (member 1 has exactly 32 inter rows: the mean over 32 IS its mean)
    for kind in kinds:
        wrong = _reference(setup, kind, m=m, slip=slip)
        ratio = _worst_ratio(setup, kind, wrong, m)
        print(f"{slip} / {kind}: {ratio:.3g} x the yardstick")
        assert ratio > 8.0, (slip, kind, ratio)


def _shape_setup(shape, seed=31):
    """``setup`` for a SHAPES entry: a synthetic record of the entry's (S, Us) whose logp column is the members' nets' own
    log-probability plus a perturbation, the nets the GPU file binds (ref.shape_nets), and the row lists of the population ref.FIRST"""
    S, Us, layout, (aw, aa), (cw, ca) = ref.SHAPES[shape]
    rec = ref.synthetic_record(seed=seed, S=S, Us=Us)
    nets = ref.shape_nets(shape, 3)
    order = ad.ppo_row_order(rec, ref.FIRST, 1, seed=4)
    g = torch.Generator().manual_seed(5)
    view = rec["logp"].reshape(-1, S + 1)
    for kind in ("inter", "intra"):
        rows = torch.arange(rec["mask_inter"].numel() // (S if kind == "inter" else 1))
        envs = (rows // (1 if kind == "inter" else S)) % 12
        batch = ad.ppo_rows(rec, kind, rows, layout)
        for m in range(3):
            with torch.no_grad():
                _, st = ad.ppo_loss_reference([(w.double(), b.double()) for w, b in ref.layers_of(nets[kind][m])], None, batch, kind, 0.2, 0.5, 0.01, False, aa)
            lp = (st["logp"] + 0.25 * torch.randn(st["logp"].shape, generator=g, dtype=torch.float64)).to(torch.float32)
            mine = (envs >= ref.FIRST[m]) & (envs < ref.FIRST[m + 1])
            if kind == "inter":
                view[rows[mine], 0] = lp[mine]
            else:
                view[rows[mine] // S, 1 + rows[mine] % S] = lp[mine]
    return {"rec": rec, "nets": nets, "order": order, "acts": (aa, ca), "layout": layout}


def _shape_reference(su, kind, m, dtype=torch.float64, slip=None):
    a, c = ("inter", "v_inter") if kind == "inter" else ("intra", "v_intra")
    f = su["order"]["first_" + kind]
    return ad.ppo_update_reference(su["rec"], kind, ref.layers_of(su["nets"][a][m]), ref.layers_of(su["nets"][c][m]), su["order"]["order_" + kind],
                                   int(f[m]), int(f[m + 1]), epochs=1, minibatch=ref.ALL, lr=0.0, grad_clip=0.0, act_actor=su["acts"][0],
                                   act_critic=su["acts"][1], layout=su["layout"], dtype=dtype, slip=slip, **HP)


def _ratios(t64, t32, other):
    """{(net, layer, "W" / "b"): the device / yardstick ratio the GPU test bounds by 8, with ``other`` for the device}"""
    out = {}
    for net in ("actor", "critic"):
        for li, (g64, g32, go) in enumerate(zip(t64["grad"][net], t32["grad"][net], other["grad"][net])):
            for name, x64, x32, xo in zip("Wb", g64, g32, go):
                n = float(x64.norm())
                out[net, li, name] = float((xo.double() - x64).norm()) / n / max(float((x32.double() - x64).norm()) / n, 1e-6)
    return out


def test_the_lds_formula_at_the_edge_of_the_plan():
    """The header's formula (ref.lds_bytes) puts case A at 162 304 of 163 840 bytes for both kinds, [512, 512, 96] at S 5 beyond
    (170 496), and every other grid case inside."""
    S, Us, layout, (aw, _), (cw, _) = ref.SHAPES["A"]
    assert ref.lds_bytes(S, Us, layout, aw, cw) == 4096 + 128 * (68 + 516 + 516 + 68 + 68) == 162304 <= ref.LDS_MAX
    assert ref.lds_bytes(5, 5, "obs", [512, 512, 96], [512, 512, 96]) == 170496 > ref.LDS_MAX
    assert [ref.net_ld(x) for x in (32, 64, 96, 128, 160, 256, 480, 512)] == [68, 68, 132, 132, 196, 260, 516, 516]
    for S, Us, layout, (aw, _), (cw, _) in ref.SHAPES.values():
        assert ref.lds_bytes(S, Us, layout, aw, cw) <= ref.LDS_MAX


@pytest.mark.parametrize("shape", list(ref.SHAPES))
def test_the_twin_is_healthy_on_the_shape_grid(shape):
    """For every member of the GPU file's population and both kinds, with the nets it binds: every gradient tensor of the float64 twin
    has a non-zero norm (a dead ReLU stack would make the GPU comparison vacuous -- and its "the twin's gradient is zero" assertion
    fail), and the float32 yardstick is finite.  This guards ref.SHAPE_SEED: change the seed, not the shape."""
    su = _shape_setup(shape)
    for kind in ("inter", "intra"):
        for m in range(3):
            t64, t32 = _shape_reference(su, kind, m), _shape_reference(su, kind, m, torch.float32)
            for net in ("actor", "critic"):
                for li, (g64, g32) in enumerate(zip(t64["grad"][net], t32["grad"][net])):
                    for name, x64, x32 in zip("Wb", g64, g32):
                        assert float(x64.norm()) > 0.0, (shape, kind, m, net, li, name)
                        assert bool(torch.isfinite(x32).all()), (shape, kind, m, net, li, name)
            worst = max(_ratios(t64, t32, t32).values())
            assert np.isfinite(worst) and worst <= 1.0 + 1e-9
            assert np.isfinite(t64["stats"]).all() and np.isfinite(t32["stats"]).all()


def test_planted_slips_at_width_leave_the_gpu_tolerance():
    """On case E's intra nets ([255, 100] tanh actor over 33 inputs, [480] relu critic), member 2: a 16 x 16 block of the widest dW
    zeroed, row 32 missing from one layer's db, and the actor's activation derivative taken for the critic each move the tensor they hit
    beyond 8x the float32 yardstick."""
    su = _shape_setup("E")
    m, kind = 2, "intra"
    f = su["order"]["first_intra"]
    assert int(f[m + 1]) - int(f[m]) > 33
    t64, t32 = _shape_reference(su, kind, m), _shape_reference(su, kind, m, torch.float32)
    # (damage to the float32 twin's own gradient: block [16:32, 16:32] of the [100, 255] layer, the dW with the most blocks)
    damaged = {"grad": {net: [(w.clone(), b.clone()) for w, b in t32["grad"][net]] for net in ("actor", "critic")}}
    assert damaged["grad"]["actor"][1][0].shape == (100, 255)
    damaged["grad"]["actor"][1][0][16:32, 16:32] = 0.0
    r = _ratios(t64, t32, damaged)
    print(f"a zeroed 16 x 16 block of dW: {r['actor', 1, 'W']:.3g} x the yardstick")
    assert r["actor", 1, "W"] > 8.0
    assert all(v <= 1.0 + 1e-9 for k, v in r.items() if k != ("actor", 1, "W"))
    r = _ratios(t64, t32, _shape_reference(su, kind, m, slip="db_drops_row_32"))
    print(f"row 32 missing from db of layer 0: actor {r['actor', 0, 'b']:.3g}, critic {r['critic', 0, 'b']:.3g} x the yardstick")
    assert r["actor", 0, "b"] > 8.0 and r["critic", 0, "b"] > 8.0
    r = _ratios(t64, t32, _shape_reference(su, kind, m, slip="critic_takes_actor_derivative"))
    print(f"tanh's derivative on the relu critic: {r['critic', 0, 'W']:.3g} x the yardstick")
    assert r["critic", 0, "W"] > 8.0 and r["critic", 0, "b"] > 8.0
    assert all(v <= 1.0 + 1e-9 for k, v in r.items() if k[0] == "actor")


def test_adam_slips_leave_four_ulp(setup):
    """Adam without bias correction, and the neighbour member's lr, each move a weight of the first step by more than 4 float32 ulp
    from the numpy restatement the GPU test compares with."""
    from tests.gpu_common import _ordered
    nets = setup["nets"]
    w = [(a.numpy(), b.numpy()) for a, b in ref.layers_of(nets["inter"][1])]
    g = [(x.numpy().astype(np.float32), y.numpy().astype(np.float32)) for x, y in setup["inter"][torch.float64]["grad"]["actor"]]
    lrs = [3e-4, 1e-3, 5e-3]
    want, _ = ref.adam_step_f32(w, g, 1, lrs[1], 0.5)
    for what, layers in (("the neighbour's lr", ref.adam_step_f32(w, g, 1, lrs[2], 0.5)[0]),
                         ("no bias correction", _adam_no_bias_correction(w, g, lrs[1], 0.5))):
        worst = max(int(np.abs(_ordered(x) - _ordered(y)).max()) for a, b in zip(want, layers) for x, y in zip(a, b))
        print(f"{what}: {worst} ulp")
        assert worst > 4, what
    # ... and the float64 twin's own step agrees with the float32 restatement to float32 rounding
    r = _reference(setup, "inter", lr=lrs[1], grad_clip=0.5)
    full, _ = ref.adam_step_f32(w + [(a.numpy(), b.numpy()) for a, b in ref.layers_of(nets["v_inter"][1])],
                                g + [(x.numpy().astype(np.float32), y.numpy().astype(np.float32)) for x, y in setup["inter"][torch.float64]["grad"]["critic"]],
                                1, lrs[1], 0.5)
    for (a, b), (x, y) in zip(full, r["actor"] + r["critic"]):
        assert np.allclose(a, x.numpy(), rtol=0, atol=1e-6) and np.allclose(b, y.numpy(), rtol=0, atol=1e-6)


def _adam_no_bias_correction(w, g, lr, grad_clip):
    params = [torch.as_tensor(x).clone() for pair in w for x in pair]
    grads = [torch.as_tensor(x).clone() for pair in g for x in pair]
    ad.ppo_adam_reference(params, grads, {}, lr, grad_clip, slip="no_bias_correction")
    return [(params[2 * i].numpy(), params[2 * i + 1].numpy()) for i in range(len(w))]


def test_the_c_abi_declares_the_entries_and_the_binding_matches():
    from intent_radio_sched_multi_slice_amd import _lib
    import ctypes as C
    header = open(os.path.join(REPO, "include", "ranenv.h")).read()
    for name in ("ranenv_ppo_bind", "ranenv_ppo_update", "ranenv_ppo_layout", "ranenv_ppo_state", "ranenv_ppo_probe_logp", "ranenv_get_net_weights"):
        assert f"int {name}(" in header and name in _lib.FUNCTIONS
    assert C.sizeof(_lib.PpoHparams) == 80 and "#define RANENV_PPO_HPARAMS_BYTES 80" in header
    assert len(_lib.PPO_STATS) == 8 and "#define RANENV_PPO_STATS 8" in header
    lib = _lib.load()
    assert lib.ranenv_ppo_bind(None, None) == -1 and b"null handle" in lib.ranenv_last_error(None)
