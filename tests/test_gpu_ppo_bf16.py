"""The bf16 spread binding of the PPO update on the device (ranenv_ppo_bind_spread_bfloat / ranenv_ppo_update; the kernels
ranenv_ppo_spread_pass_kernel_bf16 and ranenv_ppo_spread_apply_kernel_bf16; include/ranenv.h "bf16 nets over the chip"): exact nets bit
for bit; the recorded log-probability re-evaluated bit for bit; random nets against the float64 twin of the contract; one Adam step
and the re-rounded acting copy; determinism and the loop of steps; the boundary to the other bindings.

Every case: ONE agent on ref.native_workload(12), S 5 / Us 5, T 8 -- 96 inter rows and a few hundred live intra rows, every net bound
with precision="bf16".  The cap of the comparison with the twin is not a constant: per gradient tensor it is a quarter of e_bf, the
distance between the contract and f32 training of the same masters (both twins float64), computed here; the statistics take the same
rule with a floor of 1e-6.  tests/test_ppo_bf16_cpu.py shows that every planted slip of the contract moves a tensor beyond that cap."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import policy_bf16_ref as br
from tests import ppo_bf16_ref as bf
from tests import ppo_spread_ref as sp
from tests import ppo_update_ref as ref
from tests import ppo_wide_ref as wd
from tests.gpu_common import need_gpu

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -3
ALL, B = ref.ALL, 12
CASES = ["relu24", "tanh40x24", "verybig"]
FIRST = [0, B]
HP_LOOP = dict(lr=2e-3, clip=0.2, vf_coeff=0.5, ent_coeff=0.01, grad_clip=0.5)
STAT_NAMES = ("policy_loss", "value_loss", "entropy", "kl", "clip_frac")


def _nets(case):
    if case in ref.CASES:
        return sp.one_agent_nets(case), ref.CASES[case][1], ref.CASES[case][2]
    nets = wd.beyond_nets(case, n=1)
    return {r: nets[r][0] for r in ref.ROLES}, wd.BEYOND[case][1], wd.BEYOND[case][2]


def _bind_nets(env, nets, layout, stochastic=True, activation=None, precision="bf16"):
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=stochastic, seed=ref.SEED, intra_input=layout, activation=activation, precision=precision)
    env.set_value_network(nets["v_inter"], nets["v_intra"], activation=activation, precision=precision)


def _env(case, slabs=3, stochastic=True):
    """A reset env of the native shape under ONE agent of the case's nets, all bf16, under the bf16 spread binding"""
    need_gpu()
    env = ref.native_workload(B)
    nets, _, layout = _nets(case)
    _bind_nets(env, nets, layout, stochastic)
    env.ppo_bind(spread=True, slabs=slabs, bf16=True)
    env.reset()
    return env


def _order(rec, epochs, seed=3):
    from intent_radio_sched_multi_slice_amd.adapters import ppo_row_order
    return ppo_row_order(rec, FIRST, epochs, seed)


def _cut(order, n):
    """The first n entries of the first epoch's list of both kinds"""
    out = {}
    for kind in ("inter", "intra"):
        assert int(order["first_" + kind][1]) >= n
        out["order_" + kind], out["first_" + kind] = order["order_" + kind][:1, :n].contiguous(), np.array([0, n], dtype=np.int32)
    return out


def _with_outside(order, rec, n=64):
    """An n-entry list of both kinds with three entries outside the record: at its head, in its second tile and at its tail"""
    T, _, S = rec["mask_inter"].shape
    out = _cut(order, n)
    for kind, n_record in (("inter", T * B), ("intra", T * B * S)):
        o = out["order_" + kind].clone()
        o[0, 0], o[0, 32], o[0, n - 1] = -1, n_record, 2 ** 31 - 1
        out["order_" + kind] = o
    return out


def _live(lst, kind, n_record):
    rows = lst["order_" + kind][0].cpu().numpy().astype(np.int64)
    return rows[(rows >= 0) & (rows < n_record)], len(rows)


# ---- 1. exact nets --------------------------------------------------------------------------------------------------------------------
EXACT = [("a", arch) for arch in ("64x64", "40x72x40x72", "512x3")] + [("b", arch) for arch in bf.EXACT_B_ARCHS]


@pytest.mark.parametrize("family,arch", EXACT, ids=[f"{f}-{a}" for f, a in EXACT])
def test_exact_critics_bit_for_bit_under_every_split(family, arch):
    """The two families of tests/ppo_bf16_ref.py: integer-valued relu critics, the record's observations and masks overwritten in place
    with 0 / 1 and its targets with V - j 2^-9.  Every partial sum, forward and backward, is an exact float32 (asserted,
    exact_conditions), so every tile split and slab count must give the float64 gradient and value loss bit for bit: lists of 32 and
    64 entries and a 64-entry list with entries outside the record, slabs 1, 2, 3 and 32, both kinds.  Family (a): every rounding a
    no-op (j in -3..3).  Family (b): hidden and D values that the rounding DOES change, exactly decided (j in -48..48, sparse 0 / 1
    rows): there a D truncated or left unrounded, or a Wt swapped in k, flips a bit of some dW (asserted per list by
    exact_conditions), so this check tells round-to-nearest-even from its neighbours to the bit."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd.adapters import ppo_rows
    layout, S, Us = "mask_obs", ref.S, ref.US
    env = ref.native_workload(B)
    a_inter, a_intra, _, _ = br.exact_case_nets(arch, S, Us, layout, bf.EXACT_SEED + 50)
    make, jmax, density = (bf.exact_critic, 3, 0.5) if family == "a" else (bf.exact_critic_b, 48, bf.EXACT_B_DENSITY)
    critics = {"inter": make(10 * S, arch), "intra": make(ref.intra_width(Us, layout), arch, bf.EXACT_SEED + 3)}
    _bind_nets(env, {"inter": a_inter, "intra": a_intra, "v_inter": critics["inter"], "v_intra": critics["intra"]}, layout, activation="relu")
    env.ppo_bind(spread=True, slabs=1, bf16=True)
    env.reset()
    rec = env.collect(ref.T)
    T = ref.T
    rng = np.random.default_rng(bf.EXACT_SEED)
    dev = rec["obs_inter"].device
    bits = lambda x, dt: torch.as_tensor((rng.random(tuple(x.shape)) < density).astype(dt), device=dev)      # noqa: E731
    rec["obs_inter"][:T] = bits(rec["obs_inter"][:T], np.float32)
    rec["obs_intra"][:T] = bits(rec["obs_intra"][:T], np.float32)
    rec["mask_intra"][:T] = bits(rec["mask_intra"][:T], np.int8)
    host = {k: v.cpu() for k, v in rec.items()}
    vtarg = np.zeros((T, B, S + 1), dtype=np.float32)
    every = {"inter": np.arange(T * B), "intra": np.arange(T * B * S)}
    for kind in ("inter", "intra"):
        x = ppo_rows(host, kind, every[kind], layout)["x"].numpy()
        v = bf.contract_forward(x, critics[kind], "relu")[0][:, 0]
        t, _ = bf.exact_targets(v, rng, jmax)
        if kind == "inter":
            vtarg[:, :, 0] = t.reshape(T, B)
        else:
            vtarg[:, :, 1:] = t.reshape(T, B, S)
    rec["vtarg"][:T] = torch.as_tensor(vtarg, device=dev)
    host["vtarg"] = rec["vtarg"].cpu()
    order = _order(rec, 1)
    lists = [("32 entries", _cut(order, 32)), ("64 entries", _cut(order, 64)), ("64 entries, three outside the record", _with_outside(order, rec))]
    want = {}
    for what, lst in lists:
        for kind_i, kind in enumerate(("inter", "intra")):
            rows, n = _live(lst, kind, len(every[kind]))
            r = ppo_rows(host, kind, rows, layout)
            x, vt = r["x"].numpy(), r["vtarg"].numpy().astype(np.float32)
            bf.exact_conditions(x, critics[kind], vt, n, family)
            grads, vl, _ = bf.exact_critic_grad(x, critics[kind], vt, n)
            want[what, kind] = (bf.pack_grad(grads), vl)
            assert want[what, kind][0].any() and vl > 0.0
    for slabs in (1, 2, 3, 32):
        env.ppo_bind(spread=True, slabs=slabs, bf16=True)
        for what, lst in lists:
            out = env.ppo_update(rec, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, vf_coeff=bf.VF_COEFF, adv_norm=None, order=lst, grad=True)
            for kind_i, kind in enumerate(("inter", "intra")):
                lay = env.ppo_member_layout(0, kind)
                g, vl = want[what, kind]
                assert lay["critic"] == g.size
                got = out["grad"][0, kind_i, lay["actor"]:lay["actor"] + lay["critic"]].cpu().numpy()
                assert got.tobytes() == g.tobytes(), f"{arch}, {slabs} slabs, {what}, {kind}: {int((got != g).sum())} of {g.size} critic gradient floats differ"
                assert out["value_loss"][0, kind_i, 0] == vl, (arch, slabs, what, kind, out["value_loss"][0, kind_i, 0], vl)
    env.close()


# ---- 2. the log-probability -------------------------------------------------------------------------------------------------------------
def _logp_is_the_recorded_one(env, rec):
    order = _order(rec, 1)
    probe = env.ppo_update(rec, epochs=1, minibatch=40, lr=0.0, grad_clip=None, order=order, probe_logp=True)
    new, old, mask = probe["logp"].cpu().numpy(), rec["logp"].cpu().numpy(), rec["mask_inter"].cpu().numpy() != 0
    assert np.array_equal(new[..., 0].view(np.int32), old[..., 0].view(np.int32)), "inter: the re-evaluated logp is not the recorded one"
    assert np.array_equal(new[..., 1:][mask].view(np.int32), old[..., 1:][mask].view(np.int32)), "intra: the re-evaluated logp is not the recorded one"
    # (kl is the float64 log-probability against its float32 record: their rounding distance, not 0)
    assert mask.sum() > 130 and np.all(probe["clip_frac"][:, :, 0] == 0.0) and np.all(np.abs(probe["kl"][:, :, 0]) < 1e-6)


@pytest.mark.parametrize("case", ["relu24", "tanh40x24"])
def test_the_reevaluated_logp_is_the_recorded_one_bit_for_bit(case):
    """The forward pass of the update is the acting kernels' on the acting copy: right after collect(), and again after a real update
    (which re-rounds the acting copy) followed by a new collect()"""
    env = _env(case, stochastic=True)
    rec = env.collect(ref.T)
    _logp_is_the_recorded_one(env, rec)
    before = ref.state(env, 1)
    env.ppo_update(rec, epochs=2, minibatch=40, order=_order(rec, 2), **HP_LOOP)
    after = ref.state(env, 1)
    assert all(after[k].tobytes() != before[k].tobytes() for k in after if k.split("/")[-1][0] == "w"), "a weight matrix did not move"
    _logp_is_the_recorded_one(env, env.collect(ref.T))
    env.close()


# ---- 3. random nets against the twin ----------------------------------------------------------------------------------------------------
def _twins(rec_host, lst, masters, act, layout, cache, key):
    """Per kind the float64 bf16 twin and the float64 f32 twin of a one-minibatch call on the list's live rows, and the factor
    live entries / entries on their gradients and statistics (a row's weight is 1 / entries)"""
    if key in cache:
        return cache[key]
    out = {}
    T, _, S = rec_host["mask_inter"].shape
    for kind, n_record in (("inter", T * B), ("intra", T * B * S)):
        rows, n = _live(lst, kind, n_record)
        o = torch.as_tensor(rows[None, :])
        a, c = ("inter", "v_inter") if kind == "inter" else ("intra", "v_intra")
        t16 = bf.twin_grads(rec_host, kind, masters[a][0], masters[c][0], o, 0, len(rows), act, layout, "bf16")
        t32 = bf.twin_grads(rec_host, kind, masters[a][0], masters[c][0], o, 0, len(rows), act, layout, "f32")
        out[kind] = (t16, t32, len(rows) / n)
    cache[key] = out
    return out


def _check_against_the_contract(out, twins, masters, what):
    """dev_grad per tensor within a quarter of e_bf of the bf16 twin, the statistics within a quarter of the twins' distance (floor
    1e-6); returns the worst ratio error / e_bf"""
    worst = 0.0
    for kind_i, kind in enumerate(("inter", "intra")):
        t16, t32, f = twins[kind]
        a, c = ("inter", "v_inter") if kind == "inter" else ("intra", "v_intra")
        dev = ref.unpack_grad(out["grad"][0, kind_i].cpu().numpy(), masters[a][0], masters[c][0])
        g16, g32 = bf.grad_tensors(t16), bf.grad_tensors(t32)
        for (net, li, name), x16 in g16.items():
            xd = dev[net][li]["Wb".index(name)]
            if not np.linalg.norm(x16) > 0.0:
                assert not xd.any(), f"{what}: {kind} {net} layer {li} {name}: the twin's gradient is zero, the device's is not"
                continue
            e_bf, e_dev = bf.rel_l2(g32[net, li, name], x16), bf.rel_l2(xd, f * x16)
            assert e_bf > 0.0, f"{what}: {kind} {net} layer {li} {name}: bf16 and f32 training agree, the cap is empty"
            if e_dev > 0.01 * e_bf:          # (what comes near the cap is named: a short list's tiny e_bf, or flipped roundings?)
                print(f"{what}: {kind} {net} layer {li} {name}: device error {e_dev:.3g} = {e_dev / e_bf:.3g} of e_bf {e_bf:.3g}")
            worst = max(worst, e_dev / e_bf)
            assert e_dev <= 0.25 * e_bf, f"{what}: {kind} {net} layer {li} {name}: device error {e_dev:.3g}, e_bf {e_bf:.3g} (ratio {e_dev / e_bf:.3g})"
        for i, name in enumerate(STAT_NAMES):
            got, want, other = out[name][0, kind_i, 0], f * t16["stats"][0, i], f * t32["stats"][0, i]
            assert abs(got - want) <= max(0.25 * abs(want - other), 1e-6 * max(1.0, abs(want))), f"{what}: {kind} {name}: device {got:.9g}, twin {want:.9g}, f32 twin {other:.9g}"
    return worst


@pytest.mark.parametrize("case", CASES)
def test_random_nets_against_the_float64_twin_of_the_contract(case):
    """One minibatch at lr 0 with slabs 1, 3 and 32 and lists of 1 / 31 / 32 / 33 / 64 / 65 / all rows, per gradient tensor against the
    float64 bf16 twin at the exported masters; 5 and 32 slabs give the same bytes on the inter kind (three tiles under both)."""
    from intent_radio_sched_multi_slice_amd import adapters as ad
    _, act, layout = _nets(case)
    env = _env(case, slabs=1)
    rec = env.collect(ref.T)
    host = {k: v.cpu() for k, v in rec.items()}
    order = _order(rec, 1)
    assert int(order["first_inter"][1]) == 96 and int(order["first_intra"][1]) > 130
    masters = ref.weights(env, 1)
    for r in ref.ROLES:          # (seeded from the acting copy: every master weight is a bf16 number)
        assert all(np.array_equal(br.bf16(w), w) for w, _ in masters[r][0])
    # no ratio of the twin near the clip boundary: clip_frac is decided (at unchanged weights the ratio is 1 but for rounding)
    for kind, a, c in (("inter", "inter", "v_inter"), ("intra", "intra", "v_intra")):
        n = int(order["first_" + kind][1])
        batch = ad.ppo_rows(host, kind, order["order_" + kind][0, :n].cpu(), layout)
        f64 = lambda net: [(torch.as_tensor(w, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)) for w, b in net]      # noqa: E731
        _, st = ad.ppo_loss_reference(f64(masters[a][0]), f64(masters[c][0]), batch, kind, 0.2, 0.5, 0.01, True, act, act, precision="bf16")
        ratio = torch.exp(st["logp"].to(torch.float64) - batch["logp"]).numpy()
        assert np.all(np.abs(ratio - 0.8) > 1e-3) and np.all(np.abs(ratio - 1.2) > 1e-3)
    # (KEEP THE SHORT LISTS: over all rows alone a truncated D, an unrounded D and the backward product on the master stay at 0.3 to 0.4 of
    #  the cap on relu24's intra tensors -- the weights' rounding is most of e_bf there; tests/test_ppo_bf16_cpu.py shows the slips
    #  beyond the cap on the maximum over exactly these seven lists, so this check detects them through the short ones)
    lists = [(f"{n} rows", _cut(order, n)) for n in (1, 31, 32, 33, 64, 65)] + [("all rows", order)]
    cache, worst, outs = {}, 0.0, {}
    for slabs in (1, 3, 32):
        env.ppo_bind(spread=True, slabs=slabs, bf16=True)
        for what, lst in lists:
            out = env.ppo_update(rec, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, order=lst, grad=True)
            worst = max(worst, _check_against_the_contract(out, _twins(host, lst, masters, act, layout, cache, what), masters, f"{case}, {slabs} slabs, {what}"))
        outs[slabs] = out
    env.ppo_bind(spread=True, slabs=5, bf16=True)
    outs[5] = env.ppo_update(rec, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, order=order, grad=True)
    assert torch.equal(outs[5]["grad"][0, 0], outs[32]["grad"][0, 0]), "the inter kind: 5 and 32 slabs differ on three tiles"
    print(f"{case}: worst device error / e_bf over slabs, lists, kinds and tensors: {worst:.3g} (cap 0.25)")
    assert 0.0 < worst <= 0.25
    env.close()


# ---- 4. Adam and the re-round -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["relu24", "tanh40x24"])
def test_one_adam_step_and_the_rerounded_acting_copy(case):
    """One step at lr > 0 from zero moments: masters, m and v against adam_step_f32 on the call's own dev_grad within 4 ulp.  Then a
    twin handle bound with the exported masters under precision="bf16" records, for the same seeds, the bytes the trained handle
    records: the acting copy is bf16(master).  Then a one-minibatch call on the trained handle agrees with the twin of the contract at
    the new masters: the transposed copy was refreshed."""
    nets, act, layout = _nets(case)
    env = _env(case, slabs=3)
    rec = env.collect(ref.T)
    logp_first = rec["logp"].clone()           # (collect() reuses its tensors: the second record overwrites the first)
    order = _order(rec, 1)
    w0 = ref.weights(env, 1)
    hp = dict(lr=np.array([1e-2]), grad_clip=np.array([0.05]), betas=(0.9, 0.999), eps=1e-8)
    out = env.ppo_update(rec, epochs=1, minibatch=ALL, order=order, grad=True, **hp)
    w1 = ref.weights(env, 1)
    ref.check_adam_step(env, out, w0, w1, hp, 1, f"{case}, bf16, 3 slabs")
    moved = 0
    for r in ref.ROLES:
        assert all(not np.array_equal(x[0], y[0]) for x, y in zip(w0[r][0], w1[r][0])), f"a layer of {r} did not move"
        moved += sum(int((br.bf16(w) != br.bf16(v)).sum()) for (w, _), (v, _) in zip(w0[r][0], w1[r][0]))
    assert moved > 100, "the step is too small to move the acting copy: the check below would show nothing"
    twin = ref.native_workload(B)
    _bind_nets(twin, nets, layout)
    twin.reset()
    first = twin.collect(ref.T)
    torch.cuda.synchronize()
    assert all(torch.equal(first[k], rec[k]) for k in rec)
    _bind_nets(twin, {r: w1[r][0] for r in ref.ROLES}, layout, activation=act)
    rec2, rec2_twin = env.collect(ref.T), twin.collect(ref.T)
    torch.cuda.synchronize()
    for k in rec2:
        assert torch.equal(rec2[k], rec2_twin[k]), f"{k}: the trained handle does not act on bf16(master)"
    assert not torch.equal(rec2["logp"], logp_first)
    order2 = _order(rec2, 1, seed=4)
    host2 = {k: v.cpu() for k, v in rec2.items()}
    worst = 0.0
    for what, lst in [(f"{n} rows", _cut(order2, n)) for n in (1, 31, 32, 33, 64, 65)] + [("all rows", order2)]:      # (the lists the CPU test shows the slips on)
        out2 = env.ppo_update(rec2, epochs=1, minibatch=ALL, lr=0.0, grad_clip=None, order=lst, grad=True)
        worst = max(worst, _check_against_the_contract(out2, _twins(host2, lst, w1, act, layout, {}, what), w1, f"{case}, behind an Adam step, {what}"))
    print(f"{case}: behind an Adam step, worst device error / e_bf: {worst:.3g}")
    env.close()
    twin.close()


# ---- 5. determinism and the loop ------------------------------------------------------------------------------------------------------------
def _twin_envs(case, slabs=3):
    env_a, env_b = _env(case, slabs), _env(case, slabs)
    rec_a, rec_b = env_a.collect(ref.T), env_b.collect(ref.T)
    torch.cuda.synchronize()
    assert all(torch.equal(rec_a[k], rec_b[k]) for k in rec_a)
    return env_a, env_b, rec_a, rec_b


def _same_next_collect(env_a, env_b, what):
    rec_a, rec_b = env_a.collect(3), env_b.collect(3)
    torch.cuda.synchronize()
    for k in rec_a:
        assert torch.equal(rec_a[k], rec_b[k]), f"{what}: the next collect() differs in {k}: the acting copies differ"


def test_the_same_call_gives_the_same_bytes():
    env_a, env_b, rec_a, rec_b = _twin_envs("tanh40x24")
    order = _order(rec_a, 2)
    hp = dict(epochs=2, minibatch=40, lr=3e-3, order=order, grad=True)
    out_a, out_b = env_a.ppo_update(rec_a, **hp), env_b.ppo_update(rec_b, **hp)
    ref.same_state(ref.state(env_a, 1), ref.state(env_b, 1), "the same bf16 spread call on twin handles")
    assert torch.equal(out_a["grad"], out_b["grad"]) and bool(out_a["grad"].any())
    for name in out_a:
        if name != "grad":
            assert np.asarray(out_a[name]).tobytes() == np.asarray(out_b[name]).tobytes(), name
    _same_next_collect(env_a, env_b, "the same call")
    env_a.close()
    env_b.close()


@pytest.mark.parametrize("minibatch", [12, 40])
def test_the_loop_of_steps_equals_one_call_per_chunk(minibatch):
    """2 epochs of minibatches of 12 and of 40 at 3 slabs in ONE call against the same chunks one call each on a twin handle: masters,
    moments and counters byte for byte, and the acting copies through the next collect() -- a stale acting or transposed copy between
    two steps of a call would show here"""
    case, E = "tanh40x24", 2
    env_a, env_b, rec_a, rec_b = _twin_envs(case)
    order = _order(rec_a, E)
    start = ref.state(env_a, 1)
    env_a.ppo_update(rec_a, epochs=E, minibatch=minibatch, order=order, **HP_LOOP)
    n_rows = [int(order["first_" + k][1]) for k in ("inter", "intra")]
    n_chunks = [-(-n // minibatch) for n in n_rows]
    assert min(n_chunks) >= 2 and n_chunks[0] != n_chunks[1]
    for ep in range(E):
        for i in range(max(n_chunks)):
            env_b.ppo_update(rec_b, epochs=1, minibatch=ALL, order=ref.chunk_order(order, 1, minibatch, ep, i), **HP_LOOP)
    a, b = ref.state(env_a, 1), ref.state(env_b, 1)
    ref.same_state(a, b, f"minibatch {minibatch}: one call against one call per chunk")
    assert all(a[k].tobytes() != start[k].tobytes() for k in a if k.split("/")[-1][0] == "w"), "a weight matrix did not move"
    for kind_i, kind in enumerate(("inter", "intra")):
        assert int(a[f"{kind}/0/t"][0]) == int(a[f"v_{kind}/0/t"][0]) == E * n_chunks[kind_i]
    _same_next_collect(env_a, env_b, f"minibatch {minibatch}")
    env_a.close()
    env_b.close()


# ---- 6. the boundary ------------------------------------------------------------------------------------------------------------------------
def test_what_the_bf16_binding_refuses_and_how_a_rebind_ends_or_restarts_it():
    need_gpu()
    case = "tanh40x24"
    nets, act, layout = _nets(case)
    env = ref.native_workload(B)
    _bind_nets(env, nets, layout, precision="f32")
    env.reset()
    w_before = ref.weights(env, 1)
    bind = lambda **kw: env.ppo_bind(spread=True, slabs=kw.pop("slabs", 8), bf16=True, **kw)      # noqa: E731
    for slabs in (0, 257):
        code, text = ref.refusal(lambda: bind(slabs=slabs))
        assert code == E_INVALID and f"slabs {slabs} (1..256)" in text, text
    # bf16=True on f32 nets
    code, text = ref.refusal(bind)
    assert code == E_STATE and "the bound nets are float32" in text, text
    # a pair of mixed precision: bf16 actors beside f32 critics
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=ref.SEED, intra_input=layout, precision="bf16")
    code, text = ref.refusal(bind)
    assert code == E_STATE and "nets of one precision" in text and "inter value net is float32" in text, text
    w_after = ref.weights(env, 1, roles=("v_inter", "v_intra"))
    for r in ("v_inter", "v_intra"):
        for (w0, b0), (w1, b1) in zip(w_before[r][0], w_after[r][0]):
            assert w0.tobytes() == w1.tobytes() and b0.tobytes() == b1.tobytes(), f"a refused binding moved {r}"
    # without bf16=True every binding refuses the bf16 nets in today's words, and net_weights refuses them too
    env.set_value_network(nets["v_inter"], nets["v_intra"], precision="bf16")
    for kw in (dict(), dict(wide=True), dict(spread=True, slabs=8), dict(spread=True, slabs=8, wide=True)):
        code, text = ref.refusal(lambda: env.ppo_bind(**kw))
        assert code == E_STATE and "the PPO update trains float32 nets: the inter net is bf16" in text, (kw, text)
    code, text = ref.refusal(lambda: env.net_weights("inter"))
    assert code == E_STATE and "is bf16" in text, text
    # nets per slice and a population, in the binding's own words
    env.set_policy_network(nets["inter"], [nets["intra"]] * env.S, stochastic=True, seed=1, intra_input=layout, precision="bf16")
    code, text = ref.refusal(bind)
    assert code == E_STATE and "no nets per slice" in text and "per slice" in text, text
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=ref.SEED, intra_input=layout, precision="bf16")
    bind()                                     # (all four bf16, single: taken)
    rec = env.collect(ref.T)
    order = _order(rec, 1)
    env.ppo_update(rec, epochs=1, minibatch=40, lr=1e-3, order=order)
    before = ref.state(env, 1)
    assert before["v_inter/0/m"].any() and int(before["inter/0/t"][0]) == 3 and int(before["intra/0/t"][0]) > 3
    # the actors re-bound under the binding: masters re-seeded, both kinds restart, the critics keep their masters
    env.set_policy_network(nets["inter"], nets["intra"], stochastic=True, seed=ref.SEED, intra_input=layout, precision="bf16")
    after = ref.state(env, 1)
    for r in ref.ROLES:
        assert not after[f"{r}/0/m"].any() and not after[f"{r}/0/v"].any() and int(after[f"{r}/0/t"][0]) == 0, r
    for k in after:
        if k.split("/")[-1][0] in "wb":
            if k.startswith("v_"):
                assert after[k].tobytes() == before[k].tobytes(), f"re-binding the actors moved {k}"
            elif k.split("/")[-1][0] == "w":
                want = br.bf16(ref.layers_of(nets[k.split("/")[0]])[int(k.split("/")[-1][1:])][0].numpy())
                assert np.array_equal(after[k], want), f"{k}: the master is not the new acting copy widened"
    out = env.ppo_update(rec, epochs=1, minibatch=40, lr=1e-3, order=order)
    assert int(ref.state(env, 1)["inter/0/t"][0]) == 3 and np.all(np.isfinite(out["grad_norm"]))
    # a population of three members
    pop = ref.member_nets(case, 3)
    env.set_population(ref.FIRST)
    env.set_policy_network(pop["inter"], pop["intra"], stochastic=True, seed=1, intra_input=layout, precision="bf16")
    env.set_value_network(pop["v_inter"], pop["v_intra"], precision="bf16")
    code, text = ref.refusal(bind)
    assert code == E_STATE and "no population" in text and "per member" in text, text
    env.close()
    # a role re-bound as f32 ends the binding, and ppo_update says so
    env = _env(case)
    rec = env.collect(ref.T)
    env.set_value_network(nets["v_inter"], nets["v_intra"], precision="f32")
    code, text = ref.refusal(lambda: env.ppo_update(rec, epochs=1, minibatch=40, order=_order(rec, 1)))
    assert code == E_STATE and "no PPO state bound" in text, text
    env.close()
    # a role re-bound with a LARGER bf16 net no longer fits the f32 state the bind allocated: the binding ends as well.  (A pair beyond
    # the bf16 LDS plan cannot be bound on any handle -- S and Us are at most 16, a net has at most four hidden layers of 512: 159 232
    # bytes, tests/test_ppo_bf16_cpu.py -- so that refusal is a guard with no case to show here.)
    env = _env("relu24")
    rec = env.collect(ref.T)
    order = _order(rec, 1)
    env.ppo_update(rec, epochs=1, minibatch=40, lr=1e-3, order=order)
    larger = ref.make_role_nets(ref.S, ref.US, [40, 24], "relu", "obs", 4300)
    env.set_value_network(larger["v_inter"], larger["v_intra"], precision="bf16")
    code, text = ref.refusal(lambda: env.ppo_update(rec, epochs=1, minibatch=40, order=order))
    assert code == E_STATE and "no PPO state bound" in text, text
    code, text = ref.refusal(lambda: env.net_weights("v_inter"))
    assert code == E_STATE and "is bf16" in text, text
    env.ppo_bind(spread=True, slabs=3, bf16=True)          # (a new bind takes the larger critics beside the actors)
    out = env.ppo_update(rec, epochs=1, minibatch=40, lr=1e-3, order=order)
    assert int(ref.state(env, 1)["v_inter/0/t"][0]) == 3 and np.all(np.isfinite(out["grad_norm"]))
    env.close()
