"""The bf16 policy nets on the device (ranenv_mlp.precision = RANENV_NET_BF16, include/ranenv.h) against tests/policy_bf16_ref.py:
integer-valued nets that every summation order must reproduce bit for bit -- through step(), rollout() and collect(), shared and
per-slice intra nets, head actors on both sources, bf16 and f32 nets paired in one fused or split launch --, random nets inside the
float64 twin's bound with at most 2 % of the scores beyond 1e-4, an env driven by bf16 nets against the CPU oracle, and the error
rules.  tests/test_policy_bf16_cpu.py holds the reference side to its conditions on the same nets and inputs.

B = 70 is two full 32-row tiles and a tail of 6; three partitions start launches at envs that are no multiples of 32."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import policy_bf16_ref as br
from tests import policy_ref as pr
from tests.common import OBS_TOL, REW_TOL
from tests.gpu_common import make_inter_net, make_net, need_gpu

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -3
B = br.B_TEST
STATS = {"ratio": 0.0, "share": 0.0}     # over the random cases: largest error / t, largest share beyond 1e-4


def _workload(S, Us, batch=B, max_steps=1000, seed=10, trace_len=32, R=25):
    """An env whose scenarios 0..3 have every slice active and 4..7 from 1 to S slices; env b plays scenario b % 8."""
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.scenario import generate_scaled_scenarios
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    U = min(S * Us, 256)
    wl = make_mult_slice_workload(batch, torch.device("cuda", 0), policy=_lib.POLICY_MAPF, intra=_lib.INTRA_PF, n_scenarios=8,
                                  n_traces=8, trace_len=trace_len, seed=seed, n_slices=S, n_ues=U, n_rbs=R, rbs_per_rbg=1,
                                  max_ues_slice=Us, max_steps=max_steps, min_slices=1, min_ues=1)
    full = generate_scaled_scenarios(4, seed=seed + 1, n_slices=S, n_ues=U, max_ues_slice=Us, min_slices=S, min_ues=1)
    for f in dataclasses.fields(full):
        getattr(wl.tables, f.name)[:4] = getattr(full, f.name)
    env = wl.env
    env.load_scenarios(wl.tables)
    eps = env.episodes
    scen = np.arange(batch) % 8
    env.set_episodes(scenario=scen, se_base=eps["se_base"], se_len=eps["se_len"], se_offset=eps["se_offset"],
                     trf_base=scen * trace_len, trf_len=trace_len, trf_offset=eps["trf_offset"])
    wl.scenario = scen
    return wl


def _snapshot(env):
    v = env.views()
    return {k: v[k].cpu().numpy().copy() for k in ("mask_inter", "mask_intra", "episode_number", "step_number")} | {
        "obs_inter": env.obs_inter.cpu().numpy().copy(), "obs_intra": env.obs_intra.cpu().numpy().copy()}


def _inject(env, oi, oa):
    env.obs_inter.copy_(torch.from_numpy(oi))
    env.obs_intra.copy_(torch.from_numpy(oa))


def _advance(env, how):
    if how == "step":
        env.step()
    else:
        env.rollout(1)
    torch.cuda.synchronize()


def _layers(net):
    from intent_radio_sched_multi_slice_amd.batched_env import policy_net_layers
    return policy_net_layers(net)


def _ref(snap, inter, intra, stochastic, seed, layout, forward):
    n = snap["obs_inter"].shape[0]
    return pr.PolicyRef(snap["obs_inter"], snap["mask_inter"], inter, snap["obs_intra"], snap["mask_intra"], intra, stochastic=stochastic,
                        seed=seed, layout=layout, env_ids=np.arange(n), episode=snap["episode_number"], step=snap["step_number"],
                        forward=forward)


# ---- a. exact, deterministic -------------------------------------------------------------------------------------------------------
def _exact_env(case, parts=3):
    arch, key, layout = case
    S, Us = br.SHAPES[key]
    wl = _workload(S, Us, seed=40 + br.EXACT_IDS.index(arch))
    if parts:
        wl.env.set_partitions(parts)
        lo, n = C.c_int32(), C.c_int32()
        cuts = []
        for p in range(parts):
            assert wl.env._lib.ranenv_get_partition(wl.env._h, p, C.byref(lo), C.byref(n)) == 0
            cuts.append(lo.value)
        assert parts == 1 or any(c % 32 for c in cuts[1:]), cuts
    return wl, wl.env, S, Us


def _check_exact_ttis(env, case, inter, intra):
    """TTI 0 through step(), TTI 1 through rollout(1) on injected 0 / 1 inputs: scores and intra choices equal to the exact reference."""
    layout = case[2]
    for t, how in enumerate(("step", "rollout")):
        oi, oa, _ = br.exact_case_inputs(case, t)
        _inject(env, oi, oa)
        snap = _snapshot(env)
        _advance(env, how)
        ref = _ref(snap, (inter, "relu"), (intra, "relu"), False, 0, layout, br.exact_forward_ref)
        pa = env.policy_actions()
        assert np.array_equal(pa["scores"].cpu().numpy(), ref.scores), (how, "scores")      # (masked positions included: -1)
        assert (~ref.active).any() and ref.active.any(axis=0).all()
        assert np.array_equal(pa["intra"].cpu().numpy(), ref.intra), (how, "intra")
        inside = ref.active & (np.abs(ref.out[:, :env.S]) < 1.0)
        assert inside.sum() >= 0.5 * ref.active.sum() and len(np.unique(ref.scores[inside])) >= 16     # not a clamped constant


@pytest.mark.parametrize("per_slice", [False, True], ids=["shared", "per-slice"])
@pytest.mark.parametrize("case", br.EXACT_CASES, ids=br.EXACT_IDS)
def test_exact_nets_bit_equal(case, per_slice):
    need_gpu()
    wl, env, S, Us = _exact_env(case)
    inter, intra, _, _ = br.exact_case_nets(case[0], S, Us, case[2], br.exact_case_seed(case), per_slice=per_slice)
    env.set_policy_network(inter, intra, intra_input=case[2], activation="relu", precision="bf16")
    env.reset()
    _check_exact_ttis(env, case, inter, br.PerSlice(intra) if per_slice else intra)
    env.close()


def test_exact_nets_bit_equal_one_partition():
    need_gpu()
    case = br.EXACT_CASES[4]
    wl, env, S, Us = _exact_env(case, parts=1)
    inter, intra, _, _ = br.exact_case_nets(case[0], S, Us, case[2], br.exact_case_seed(case))
    env.set_policy_network(inter, intra, intra_input=case[2], activation="relu", precision="bf16")
    env.reset()
    _check_exact_ttis(env, case, inter, intra)
    env.close()


@pytest.mark.parametrize("source", ["head", "inter"])
@pytest.mark.parametrize("case", br.EXACT_CASES, ids=br.EXACT_IDS)
def test_exact_head_actor_bit_equal(case, source):
    need_gpu()
    wl, env, S, Us = _exact_env(case)
    actor = br.exact_case_nets(case[0], S, Us, case[2], br.exact_case_seed(case) + 5, head_out=S)[0]
    if source == "head":
        env.enable_heads()
    env.set_head_policy_network(actor, "gauss_clip", log_std=np.zeros(S, dtype=np.float32), activation="relu", allow_sorted=True,
                                observation=source, precision="bf16")
    env.reset()
    for t, how in enumerate(("step", "rollout")):
        oi = br.exact_case_inputs(case, t)[0]
        (env.head_obs if source == "head" else env.obs_inter).copy_(torch.from_numpy(oi))
        _advance(env, how)
        want = np.clip(br.exact_forward(oi, actor), -1.0, 1.0)
        assert np.array_equal(env.policy_actions()["scores"].cpu().numpy(), want), how
        assert len(np.unique(want)) >= 16
    env.close()


# ---- b. exact through collect(2): bf16 and f32 nets paired in one launch ------------------------------------------------------------
@pytest.mark.parametrize("precisions", [("bf16", "bf16"), ("bf16", "f32"), ("f32", "bf16")], ids=lambda p: f"actor-{p[0]}-critic-{p[1]}")
@pytest.mark.parametrize("case", [br.EXACT_CASES[1], br.EXACT_CASES[4]], ids=[br.EXACT_IDS[1], br.EXACT_IDS[4]])
def test_exact_through_collect(case, precisions):
    need_gpu()
    pa, pv = precisions
    wl, env, S, Us = _exact_env(case)
    layout = case[2]
    a_inter, a_intra, v_inter, v_intra = br.exact_case_nets(case[0], S, Us, layout, br.exact_case_seed(case))
    env.set_policy_network(a_inter, a_intra, intra_input=layout, activation="relu", precision=pa)
    env.set_value_network(v_inter, v_intra, activation="relu", precision=pv)
    env.reset()
    for split in (0, 1):
        env.set_option("collect_split", split)
        oi, oa, _ = br.exact_case_inputs(case, split)
        _inject(env, oi, oa)
        snap = _snapshot(env)
        rec = {k: v.cpu().numpy() for k, v in env.collect(2).items()}
        # slot 0, the injected inputs: bit-equal
        assert np.array_equal(rec["obs_inter"][0], oi) and np.array_equal(rec["obs_intra"][0], oa)
        active = pr.sorted_mask(snap["mask_inter"])
        mean = br.exact_forward(oi, a_inter)[:, :S]
        assert np.array_equal(rec["action_inter"][0], np.where(active, mean, -1.0)), (split, "action_inter")
        xa = pr.intra_input(oa, snap["mask_intra"], layout)
        lg = br.exact_forward(xa, a_intra).reshape(B, S, 3)
        assert np.array_equal(rec["action_intra"][0], np.argmax(lg, axis=-1)), (split, "action_intra")
        assert np.array_equal(rec["vf"][0][:, 0].astype(np.float64), br.exact_forward(oi, v_inter)[:, 0]), (split, "vf inter")
        assert np.array_equal(rec["vf"][0][:, 1:].astype(np.float64), br.exact_forward(xa, v_intra).reshape(B, S)), (split, "vf intra")
        # slot 1 and the bootstrap slot, real observations: inside the bound of each net's precision
        fwd = {"bf16": br.mlp64_bf16, "f32": pr.mlp64}
        y, t = fwd[pa](rec["obs_inter"][1], a_inter, "relu")
        act1 = pr.sorted_mask(rec["mask_inter"][1])
        assert np.all(np.abs(rec["action_inter"][1] - y[:, :S])[act1] <= t[:, :S][act1]) and np.all(rec["action_inter"][1][~act1] == -1.0)
        for slot, obs in ((1, rec["obs_inter"][1]), (2, env.obs_inter.cpu().numpy())):
            y, t = fwd[pv](obs, v_inter, "relu")
            assert np.all(np.abs(rec["vf"][slot][:, 0] - y[:, 0]) <= t[:, 0] + 2.0 ** -24 * np.abs(y[:, 0])), (split, slot)
        y, t = fwd[pv](pr.intra_input(rec["obs_intra"][1], rec["mask_intra"][1], layout), v_intra, "relu")
        y, t = y.reshape(B, S), t.reshape(B, S)
        assert np.all(np.abs(rec["vf"][1][:, 1:] - y) <= t + 2.0 ** -24 * np.abs(y)), split
    env.close()


def test_collect_records_the_unrounded_observation():
    need_gpu()
    case = br.RANDOM_CASES[0]
    S, Us = br.SHAPES[case[1]]
    env = _workload(S, Us, seed=47).env
    inter, intra = br.random_case_nets(case)
    env.set_policy_network(inter, intra, precision="bf16")
    env.set_value_network(make_net([10 * S, 64, 1], "tanh", 3), None, precision="bf16")
    env.reset()
    oi, oa = br.random_case_inputs(case)
    assert not np.array_equal(br.bf16(oi), oi)
    _inject(env, oi, oa)
    rec = env.collect(1)
    assert np.array_equal(rec["obs_inter"][0].cpu().numpy(), oi) and np.array_equal(rec["obs_intra"][0].cpu().numpy(), oa)
    env.close()


# ---- c. random nets -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", br.RANDOM_CASES, ids=br.RANDOM_IDS)
def test_random_nets_within_bound(case):
    need_gpu()
    name, key, widths, act, st, gain = case
    S, Us = br.SHAPES[key]
    env = _workload(S, Us, seed=50 + br.RANDOM_IDS.index(name)).env
    env.set_partitions(3)
    inter, intra = br.random_case_nets(case)
    seed = 0x9E37_79B9_7F4A_7C15 + br.RANDOM_IDS.index(name)
    env.set_policy_network(inter, intra, stochastic=st, seed=seed, precision="bf16")
    env.reset()
    far = n = 0
    worst = 0.0
    for t, how in enumerate(("step", "rollout")):
        _inject(env, *br.random_case_inputs(case, t))
        snap = _snapshot(env)
        _advance(env, how)
        ref = _ref(snap, _layers(inter), _layers(intra), st, seed, "obs", br.mlp64_bf16)
        pa = env.policy_actions()
        sc = pa["scores"].cpu().numpy()
        err = np.abs(sc - ref.scores)[ref.active]
        bnd = ref.score_bound[ref.active]
        worst = max(worst, float(np.max(err[bnd > 0] / bnd[bnd > 0])))
        far, n = far + int((err > 1e-4).sum()), n + err.size
        print(f"{name} TTI {t}: largest score error {err.max():.3g}, largest error / t {worst:.3g}, beyond 1e-4 {int((err > 1e-4).sum())} of {err.size}")
        assert pr.check_actions(ref, sc, pa["intra"].cpu(), min_safe=0.5) >= 0.5 * B * S
    share = far / n
    print(f"{name}: largest error / t {worst:.3g}, share of scores beyond 1e-4 {share:.3%}")
    STATS["ratio"], STATS["share"] = max(STATS["ratio"], worst), max(STATS["share"], share)
    assert share <= 0.02
    env.close()


# ---- d. env level ---------------------------------------------------------------------------------------------------------------------
def test_env_under_bf16_nets_matches_oracle_across_autoreset():
    need_gpu()
    from oracle import pyoracle
    S, Us, batch, L, steps, trace_len = 5, 5, 33, 5, 12, 16
    wl = _workload(S, Us, batch, max_steps=L, seed=61, trace_len=trace_len)
    env, tabs = wl.env, wl.tables
    inter = make_inter_net(S, [64, 64], "tanh", 71)
    intra = make_net([env.W + env.Us, 64, 64, 3], "relu", 72)
    env.set_policy_network(inter, intra, stochastic=True, seed=0x1357_9BDF, intra_input="mask_obs", precision="bf16")
    n_ep, first = 8, 0x0100_0000
    ep_no = np.arange(n_ep)
    env.set_episode_table(scenario=ep_no % 8, se_base=(ep_no % 8) * trace_len, se_len=trace_len, se_offset=(ep_no * 5) % trace_len,
                          trf_base=(ep_no % 8) * trace_len, trf_len=trace_len, trf_offset=(ep_no * 3) % trace_len, first_episode=first)
    start = first + np.arange(batch) % n_ep
    env.enable_autoreset(first, first + n_ep, episode_numbers=start)
    tab = env.episode_table
    se_host = wl.se_pool.transpose(1, 2).contiguous().cpu().numpy()
    trf_host = wl.traffic_pool.cpu().numpy().astype(np.float64)

    def tile(ep, t): r = tab[ep - first]; return int(r["se_base"] + (r["se_offset"] + t) % r["se_len"])
    def trow(ep, t): r = tab[ep - first]; return int(r["trf_base"] + (r["trf_offset"] + t) % r["trf_len"])

    ocfg = pyoracle.make_cfg(S, env.U, env.R, env.G, Us, max_steps=10 ** 6)
    oenvs, cur, tstep = [], start.copy(), np.zeros(batch, dtype=int)
    for b in range(batch):
        o = pyoracle.OracleEnv(ocfg); o.set_scenario(tabs, int(tab[cur[b] - first]["scenario"])); o.reset(se_host[tile(cur[b], 0)])
        oenvs.append(o)
    env.reset()
    ends = 0
    for t in range(steps):
        snap = _snapshot(env)
        env.step()
        torch.cuda.synchronize()
        ref = _ref(snap, _layers(inter), _layers(intra), True, 0x1357_9BDF, "mask_obs", br.mlp64_bf16)
        pa = env.policy_actions()
        pr.check_actions(ref, pa["scores"].cpu(), pa["intra"].cpu(), min_safe=0.0)           # (real observations: ties)
        sc, ic = pa["scores"].cpu().numpy(), pa["intra"].cpu().numpy().astype(np.int32)
        g = {name: x.cpu().numpy() for name, x in env.views().items()}
        oi, oa, rw, dn = (env.obs_inter.cpu().numpy(), env.obs_intra.cpu().numpy(), env.reward.cpu().numpy(), env.done.cpu().numpy())
        for b, o in enumerate(oenvs):
            o.step(sc[b].copy(), ic[b].copy(), se_host[tile(cur[b], tstep[b])], trf_host[trow(cur[b], tstep[b])])
            tstep[b] += 1
            oo = o.obs()
            np.testing.assert_allclose(rw[b], oo["reward"], rtol=0, atol=REW_TOL)
            is_done = tstep[b] >= L
            assert bool(dn[b]) == is_done, (t, b)
            if not is_done:
                raw = o.raw()
                for name in ("pkt_effective_thr", "dropped_pkts", "pkt_throughputs"):
                    assert np.array_equal(g[name][b], raw[name]), (name, t, b)
                np.testing.assert_allclose(oi[b], oo["obs_inter"], rtol=0, atol=OBS_TOL)
                np.testing.assert_allclose(oa[b], oo["obs_intra"], rtol=0, atol=OBS_TOL)
                continue
            ends += 1
            nxt = cur[b] + 1 if cur[b] + 1 < first + n_ep else first
            cur[b], tstep[b] = nxt, 0
            assert int(g["episode_number"][b]) == nxt
            o.set_scenario(tabs, int(tab[nxt - first]["scenario"]))
            o.reset(se_host[tile(nxt, 0)])
            ro = o.obs()
            np.testing.assert_allclose(oi[b], ro["obs_inter"], rtol=0, atol=OBS_TOL)
            np.testing.assert_allclose(oa[b], ro["obs_intra"], rtol=0, atol=OBS_TOL)
    assert ends == 2 * batch and OBS_TOL <= 1e-5 and REW_TOL <= 1e-9
    env.close()


# ---- e. errors and state ----------------------------------------------------------------------------------------------------------------
def _f32_check(env, inter, intra, rng):
    oi, oa = pr.injected_inputs(rng, env.B, env.S, env.Us)
    _inject(env, oi, oa)
    snap = _snapshot(env)
    env.step()
    pa = env.policy_actions()
    pr.check_actions(_ref(snap, _layers(inter), _layers(intra), False, 0, "obs", pr.mlp64), pa["scores"].cpu(), pa["intra"].cpu())
    return pa["scores"].cpu().numpy().copy()


def test_error_rules_and_rebinding():
    need_gpu()
    from intent_radio_sched_multi_slice_amd import _lib
    S, Us = 5, 5
    env = _workload(S, Us, seed=81).env
    lib, h, stream = env._lib, env._h, env._stream()
    rng = np.random.default_rng(9)
    inter, intra = make_inter_net(S, [64, 64], "tanh", 91), make_net([env.W, 33, 3], "tanh", 92)
    other = make_inter_net(S, [96], "relu", 93)
    env.set_policy_network(inter, intra)
    env.reset()
    _f32_check(env, inter, intra, rng)
    keep = []
    mlp = lambda net, precision, layout=_lib.NET_IN_OBS: env._mlp_struct(*_layers(net), layout, keep, precision)  # noqa: E731
    # an unknown precision: refused, and the previous nets go on acting
    assert lib.ranenv_set_policy_network(h, C.byref(mlp(other, 2)), None, 0, 0, stream) == E_INVALID and b"precision" in lib.ranenv_last_error(h)
    assert lib.ranenv_set_policy_network(h, C.byref(mlp(other, 0)), C.byref(mlp(intra, -1)), 0, 0, stream) == E_INVALID
    with pytest.raises(ValueError):
        env.set_policy_network(other, precision="fp8")
    _f32_check(env, inter, intra, rng)
    # per-slice copies of mixed precision
    copies = [mlp(make_net([env.W, 33, 3], "tanh", 100 + s), s % 2) for s in range(S)]
    arr = (C.POINTER(_lib.Mlp) * S)(*[C.pointer(m) for m in copies])
    assert lib.ranenv_set_intra_policy_networks(h, S, arr, stream) == E_INVALID and b"precision" in lib.ranenv_last_error(h)
    _f32_check(env, inter, intra, rng)
    # bf16, then f32 again on the same slots: the f32 results
    env.set_policy_network(inter, intra, precision="bf16")
    oi, oa = pr.injected_inputs(rng, env.B, S, Us)
    _inject(env, oi, oa)
    snap = _snapshot(env)
    env.step()
    pa = env.policy_actions()
    ref16 = _ref(snap, _layers(inter), _layers(intra), False, 0, "obs", br.mlp64_bf16)
    pr.check_actions(ref16, pa["scores"].cpu(), pa["intra"].cpu(), min_safe=0.5)
    ref32 = _ref(snap, _layers(inter), _layers(intra), False, 0, "obs", pr.mlp64)
    assert (np.abs(pa["scores"].cpu().numpy() - ref32.scores) > ref32.score_bound)[ref32.active].mean() > 0.5     # (it did run in bf16)
    env.set_policy_network(inter, intra, precision="f32")
    _f32_check(env, inter, intra, rng)
    env.close()


def test_sac_rules():
    need_gpu()
    from intent_radio_sched_multi_slice_amd import _lib
    from tests import head_policy_ref as hr
    from tests import sac_ref as sr
    case = "64x64"
    _, env, _ = hr.make_env("S5U25", "64x64", "gauss_tanh", 8, bind=False)
    actor, q1, q2 = sr.sac_nets(case)
    lib, h, stream = env._lib, env._h, env._stream()
    keep = []
    mlp = lambda net, precision: env._mlp_struct(*hr.layers_of(net), _lib.NET_IN_OBS, keep, precision)  # noqa: E731
    obs, reward, done = (torch.as_tensor(a[:40]) for a in sr.sac_inputs(case))
    env.set_head_policy_network(actor, "gauss_tanh", stochastic=True, seed=1)
    assert lib.ranenv_set_sac_critics(h, C.byref(mlp(q1, 1)), C.byref(mlp(q2, 1)), stream) == E_INVALID
    assert lib.ranenv_set_sac_critics(h, C.byref(mlp(q1, 0)), C.byref(mlp(q2, 1)), stream) == E_INVALID
    with pytest.raises(_lib.RanEnvError, match="critics"):          # (no refused binding bound anything)
        env.sac_targets(obs, reward, done)
    env.set_sac_critics(q1, q2)
    want = env.sac_targets(obs, reward, done, seed=5, draw=6)["target"].clone()
    env.set_head_policy_network(actor, "gauss_tanh", stochastic=True, seed=1, precision="bf16")
    with pytest.raises(_lib.RanEnvError, match=r"\(-3\)"):
        env.sac_targets(obs, reward, done, seed=5, draw=6)
    env.step()                                                       # the bf16 head actor itself acts
    torch.cuda.synchronize()
    env.set_head_policy_network(actor, "gauss_tanh", stochastic=True, seed=1)
    assert torch.equal(env.sac_targets(obs, reward, done, seed=5, draw=6)["target"], want)
    env.close()


def test_f32_actor_unmoved_by_a_bf16_critic_beside_it():
    need_gpu()
    S, Us = 5, 5
    inter, intra = make_inter_net(S, [64, 64], "tanh", 95), make_net([2 * Us + 9, 64, 64, 3], "relu", 96)
    v_inter, v_intra = make_net([10 * S, 64, 64, 1], "tanh", 97), make_net([2 * Us + 9, 64, 64, 1], "relu", 98)
    recs = []
    for pv in ("f32", "bf16"):
        env = _workload(S, Us, seed=83).env
        env.set_policy_network(inter, intra, stochastic=True, seed=7)
        env.set_value_network(v_inter, v_intra, precision=pv)
        env.reset()
        rec = {k: v.cpu().clone() for k, v in env.collect(3).items()}
        rec["scores"] = env.policy_actions()["scores"].cpu().clone()
        recs.append(rec)
        env.close()
    for k in ("action_inter", "action_intra", "logp", "obs_inter", "reward", "scores"):
        assert torch.equal(recs[0][k], recs[1][k]), k
    assert not torch.equal(recs[0]["vf"], recs[1]["vf"])             # (the critic did change)
    assert (recs[0]["vf"] - recs[1]["vf"]).abs().max() < 0.05


def test_zz_report():
    """Not a check: the random cases' figures."""
    need_gpu()
    print(f"\nbf16 policy nets, random cases: largest error / t {STATS['ratio']:.3g}, largest share of scores beyond 1e-4 {STATS['share']:.3%}")
