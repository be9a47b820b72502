"""Non-shared intra policies on the device (ranenv_set_intra_policy_networks / _intra_value_networks; the sliced policy kernels):
S copies of one net against the shared path bit for bit, distinct nets against the float64 twin of tests/per_slice_policy_ref.py,
every path that launches the nets (step, ranges, partitioned rollouts, collect with fused and split critics), one closed loop
against the CPU oracle, and the binding rules of include/ranenv.h.

Batches of 33 and 70 are one and two full tiles of 32 envs plus a tail; widths 48 and 40 are padded, 512 is the LDS maximum."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import per_slice_policy_ref as ps
from tests import policy_ref as pr
from tests.common import OBS_TOL, REW_TOL
from tests.gpu_common import LOOSE_WIN_SENT, LOOSE_WIN_SENT_AND_SE, assert_same_state, make_net, need_gpu, to_host
from tests.test_gpu_policy_network import _KEYS, _episode_table
from tests.test_gpu_policy_network_shapes import _inject, _outside_untouched, _sentinel, _snapshot, _workload

pytestmark = pytest.mark.gpu

SEED = 0x2468_ACE0_1357_9BDF
E_INVALID, E_STATE = -1, -3
MODES = [False, True]
FIELDS = ("obs_inter", "obs_intra", "mask_inter", "mask_intra", "action_inter", "action_intra", "logp", "vf", "reward", "done", "adv", "vtarg")
K_CASES = range(len(ps.CASES))


def _env(case, seed, max_steps=1000, se_mode="stream"):
    S, Us, B = case[:3]
    wl = _workload(S, Us, B, max_steps=max_steps, seed=seed)
    wl.env.set_se_mode(se_mode)
    return wl, wl.env


def _bind(env, nets, layout, stochastic, actors=True, critics=True, with_critics=True):
    """The inter nets with per-slice (True) or shared (False: slice 0's net) intra actors / critics"""
    inter, intras, v_inter, v_intras = nets
    env.set_policy_network(inter, intras if actors else intras[0], stochastic=stochastic, seed=SEED, intra_input=layout)
    if with_critics:
        env.set_value_network(v_inter, v_intras if critics else v_intras[0])


def _actions(env):
    torch.cuda.synchronize()
    pa = env.policy_actions()
    return pa["scores"].cpu().numpy().copy(), pa["intra"].cpu().numpy().copy()


def _raw_set(env, call, nets, n, in_dim, out_dim, layout):
    """The C call itself on a list of nets (n as given): its status"""
    from intent_radio_sched_multi_slice_amd.batched_env import NET_INPUTS, policy_net_layers
    keep, structs = [], []
    for net in nets:
        layers, act = policy_net_layers(net, None, in_dim, out_dim)
        structs.append(env._mlp_struct(layers, act, NET_INPUTS[layout], keep))
    arr = (C.POINTER(type(structs[0])) * len(structs))(*[C.pointer(m) for m in structs])
    with torch.cuda.device(env.device):
        rc = getattr(env._lib, call)(env._h, n, arr, env._stream())
    torch.cuda.synchronize()               # (the sources may go once the copies have run)
    env._policy_views = None
    return rc


# ---- 1. S copies of one net are the shared path, bit for bit -----------------------------------------------------------------
@pytest.mark.parametrize("stochastic", MODES)
@pytest.mark.parametrize("k", K_CASES, ids=ps.CASE_IDS)
def test_copies_of_one_net_are_the_shared_path_bit_for_bit(k, stochastic):
    """Twin envs under one intra actor / critic: bound once, or as a list of S references to it -- both sets, the actors alone (shared
    critic), the critics alone (shared actor).  policy_actions() of a step on injected observations, the state after rollout(6) and
    every field of collect(6) agree exactly: each output element goes through the same MFMA sequence whichever tile row it sits in."""
    need_gpu()
    case = ps.CASES[k]
    S, layout = case[0], case[5]
    inter, intras, v_inter, v_intras = ps.make_nets(case, 700 + 10 * k)
    nets = (inter, [intras[0]] * S, v_inter, [v_intras[0]] * S)
    runs = {}
    for how, (actors, critics) in {"shared": (False, False), "both": (True, True), "actors": (True, False), "critics": (False, True)}.items():
        wl, env = _env(case, 70 + k)
        _bind(env, nets, layout, stochastic, actors, critics)
        env.reset()
        _inject(env, np.random.default_rng(k))
        env.step()
        out = dict(zip(("step_scores", "step_intra"), _actions(env)))
        env.rollout(6)
        out.update({"view_" + name: x for name, x in to_host(env.views()).items()})
        out.update({"out_" + name: getattr(env, name).cpu().numpy().copy() for name in ("obs_inter", "obs_intra", "reward", "done")})
        out.update({"rec_" + name: x for name, x in to_host(env.collect(6)).items()})
        out.update(dict(zip(("end_scores", "end_intra"), _actions(env))))
        runs[how] = out
        env.close()
    assert set(FIELDS) <= {name[4:] for name in runs["shared"] if name.startswith("rec_")}
    assert np.any(runs["shared"]["rec_logp"][:, :, 1:] != 0.0) and np.any(runs["shared"]["rec_vf"][-1][:, 1:] != 0.0)
    for how in ("both", "actors", "critics"):
        for name, want in runs["shared"].items():
            assert np.array_equal(runs[how][name], want), (how, name, int((runs[how][name] != want).sum()))


# ---- 2. distinct nets against the float64 twin -------------------------------------------------------------------------------
@pytest.mark.parametrize("stochastic", MODES)
@pytest.mark.parametrize("k", K_CASES, ids=ps.CASE_IDS)
def test_distinct_nets_match_the_float64_twin(k, stochastic):
    """A step on injected observations: scores and intra choices of every (env, slice) row -- inactive slices' rows included, the
    kernel computes them all -- against slice s's net in float64; then collect(3): the intra columns of logp and of vf, bootstrap slot
    included, within the bounds of collect_ref on the recorded rows."""
    need_gpu()
    case = ps.CASES[k]
    S, Us, B, widths, act, layout = case
    nets = ps.make_nets(*ps.TWIN_NETS[k])
    inter, intras, v_inter, v_intras = nets
    wl, env = _env(case, 80 + k)
    _bind(env, nets, layout, stochastic)
    env.reset()
    rng = np.random.default_rng(10 + k)
    checked = 0
    for t in range(2):
        _inject(env, rng)
        snap = _snapshot(env)
        env.step()
        torch.cuda.synchronize()
        pa = env.policy_actions()
        checked += pr.check_actions(ps.policy_ref(snap, inter, intras, stochastic, SEED, layout), pa["scores"].cpu(), pa["intra"].cpu(), min_safe=0.9)
    assert checked >= 0.9 * 2 * B * S
    _inject(env, rng)
    rec = to_host(env.collect(3))
    assert not rec["mask_inter"].all() and rec["mask_inter"][:, 0].all()        # inactive slices' rows are among those compared
    worst = {"logp": 0.0, "vf": 0.0}
    for t in range(3):
        worst["logp"] = max(worst["logp"], ps.check_intra_logp(rec, t, intras, layout))
        worst["vf"] = max(worst["vf"], ps.check_intra_values(rec["vf"][t], rec["obs_inter"][t], rec["obs_intra"][t], rec["mask_intra"][t],
                                                               v_inter, v_intras, layout, f"vf[{t}]"))
    worst["vf_T"] = ps.check_intra_values(rec["vf"][3], env.obs_inter, env.obs_intra, env.views()["mask_intra"], v_inter, v_intras, layout, "vf[T]")
    print(f"{ps.CASE_IDS[k]} stochastic={stochastic}: worst error / bound {worst}")
    env.close()


# ---- 3. launch paths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("se_mode", ["stream", "gather"])
@pytest.mark.parametrize("k", [1, 3], ids=[ps.CASE_IDS[1], ps.CASE_IDS[3]])
def test_partitioned_rollouts_equal_the_step_loop(k, se_mode):
    """rollout(n) over 1 and 3 partitions == n x step() under distinct nets, stochastic, across episode ends (episodes of 4 TTIs, n = 9)"""
    need_gpu()
    case, n = ps.CASES[k], 9
    nets = ps.make_nets(case, 900 + k)

    def make(parts):
        wl, env = _env(case, 90 + k, max_steps=4, se_mode=se_mode)
        _bind(env, nets, case[5], True, with_critics=False)
        _episode_table(env)
        if parts > 1:
            env.set_partitions(parts)
        env.reset()
        return wl, env
    wl, ref = make(1)
    for _ in range(n):
        ref.step()
    assert bool((ref.views()["step_number"] == n % 4).all())       # (every env is in its third episode)
    for parts in (1, 3):
        _, env = make(parts)
        env.rollout(n)
        assert_same_state(ref, env, wl.tables, (parts, se_mode), loose=LOOSE_WIN_SENT, keys=_KEYS, actions=("scores", "intra"))
        env.close()
    ref.close()


@pytest.mark.parametrize("se_mode", ["stream", "gather"])
def test_ranges_whose_boundary_is_no_tile_boundary_equal_the_whole_batch_step(se_mode):
    """step_async on two ranges of 35 envs each == step() of the 70, TTI by TTI over 7 TTIs under auto-reset with episodes of 3, 4 and 5
    TTIs (env b: 3 + b % 3), so the ranges' launches follow device-side resets and see episode and step counters that differ from env
    to env; at every TTI a range's launch leaves the other range's actions alone (sentinel fill) and gives the whole batch's actions."""
    need_gpu()
    case, n = ps.CASES[1], 7
    B = case[2]
    nets = ps.make_nets(case, 910)
    envs = []
    for ranged in (False, True):
        wl, env = _env(case, 95, max_steps=4, se_mode=se_mode)
        _bind(env, nets, case[5], True, with_critics=False)
        env.set_max_steps(3 + np.arange(B) % 3)
        _episode_table(env)
        ranges = env.set_ranges(2) if ranged else None
        env.reset()
        _inject(env, np.random.default_rng(5))
        envs.append(env)
    whole, env = envs
    assert ranges[0][1] == ranges[1][0] and ranges[0][1] % 32 != 0, ranges
    ends = np.zeros(B, dtype=int)
    for t in range(n):
        whole.step()
        want = _actions(whole)
        for r, (lo, hi) in enumerate(ranges):
            _sentinel(env)
            env.step_async(r)
            env.step_wait(r)
            torch.cuda.synchronize()
            _outside_untouched(env, lo, hi)
            got = _actions(env)
            assert np.array_equal(got[0][lo:hi], want[0][lo:hi]) and np.array_equal(got[1][lo:hi], want[1][lo:hi]), (t, r)
        for name in ("obs_inter", "obs_intra", "reward", "done", "term_obs_inter", "term_obs_intra"):
            assert torch.equal(getattr(env, name), getattr(whole, name)), (t, name)
        for name in ("pkt_effective_thr", "queue_pkts", "step_number", "episode_number"):
            assert torch.equal(env.views()[name], whole.views()[name]), (t, name)
        ends += whole.done.cpu().numpy() != 0
    assert np.array_equal(ends, n // (3 + np.arange(B) % 3))       # (every env restarted on the device, at its own TTIs)
    v = whole.views()
    assert len(set(v["step_number"].cpu().tolist())) == 3 and bool((v["episode_number"].cpu() != torch.arange(B)).all())
    whole.close()
    env.close()


# ---- 4. collect --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2], ids=[ps.CASE_IDS[1], ps.CASE_IDS[2]])
def test_collect_records_the_step_loop_and_moves_nothing_else(k):
    """collect(T) over 1 and 3 partitions under distinct actors and critics, stochastic, auto-reset: the record is TTI by TTI what a
    step() loop on a twin sees; state, caller buffers and policy_actions() afterwards are rollout(T)'s; fused and split critic launches
    (option collect_split) and the library's own choice give one record."""
    need_gpu()
    case, T = ps.CASES[k], 6
    nets = ps.make_nets(case, 920 + k)

    def make(parts=1, split=-1):
        wl, env = _env(case, 96 + k, max_steps=4)
        _bind(env, nets, case[5], True)
        _episode_table(env)
        if parts > 1:
            env.set_partitions(parts)
        assert env.get_option("collect_split") == -1
        env.set_option("collect_split", split)
        env.reset()
        return wl, env
    wl, ref = make()
    want = {name: [] for name in ("obs_inter", "obs_intra", "mask_inter", "mask_intra", "scores", "action_intra", "reward", "done")}
    v = ref.views()
    for _ in range(T):
        for name, x in (("obs_inter", ref.obs_inter), ("obs_intra", ref.obs_intra), ("mask_inter", v["mask_inter"]), ("mask_intra", v["mask_intra"])):
            want[name].append(x.clone())
        ref.step()
        pa = ref.policy_actions()
        for name, x in (("scores", pa["scores"]), ("action_intra", pa["intra"]), ("reward", ref.reward), ("done", ref.done)):
            want[name].append(x.clone())
    want = {name: torch.stack(x) for name, x in want.items()}
    assert bool(want["done"].any())
    ref.close()
    records = []
    for parts, split in ((1, -1), (3, 0), (3, 1)):
        _, a = make(parts, split)
        _, b = make(parts)
        rec = a.collect(T)
        b.rollout(T)
        torch.cuda.synchronize()
        for name in ("obs_inter", "obs_intra", "mask_inter", "mask_intra", "action_intra", "reward", "done"):
            assert torch.equal(rec[name], want[name]), (name, parts, split)
        assert torch.equal(rec["action_inter"].clamp(-1.0, 1.0), want["scores"]), (parts, split)
        assert_same_state(a, b, wl.tables, (parts, split), loose=LOOSE_WIN_SENT_AND_SE, actions=("scores", "intra"))
        records.append(to_host(rec))
        a.close()
        b.close()
    for name in FIELDS:
        assert np.array_equal(records[0][name], records[1][name]) and np.array_equal(records[1][name], records[2][name]), name
    assert np.any(records[0]["vf"][:, :, 1:] != 0.0) and np.any(records[0]["adv"][:, :, 1:] != 0.0)


# ---- 5. against the CPU oracle -----------------------------------------------------------------------------------------------
def test_env_driven_by_its_per_slice_actions_matches_the_oracle():
    """20 TTIs, episodes of 8: the oracle fed the device's own scores and per-slice intra choices stays with the device (integers
    exact, observations and rewards within OBS_TOL / REW_TOL), across the episode ends."""
    need_gpu()
    from oracle import pyoracle
    case = (3, 4, 7, [32], "tanh", "obs")
    S, Us, B, L, steps, trace_len = 3, 4, 7, 8, 20, 16
    wl = _workload(S, Us, B, max_steps=L, seed=97, trace_len=trace_len)
    env, tabs = wl.env, wl.tables
    nets = ps.make_nets(case, 930)
    _bind(env, nets, "obs", True, with_critics=False)
    n_ep, first = 8, 0x0100_0000
    ep_no = np.arange(n_ep)
    env.set_episode_table(scenario=ep_no % 8, se_base=(ep_no % 8) * trace_len, se_len=trace_len, se_offset=(ep_no * 5) % trace_len,
                          trf_base=(ep_no % 8) * trace_len, trf_len=trace_len, trf_offset=(ep_no * 3) % trace_len, first_episode=first)
    start = first + np.arange(B) % n_ep
    env.enable_autoreset(first, first + n_ep, episode_numbers=start)
    tab = env.episode_table
    se_host = wl.se_pool.transpose(1, 2).contiguous().cpu().numpy()
    trf_host = wl.traffic_pool.cpu().numpy().astype(np.float64)

    def tile(ep, t): r = tab[ep - first]; return int(r["se_base"] + (r["se_offset"] + t) % r["se_len"])
    def trow(ep, t): r = tab[ep - first]; return int(r["trf_base"] + (r["trf_offset"] + t) % r["trf_len"])

    ocfg = pyoracle.make_cfg(S, env.U, env.R, env.G, Us, max_steps=10 ** 6)
    oenvs, cur, tstep = [], start.copy(), np.zeros(B, dtype=int)
    for b in range(B):
        o = pyoracle.OracleEnv(ocfg); o.set_scenario(tabs, int(tab[cur[b] - first]["scenario"])); o.reset(se_host[tile(cur[b], 0)])
        oenvs.append(o)
    env.reset()
    ends, choices = 0, set()
    for t in range(steps):
        env.step()
        sc, ic = _actions(env)
        choices |= {(s, int(c)) for s in range(S) for c in ic[:, s]}
        g = {name: x.cpu().numpy() for name, x in env.views().items()}
        oi, oa, rw, dn = (env.obs_inter.cpu().numpy(), env.obs_intra.cpu().numpy(), env.reward.cpu().numpy(), env.done.cpu().numpy())
        for b, o in enumerate(oenvs):
            o.step(sc[b].copy(), ic[b].astype(np.int32), se_host[tile(cur[b], tstep[b])], trf_host[trow(cur[b], tstep[b])])
            tstep[b] += 1
            oo = o.obs()
            np.testing.assert_allclose(rw[b], oo["reward"], rtol=0, atol=REW_TOL)
            is_done = tstep[b] >= L
            assert bool(dn[b]) == is_done, (t, b)
            if is_done:
                ends += 1
                cur[b], tstep[b] = (cur[b] + 1 if cur[b] + 1 < first + n_ep else first), 0
                assert int(g["episode_number"][b]) == cur[b]
                o.set_scenario(tabs, int(tab[cur[b] - first]["scenario"]))
                o.reset(se_host[tile(cur[b], 0)])
                oo = o.obs()
            else:
                raw = o.raw()
                for name in ("pkt_effective_thr", "dropped_pkts", "pkt_throughputs"):
                    assert np.array_equal(g[name][b], raw[name]), (name, t, b)
            np.testing.assert_allclose(oi[b], oo["obs_inter"], rtol=0, atol=OBS_TOL)
            np.testing.assert_allclose(oa[b], oo["obs_intra"], rtol=0, atol=OBS_TOL)
    assert ends == 2 * B and len(choices) > S          # (the slices' nets do not all choose one scheduler)
    env.close()


# ---- 6. binding rules --------------------------------------------------------------------------------------------------------
def _step_and_check(env, rng, inter, intras, layout, stochastic=True):
    """A step on injected observations against the twin under ``intras`` (a list: per slice; one net: shared)"""
    _inject(env, rng)
    snap = _snapshot(env)
    env.step()
    torch.cuda.synchronize()
    pa = env.policy_actions()
    nets = intras if isinstance(intras, list) else [intras] * env.S
    pr.check_actions(ps.policy_ref(snap, inter, nets, stochastic, SEED, layout), pa["scores"].cpu(), pa["intra"].cpu(), min_safe=0.9)


def test_refused_calls_leave_the_previous_binding_in_place():
    need_gpu()
    case = ps.CASES[1]
    S, Us, B, widths, act, layout = case
    n_in = ps.intra_width(Us, layout)
    inter, intras, v_inter, v_intras = ps.make_nets(*ps.TWIN_NETS[1])
    wl, env = _env(case, 98)
    actor_call, value_call = "ranenv_set_intra_policy_networks", "ranenv_set_intra_value_networks"
    assert _raw_set(env, actor_call, intras, S, n_in, 3, layout) == E_STATE                 # no inter net bound
    with pytest.raises(ValueError, match="one per slice"):
        env.set_policy_network(inter, intras[:S - 1], intra_input=layout)
    with pytest.raises(ValueError, match="one per slice"):
        env.set_value_network(v_inter, v_intras + v_intras[:1])
    _bind(env, (inter, intras, v_inter, v_intras), layout, True)
    env.reset()
    rng = np.random.default_rng(6)
    other = make_net([n_in, 24, 3], act, 1)                                                  # another shape
    other_act = make_net([n_in] + list(widths) + [3], "tanh", 2)                             # another activation
    other_layout = make_net([n_in - Us] + list(widths) + [3], act, 3)                        # a valid "obs" net among "mask_obs" ones
    assert _raw_set(env, actor_call, intras, S - 1, n_in, 3, layout) == E_INVALID            # n != S
    assert _raw_set(env, actor_call, intras[:-1] + [other], S, n_in, 3, layout) == E_INVALID
    assert _raw_set(env, actor_call, intras[:-1] + [other_act], S, n_in, 3, layout) == E_INVALID
    assert env._lib.ranenv_set_intra_policy_networks(env._h, S, None, env._stream()) == E_INVALID
    # (a net of the other layout among the rest: its struct says "obs", its width is that layout's)
    from intent_radio_sched_multi_slice_amd.batched_env import NET_INPUTS, policy_net_layers
    keep = []
    structs = [env._mlp_struct(policy_net_layers(n)[0], act, NET_INPUTS[lay], keep) for n, lay in
               [(x, layout) for x in intras[:-1]] + [(other_layout, "obs")]]
    arr = (C.POINTER(type(structs[0])) * S)(*[C.pointer(m) for m in structs])
    assert env._lib.ranenv_set_intra_policy_networks(env._h, S, arr, env._stream()) == E_INVALID
    # critics: another layout than the actors', unequal shapes
    obs_critics = [make_net([n_in - Us] + list(widths) + [1], act, 10 + s) for s in range(S)]
    assert _raw_set(env, value_call, obs_critics, S, n_in - Us, 1, "obs") == E_INVALID
    assert _raw_set(env, value_call, v_intras[:-1] + [make_net([n_in, 24, 1], act, 4)], S, n_in, 1, layout) == E_INVALID
    assert _raw_set(env, value_call, v_intras, S + 1, n_in, 1, layout) == E_INVALID
    _step_and_check(env, rng, inter, intras, layout)                                         # the previous binding still acts
    rec = to_host(env.collect(2))
    ps.check_intra_values(rec["vf"][0], rec["obs_inter"][0], rec["obs_intra"][0], rec["mask_intra"][0], v_inter, v_intras, layout)
    env.close()


def test_a_refused_list_through_the_python_api_leaves_the_previous_binding_in_place():
    """A per-slice bind from Python is two library calls, and the first drops the previous set: a list the second would refuse -- nets
    of unequal hidden widths or activation, critics of the actors' other layout, critics with no intra actor -- raises ValueError before
    either call, and the nets bound before still act (actions and values against the twin)."""
    need_gpu()
    case = ps.CASES[1]
    S, Us, B, widths, act, layout = case
    n_in = ps.intra_width(Us, layout)
    inter, intras, v_inter, v_intras = ps.make_nets(*ps.TWIN_NETS[1])
    wl, env = _env(case, 98)
    with pytest.raises(ValueError, match="no intra actor is bound"):
        env.set_value_network(v_inter, v_intras)
    env.set_policy_network(inter, None, stochastic=True, seed=SEED)
    with pytest.raises(ValueError, match="no intra actor is bound"):
        env.set_value_network(v_inter, v_intras)
    _bind(env, (inter, intras, v_inter, v_intras), layout, True)
    env.reset()
    other_inter = ps.make_nets(case, 990)[0]
    for bad in (make_net([n_in, 24, 3], act, 1), make_net([n_in] + list(widths) + [3], "tanh", 2)):     # hidden widths, activation
        with pytest.raises(ValueError, match="differs from net 0"):
            env.set_policy_network(other_inter, intras[:-1] + [bad], stochastic=False, seed=1, intra_input=layout)
    with pytest.raises(ValueError, match="differs from net 0"):
        env.set_value_network(v_inter, v_intras[:-1] + [make_net([n_in, 24, 1], act, 4)])
    with pytest.raises(ValueError, match="the other layout"):
        env.set_value_network(v_inter, [make_net([n_in - Us] + list(widths) + [1], act, 10 + s) for s in range(S)])
    _step_and_check(env, np.random.default_rng(7), inter, intras, layout)
    rec = to_host(env.collect(2))
    ps.check_intra_values(rec["vf"][0], rec["obs_inter"][0], rec["obs_intra"][0], rec["mask_intra"][0], v_inter, v_intras, layout)
    env.close()


def test_a_shared_net_afterwards_and_unbinding():
    """set_policy_network with a shared net behind a per-slice set == a fresh env under that net; n = 0 unbinds: the shared net of the
    last set_policy_network stands again, and the per-slice critics go with the per-slice actors."""
    need_gpu()
    case = ps.CASES[0]
    S, Us, B, widths, act, layout = case
    n_in = ps.intra_width(Us, layout)
    inter, intras, v_inter, v_intras = ps.make_nets(case, 950)
    got = {}
    for how in ("fresh", "rebound", "unbound"):
        wl, env = _env(case, 99)
        if how == "fresh":
            env.set_policy_network(inter, intras[1], stochastic=True, seed=SEED, intra_input=layout)
            env.set_value_network(v_inter, v_intras[1])
        elif how == "rebound":
            _bind(env, (inter, intras, v_inter, v_intras), layout, True)
            env.set_policy_network(inter, intras[1], stochastic=True, seed=SEED, intra_input=layout)
            env.set_value_network(v_inter, v_intras[1])
        else:
            env.set_policy_network(inter, intras[1], stochastic=True, seed=SEED, intra_input=layout)
            env.set_value_network(v_inter, v_intras[1])
            assert _raw_set(env, "ranenv_set_intra_policy_networks", intras, S, n_in, 3, layout) == 0
            assert _raw_set(env, "ranenv_set_intra_value_networks", v_intras, S, n_in, 1, layout) == 0
            assert env._lib.ranenv_set_intra_policy_networks(env._h, 0, None, env._stream()) == 0
        env.reset()
        _inject(env, np.random.default_rng(8))
        rec = to_host(env.collect(3))
        got[how] = (rec, _actions(env))
        env.close()
    for how in ("rebound", "unbound"):
        for name in FIELDS:
            assert np.array_equal(got[how][0][name], got["fresh"][0][name]), (how, name)
        assert np.array_equal(got[how][1][0], got["fresh"][1][0]) and np.array_equal(got[how][1][1], got["fresh"][1][1]), how
    # per-slice actors bound through Python stand alone: unbinding them leaves no intra net at all
    wl, env = _env(case, 99)
    _bind(env, (inter, intras, v_inter, v_intras), layout, False)
    assert env.policy_actions()["intra"] is not None
    assert env._lib.ranenv_set_intra_value_networks(env._h, 0, None, env._stream()) == 0
    assert env._lib.ranenv_set_intra_policy_networks(env._h, 0, None, env._stream()) == 0
    env._policy_views = None
    assert env.policy_actions()["intra"] is None
    env.close()


@pytest.mark.parametrize("per_slice_between", [False, True], ids=["pair", "per-slice-between"])
@pytest.mark.parametrize("widths", [[40], [96, 7]], ids=["40", "96x7"])
def test_an_inter_critic_alone_behind_a_critic_pair(widths, per_slice_between):
    """set_value_network(v_inter2, None) behind a critic pair -- and behind per-slice critics bound in between -- leaves no intra critic:
    columns 1..S of the next record's vf are exactly 0, and the record is, bit for bit, that of a fresh env bound to (v_inter2, None)
    from the start and taken through the same two collect(2) calls.  B = 33: one full tile of 32 rows and a one-row tail."""
    need_gpu()
    case = (5, 5, 33, widths, "tanh", "obs")
    S = case[0]
    inter, intras, v_inter, v_intras = ps.make_nets(case, 990)
    v_inter2 = make_net([10 * S] + widths + [1], "tanh", 995)
    recs = {}
    for how in ("rebound", "fresh"):
        wl, env = _env(case, 101)
        env.set_policy_network(inter, intras[0], stochastic=True, seed=SEED, intra_input="obs")
        if how == "rebound":
            env.set_value_network(v_inter, v_intras[0])
        else:
            env.set_value_network(v_inter2, None)
        env.reset()
        first = to_host(env.collect(2))
        if how == "rebound":
            assert np.any(first["vf"][..., 1:] != 0.0)
            if per_slice_between:
                env.set_value_network(v_inter, v_intras)
            env.set_value_network(v_inter2, None)
        recs[how] = to_host(env.collect(2))
        env.close()
    assert np.all(recs["rebound"]["vf"][..., 1:] == 0.0)
    assert np.any(recs["rebound"]["vf"][..., 0] != 0.0) and np.any(recs["rebound"]["logp"][..., 1:] != 0.0)
    assert np.array_equal(recs["rebound"]["vf"][..., 0], recs["fresh"]["vf"][..., 0])
    for name in FIELDS:
        assert np.array_equal(recs["rebound"][name], recs["fresh"][name]), name


def test_rebind_larger_then_smaller_right_after_a_partitioned_rollout():
    """Per-slice sets re-bound behind partitioned rollouts without a host sync == the same sequence with syncs; the last, smaller set --
    copied in place over the larger one's buffer -- then acts as the twin says (stale weights or padding would show)."""
    need_gpu()
    S, Us, B = 5, 5, 70
    small, large = (S, Us, B, [40], "relu", "obs"), (S, Us, B, [512, 96], "relu", "obs")
    sets = [ps.make_nets(small, 960), ps.make_nets(large, 970), ps.make_nets(*ps.TWIN_NETS[-1])]
    out = []
    for sync in (False, True):
        wl, env = _env(small, 100)
        env.set_partitions(3)
        for i, nets in enumerate(sets):
            _bind(env, nets, "obs", True)
            if i == 0:
                env.reset()
            env.rollout(4)
            if sync:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        out.append([*_actions(env), env.obs_inter.cpu().numpy().copy(), env.reward.cpu().numpy().copy(),
                    env.views()["pkt_effective_thr"].cpu().numpy().copy()])
        if sync:
            _step_and_check(env, np.random.default_rng(9), sets[2][0], sets[2][1], "obs")
        env.close()
    for x, y in zip(*out):
        assert np.array_equal(x, y)
