"""Populations on the device (ranenv_set_population ..., the ranenv_policy_pop_* kernels): G copies of one net against the one-net
path bit for bit, distinct members against their own one-net twins bit for bit and against the float64 twin of
tests/population_ref.py, launch ranges that cut members, collect with fused and split critics, rebinding one member in place, one
closed loop against the CPU oracle, the binding rules of include/ranenv.h, and bf16 members.

Members of 5, 32 and 33 envs are less than a tile of 32 rows, a tile, a tile and one row; 64 members of one and two envs reach the
last lane of the kernel's member search; widths 48 and 40 are padded and take the other LDS row stride."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import policy_bf16_ref as bref
from tests import policy_ref as pr
from tests import population_ref as pop
from tests.common import OBS_TOL, REW_TOL
from tests.gpu_common import make_net, need_gpu, to_host
from tests.test_gpu_policy_network import _episode_table
from tests.test_gpu_policy_network_shapes import _inject, _outside_untouched, _sentinel, _snapshot, _workload

pytestmark = pytest.mark.gpu

SEED = 0x2468_ACE0_1357_9BDF
E_INVALID, E_STATE = -1, -3
MODES = [False, True]
FIELDS = ("obs_inter", "obs_intra", "mask_inter", "mask_intra", "action_inter", "action_intra", "logp", "vf", "reward", "done", "adv", "vtarg")
A_CASES = ["a-S3-32", "a-S5-48x40"]


def _env(name, seed, max_steps=1000, se_mode="stream"):
    S, Us, first = pop.CASES[name][:3]
    wl = _workload(S, Us, first[-1], max_steps=max_steps, seed=seed)
    wl.env.set_se_mode(se_mode)
    return wl, wl.env


def _bind_pop(env, name, nets, stochastic, actors=True, critics=True, with_critics=True, precision="f32", activation=None):
    """The case's grouping with the members' nets; ``actors`` / ``critics`` False: member 0's pair for all members instead"""
    inters, intras, v_inters, v_intras = nets
    layout = pop.CASES[name][5]
    env.set_population(pop.CASES[name][2])
    a = (inters, intras) if actors else (inters[0], intras[0])
    env.set_policy_network(*a, stochastic=stochastic, seed=SEED, intra_input=layout, precision=precision, activation=activation)
    if with_critics:
        v = (v_inters, v_intras) if critics else (v_inters[0], v_intras[0])
        env.set_value_network(*v, precision=precision, activation=activation)


def _bind_one(env, name, nets, m, stochastic, with_critics=True, precision="f32", activation=None, m_critic=None):
    """Member m's nets as the one pair of the whole batch (``m_critic``: another member's critics)"""
    inters, intras, v_inters, v_intras = nets
    env.set_policy_network(inters[m], intras[m], stochastic=stochastic, seed=SEED, intra_input=pop.CASES[name][5], precision=precision,
                           activation=activation)
    if with_critics:
        k = m if m_critic is None else m_critic
        env.set_value_network(v_inters[k], v_intras[k], precision=precision, activation=activation)


def _actions(env):
    torch.cuda.synchronize()
    pa = env.policy_actions()
    return pa["scores"].cpu().numpy().copy(), pa["intra"].cpu().numpy().copy()


def _step_and_rollout(env, rng_seed, n=12, inject=None):
    """reset, a step on injected observations, rollout(n): {name: host array [B, ...]} of the step's actions and every view afterwards"""
    env.reset()
    if inject is None:
        _inject(env, np.random.default_rng(rng_seed))
    else:
        inject(env)
    env.step()
    out = dict(zip(("step_scores", "step_intra"), _actions(env)))
    env.rollout(n)
    out.update({"view_" + k: x for k, x in to_host(env.views()).items()})
    out.update({"out_" + k: getattr(env, k).cpu().numpy().copy() for k in ("obs_inter", "obs_intra", "reward", "done")})
    return out


def _same_on(got, want, lo, hi, what):
    for k, x in want.items():
        assert np.array_equal(got[k][lo:hi], x[lo:hi]), (what, k, int((got[k][lo:hi] != x[lo:hi]).sum()))


def _members_equal_their_twins(name, nets, stochastic, seed, precision="f32", activation=None, inject=None):
    """The population's step actions and the views after rollout(12), member by member, against a twin env bound to that member's
    nets alone (a fresh one per member: a reset keeps the history windows) -- after the twins of adjacent members were seen to differ
    on the envs either side of every boundary."""
    first = pop.CASES[name][2]
    G = len(first) - 1
    wl, env = _env(name, seed)
    _bind_pop(env, name, nets, stochastic, with_critics=False, precision=precision, activation=activation)
    got = _step_and_rollout(env, seed, inject=inject)
    env.close()
    twins = []
    for m in range(G):
        wl, twin = _env(name, seed)
        _bind_one(twin, name, nets, m, stochastic, with_critics=False, precision=precision, activation=activation)
        twins.append(_step_and_rollout(twin, seed, inject=inject))
        twin.close()
    for m in range(G - 1):
        e = first[m + 1]
        for b in (e - 1, e):
            assert not np.array_equal(twins[m]["step_scores"][b], twins[m + 1]["step_scores"][b]), (m, b)
    if G > 1:
        assert any(not np.array_equal(twins[m]["step_intra"][first[m + 1] - 1:first[m + 1] + 1], twins[m + 1]["step_intra"][first[m + 1] - 1:first[m + 1] + 1])
                   for m in range(G - 1))
    for m in range(G):
        _same_on(got, twins[m], first[m], first[m + 1], (name, m))


# ---- 1. copies of one net are the one-net path, bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("stochastic", MODES)
@pytest.mark.parametrize("name", list(pop.CASES))
def test_copies_of_one_net_are_the_one_net_path_bit_for_bit(name, stochastic):
    need_gpu()
    G = len(pop.CASES[name][2]) - 1
    nets = tuple([x[0]] * G for x in pop.make_nets(name, 1700))
    runs = []
    for population in (False, True):
        wl, env = _env(name, 170)
        if population:
            _bind_pop(env, name, nets, stochastic, with_critics=False)
            assert env.population().tolist() == pop.CASES[name][2]
        else:
            _bind_one(env, name, nets, 0, stochastic, with_critics=False)
        runs.append(_step_and_rollout(env, 17))
        env.close()
    assert len([k for k in runs[0] if k.startswith("view_")]) >= 18 and np.any(runs[0]["step_intra"] != runs[0]["step_intra"][0, 0])
    _same_on(runs[1], runs[0], 0, None, name)


# ---- 2. distinct members are their own one-net twins, bit for bit ---------------------------------------------------------------
@pytest.mark.parametrize("name,stochastic", [(n, st) for n in A_CASES for st in MODES] + [("b-G64", True)])
def test_distinct_members_equal_their_own_one_net_twins_bit_for_bit(name, stochastic):
    """(the 64 members' twins are 64 envs: once, stochastic -- the deterministic epilogue is the same map)"""
    need_gpu()
    _members_equal_their_twins(name, pop.make_nets(name, 1800), stochastic, 180)


# ---- 3. against the float64 twin ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stochastic", MODES)
@pytest.mark.parametrize("k", range(len(pop.TWIN_NETS)), ids=[n for n, _ in pop.TWIN_NETS])
def test_distinct_members_match_the_float64_twin(k, stochastic):
    need_gpu()
    name, seed = pop.TWIN_NETS[k]
    S, Us, first, widths, act, layout = pop.CASES[name]
    nets = pop.make_nets(name, seed)
    wl, env = _env(name, 190 + k)
    _bind_pop(env, name, nets, stochastic, with_critics=False)
    env.reset()
    rng = np.random.default_rng(30 + k)
    checked = 0
    for t in range(2):
        _inject(env, rng)
        snap = _snapshot(env)
        env.step()
        sc, ic = _actions(env)
        checked += pr.check_actions(pop.policy_ref(snap, nets[0], nets[1], first, stochastic, SEED, layout), sc, ic, min_safe=0.9)
    assert checked >= 0.9 * 2 * first[-1] * S
    env.close()


# ---- 4. launch ranges that cut members -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("se_mode", ["stream", "gather"])
def test_partitions_and_ranges_that_cut_members_equal_the_step_loop(se_mode):
    """B 70 under members of 5 / 32 / 33: rollout(9) over 3 partitions (edges 24 / 48, inside members 1 and 2) and step_async over two
    ranges (edge 36, inside member 1) against the unpartitioned step() loop, stochastic, across episode ends (episodes of 4 TTIs): actions
    TTI by TTI for the ranges -- a range's launch leaves the other range's actions alone --, actions, outputs and views at the end."""
    need_gpu()
    name, n = "a-S5-48x40", 9
    nets = pop.make_nets(name, 1900)
    keys = ("pkt_effective_thr", "dropped_pkts", "queue_pkts", "queue_age_sum", "rb_start", "rb_count", "step_number", "episode_number",
            "policy_scores", "mask_inter", "mask_intra")

    def make():
        wl, env = _env(name, 195, max_steps=4, se_mode=se_mode)
        _bind_pop(env, name, nets, True, with_critics=False)
        _episode_table(env)
        return env

    def state(env):
        out = dict(zip(("scores", "intra"), _actions(env)))
        out.update({k: env.views()[k].cpu().numpy().copy() for k in keys})
        out.update({k: getattr(env, k).cpu().numpy().copy() for k in ("obs_inter", "obs_intra", "reward", "done")})
        return out

    ref = make()
    ref.reset()
    per_tti = []
    for _ in range(n):
        ref.step()
        per_tti.append(_actions(ref))
    want = state(ref)
    assert np.all(want["step_number"] == n % 4)
    ref.close()

    env = make()
    env.set_partitions(3)
    lo, cnt = C.c_int32(), C.c_int32()
    edges = []
    for k in range(3):
        assert env._lib.ranenv_get_partition(env._h, k, C.byref(lo), C.byref(cnt)) == 0
        edges.append(lo.value)
    assert edges == [0, 24, 48] and pop.owner(pop.FIRST_A, np.array(edges)).tolist() == [0, 1, 2] and not set(edges[1:]) & set(pop.FIRST_A)
    env.reset()
    env.rollout(n)
    _same_on(state(env), want, 0, None, ("partitions", se_mode))
    env.close()

    env = make()
    ranges = env.set_ranges(2)
    assert ranges == [(0, 36), (36, 70)] and ranges[0][1] % 32 != 0 and pop.owner(pop.FIRST_A, 36) == pop.owner(pop.FIRST_A, 35) == 1
    env.reset()
    for t in range(n):
        for r, (a, b) in enumerate(ranges):
            _sentinel(env)
            env.step_async(r)
            env.step_wait(r)
            torch.cuda.synchronize()
            _outside_untouched(env, a, b)
            got = _actions(env)
            assert np.array_equal(got[0][a:b], per_tti[t][0][a:b]) and np.array_equal(got[1][a:b], per_tti[t][1][a:b]), (t, r)
    got = state(env)
    for k in keys + ("obs_inter", "obs_intra", "reward", "done"):
        if k != "policy_scores":             # (the step read the ranges' scores; the sentinel fill overwrote the buffer between them)
            assert np.array_equal(got[k], want[k]), ("ranges", se_mode, k)
    env.close()


# ---- 5. collect ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts,split,how", [(1, -1, "both"), (3, 0, "both"), (3, 1, "both"), (1, -1, "actors"), (3, 1, "actors"),
                                             (1, -1, "critics"), (3, 1, "critics")])
def test_collect_records_per_member_what_the_members_twin_records(parts, split, how):
    """collect(3) across episode ends (episodes of 2 TTIs), stochastic: every field of the record on member m's envs -- observations,
    masks, actions, logp, vf with the bootstrap slot, reward, done, adv, vtarg -- is what a twin bound to member m's nets alone records
    there.  how "actors": population actors with member 0's critic pair for all; "critics": member 0's actors with population critics."""
    need_gpu()
    name, T = "a-S5-48x40", 3
    first = pop.CASES[name][2]
    nets = pop.make_nets(name, 2000)

    def make(bind):
        wl, env = _env(name, 200, max_steps=2)
        bind(env)
        _episode_table(env)
        if parts > 1:
            env.set_partitions(parts)
        env.set_option("collect_split", split)
        env.reset()
        rec = to_host(env.collect(T))
        env.close()
        return rec
    got = make(lambda env: _bind_pop(env, name, nets, True, actors=how != "critics", critics=how != "actors"))
    assert set(FIELDS) <= set(got) and got["done"].any() and np.any(got["vf"][-1][:, 1:] != 0.0) and np.any(got["logp"][:, :, 1:] != 0.0)
    twins = [make(lambda env, m=m: _bind_one(env, name, nets, 0 if how == "critics" else m, True, m_critic=0 if how == "actors" else m))
             for m in range(len(first) - 1)]
    for m in range(len(first) - 2):          # adjacent twins differ either side of the boundary, in what `how` varies
        e = first[m + 1]
        for b in (e - 1, e):
            if how != "critics":
                assert not np.array_equal(twins[m]["action_inter"][0, b], twins[m + 1]["action_inter"][0, b]), (m, b)
            if how != "actors":
                assert not np.array_equal(twins[m]["vf"][0, b], twins[m + 1]["vf"][0, b]), (m, b)
    for m, want in enumerate(twins):
        for k in FIELDS:
            a, b = got[k][:, first[m]:first[m + 1]], want[k][:, first[m]:first[m + 1]]
            assert np.array_equal(a, b), (how, m, k, int((a != b).sum()))


# ---- 6. one member rebound in place ---------------------------------------------------------------------------------------------
def test_set_population_member_rebinds_one_member_and_touches_no_other():
    need_gpu()
    name = "a-S5-48x40"
    first = pop.CASES[name][2]
    nets = pop.make_nets(name, 2100)
    inters, intras, v_inters, v_intras = nets

    def run(env):
        env.reset()
        _inject(env, np.random.default_rng(21))
        env.step()
        out = dict(zip(("step_scores", "step_intra"), _actions(env)))
        out.update({"rec_" + k: x for k, x in to_host(env.collect(2)).items()})
        return {k: (x if not k.startswith("rec_") else np.moveaxis(x, 1, 0)) for k, x in out.items()}       # (env-major, for _same_on)

    def pop_run(rebind):
        wl, env = _env(name, 210)           # (a fresh env per run: a reset keeps the history windows)
        _bind_pop(env, name, nets, True)
        env.reset()
        env.rollout(2)                      # (rebinding in place behind launches that read the buffer, on the same stream)
        rebind(env)
        out = run(env)
        env.close()
        return out

    def twin_run(bind):
        wl, twin = _env(name, 210)
        _bind_one(twin, name, nets, 1, True)
        twin.reset()
        twin.rollout(2)
        bind(twin)
        out = run(twin)
        twin.close()
        return out
    before = pop_run(lambda env: None)
    after = pop_run(lambda env: env.set_population_member(1, inter=inters[2], intra=intras[2], v_inter=v_inters[2], v_intra=v_intras[2]))
    third = pop_run(lambda env: env.set_population_member(1, v_inter=v_inters[0]))            # one role alone: the others stay
    want = twin_run(lambda twin: _bind_one(twin, name, nets, 2, True))
    want3 = twin_run(lambda twin: twin.set_value_network(v_inters[0], v_intras[1]))
    lo, hi = first[1], first[2]
    assert not np.array_equal(before["step_scores"][lo:hi], after["step_scores"][lo:hi])
    assert not np.array_equal(before["rec_vf"][lo:hi], after["rec_vf"][lo:hi])
    _same_on(after, want, lo, hi, "member 1 is member 2's twin")
    _same_on(third, want3, lo, hi, "member 1 with member 0's inter critic")
    assert not np.array_equal(third["rec_vf"][lo:hi, :, 0], before["rec_vf"][lo:hi, :, 0]) and np.array_equal(third["rec_vf"][lo:hi, :-1, 1:], before["rec_vf"][lo:hi, :-1, 1:])
    for m in (0, 2):
        _same_on(after, before, first[m], first[m + 1], ("untouched", m))
        _same_on(third, before, first[m], first[m + 1], ("untouched", m))


# ---- 7. against the CPU oracle --------------------------------------------------------------------------------------------------
def test_env_driven_by_its_population_actions_matches_the_oracle():
    """20 TTIs, episodes of 8, members of 2 / 3 / 2 envs: the oracle fed the device's own scores and intra choices stays with the device
    (integers exact, observations and rewards within OBS_TOL / REW_TOL), across the episode ends."""
    need_gpu()
    from oracle import pyoracle
    S, Us, B, L, steps, trace_len = 3, 4, 7, 8, 20, 16
    wl = _workload(S, Us, B, max_steps=L, seed=97, trace_len=trace_len)
    env, tabs = wl.env, wl.tables
    inters, intras, _, _ = pop.make_member_nets(S, Us, 3, [32], "tanh", "obs", 2200)
    env.set_population(sizes=[2, 3, 2])
    env.set_policy_network(inters, intras, stochastic=True, seed=SEED)
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
    assert ends == 2 * B and len(choices) > S
    env.close()


# ---- 8. binding rules ------------------------------------------------------------------------------------------------------------
def _mlp_array(env, nets, in_dim, out_dim, layout, precision="f32", keep=None):
    from intent_radio_sched_multi_slice_amd.batched_env import NET_INPUTS, policy_net_layers
    structs = []
    for i, net in enumerate(nets):
        layers, act = policy_net_layers(net, None, in_dim, out_dim)
        structs.append(env._mlp_struct(layers, act, NET_INPUTS[layout], keep, precision[i] if isinstance(precision, list) else precision))
    keep += structs
    return (C.POINTER(type(structs[0])) * len(structs))(*[C.pointer(m) for m in structs])


def test_refused_calls_leave_the_previous_binding_acting():
    need_gpu()
    name, seed = pop.TWIN_NETS[1]
    S, Us, first, widths, act, layout = pop.CASES[name]
    G, n_in = len(first) - 1, pop.intra_width(Us, layout)
    nets = pop.make_nets(name, seed)
    inters, intras, v_inters, v_intras = nets
    wl, env = _env(name, 220)
    lib, h, keep = env._lib, env._h, []
    ia, aa = _mlp_array(env, inters, 10 * S, 2 * S, "obs", keep=keep), _mlp_array(env, intras, n_in, 3, layout, keep=keep)
    tab = lambda t: (C.c_int32 * len(t))(*t)  # noqa: E731
    # no population yet; tables that are none
    assert lib.ranenv_set_population_policy(h, G, ia, aa, 1, SEED, env._stream()) == E_STATE
    for bad in ([0, 5, 5, 70], [0, 37, 5, 70], [1, 5, 70], [0, 5, 69], [0, 5, 71]):
        assert lib.ranenv_set_population(h, len(bad) - 1, tab(bad)) == E_INVALID, bad
    assert lib.ranenv_set_population(h, 0, tab([0])) == E_INVALID and lib.ranenv_set_population(h, 65, tab(list(range(66)))) == E_INVALID
    assert lib.ranenv_set_population(h, 3, None) == E_INVALID
    assert env.population() is None
    _bind_pop(env, name, nets, True)
    env.reset()
    # the per-slice calls under a bound population, a grouping change under bound nets (the same table again is none)
    for call, arr in (("ranenv_set_intra_policy_networks", _mlp_array(env, intras[:1] * S, n_in, 3, layout, keep=keep)),
                      ("ranenv_set_intra_value_networks", _mlp_array(env, v_intras[:1] * S, n_in, 1, layout, keep=keep))):
        assert getattr(lib, call)(h, S, arr, env._stream()) == E_STATE, call
    assert lib.ranenv_set_population(h, 2, tab([0, 35, 70])) == E_STATE
    assert lib.ranenv_set_population(h, 3, tab(first)) == 0
    # n, shapes, precision, member index
    other = make_net([10 * S, 24, 2 * S], act, 1)
    assert lib.ranenv_set_population_policy(h, G - 1, ia, aa, 1, SEED, env._stream()) == E_INVALID
    assert lib.ranenv_set_population_value(h, G + 1, _mlp_array(env, v_inters, 10 * S, 1, "obs", keep=keep), None, env._stream()) == E_INVALID
    assert lib.ranenv_set_population_policy(h, G, _mlp_array(env, inters[:2] + [other], 10 * S, 2 * S, "obs", keep=keep), aa, 1, SEED, env._stream()) == E_INVALID
    assert lib.ranenv_set_population_policy(h, G, _mlp_array(env, inters, 10 * S, 2 * S, "obs", ["f32", "f32", "bf16"], keep=keep), aa, 1, SEED,
                                            env._stream()) == E_INVALID
    assert lib.ranenv_set_population_policy(h, G, ia, _mlp_array(env, intras, n_in, 3, layout, ["f32", "bf16", "f32"], keep=keep), 1, SEED,
                                            env._stream()) == E_INVALID
    assert lib.ranenv_set_population_policy(h, G, None, aa, 1, SEED, env._stream()) == E_INVALID
    one = _mlp_array(env, [inters[0], other], 10 * S, 2 * S, "obs", keep=keep)
    for m in (-1, G):
        assert lib.ranenv_set_population_member(h, m, one[0], None, None, None, env._stream()) == E_INVALID
    assert lib.ranenv_set_population_member(h, 1, one[1], None, None, None, env._stream()) == E_INVALID               # another shape
    assert lib.ranenv_set_population_member(h, 1, _mlp_array(env, inters[:1], 10 * S, 2 * S, "obs", "bf16", keep=keep)[0], None, None, None,
                                            env._stream()) == E_INVALID                                               # another precision
    torch.cuda.synchronize()
    env._policy_views = None
    # the previous binding still acts: the members' nets, against the float64 twin
    _inject(env, np.random.default_rng(22))
    snap = _snapshot(env)
    env.step()
    sc, ic = _actions(env)
    pr.check_actions(pop.policy_ref(snap, inters, intras, first, True, SEED, layout), sc, ic, min_safe=0.9)
    # a plain set_policy_network afterwards unbinds the population's actors AND critics -- the grouping stays -- and is the one-net path
    # bit for bit: slot 0 of collect(1) on injected observations (what does not depend on the history the steps above left) against a
    # fresh env through the same two resets
    from intent_radio_sched_multi_slice_amd._lib import RanEnvError
    env.set_policy_network(inters[1], intras[1], stochastic=True, seed=SEED, intra_input=layout)
    assert env.population().tolist() == first
    with pytest.raises(RanEnvError, match="no value network bound"):
        env.collect(1)
    runs = []
    for fresh in (False, True):
        if fresh:
            env.close()
            wl, env = _env(name, 220)
            env.reset()
        _bind_one(env, name, nets, 1, True)
        env.reset()
        _inject(env, np.random.default_rng(23))
        rec = to_host(env.collect(1))
        runs.append({k: rec[k][0] for k in ("obs_inter", "obs_intra", "mask_inter", "mask_intra", "action_inter", "action_intra", "logp", "vf")})
    assert np.any(runs[0]["vf"][:, 1:] != 0.0)
    _same_on(runs[0], runs[1], 0, None, "plain afterwards")
    env.close()


def test_removing_the_grouping_unbinds_the_populations_nets():
    need_gpu()
    name = "a-S3-32"
    nets = pop.make_nets(name, 2300)
    wl, env = _env(name, 230)
    _bind_pop(env, name, nets, False)
    assert [(s.start, s.stop) for s in env.population_slices()] == [(0, 5), (5, 37), (37, 70)]
    env.reset()
    env.step()
    env.set_population()
    assert env.population() is None
    from intent_radio_sched_multi_slice_amd._lib import RanEnvError
    with pytest.raises(RanEnvError, match="no policy network bound"):
        env.step()
    env.close()


# ---- 9. bf16 members ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", A_CASES)
def test_bf16_copies_of_one_net_are_the_one_net_path_bit_for_bit(name):
    need_gpu()
    G = len(pop.CASES[name][2]) - 1
    nets = tuple([x[0]] * G for x in pop.make_nets(name, 2400))
    runs = []
    for population in (False, True):
        wl, env = _env(name, 240)
        (_bind_pop if population else lambda e, n, x, st, **kw: _bind_one(e, n, x, 0, st, **kw))(env, name, nets, True, precision="bf16")
        out = _step_and_rollout(env, 24)
        out.update({"rec_" + k: np.moveaxis(x, 1, 0) for k, x in to_host(env.collect(2)).items()})
        runs.append(out)
        env.close()
    _same_on(runs[1], runs[0], 0, None, name)
    wl, env = _env(name, 240)                      # (... and bf16 is not f32: the precision reached the members' copies)
    _bind_pop(env, name, nets, True, with_critics=False)
    assert not np.array_equal(_step_and_rollout(env, 24)["step_scores"], runs[0]["step_scores"])
    env.close()


def test_bf16_members_of_integer_valued_nets_equal_their_twins_and_the_exact_forward():
    """Members of policy_bf16_ref's exact nets (every summation order reproduces them) on 0 / 1 observations: bit for bit their one-net
    twins, and the deterministic scores of the step exactly the float64 forward of the env's own member."""
    need_gpu()
    name = "a-S5-48x40"
    S, Us, first, _, _, layout = pop.CASES[name]
    G = len(first) - 1
    sets = [bref.exact_case_nets("33", S, Us, layout, 2500 + 10 * m) for m in range(G)]
    nets = tuple([sets[m][r] for m in range(G)] for r in range(4))
    oi, oa = bref.exact_inputs(np.random.default_rng(25), first[-1], S, Us)

    def inject(env):
        env.obs_inter.copy_(torch.from_numpy(oi))
        env.obs_intra.copy_(torch.from_numpy(oa))
    _members_equal_their_twins(name, nets, False, 250, precision="bf16", activation="relu", inject=inject)
    wl, env = _env(name, 250)
    _bind_pop(env, name, nets, False, with_critics=False, precision="bf16", activation="relu")
    env.reset()
    inject(env)
    active = pr.sorted_mask(env.views()["mask_inter"].cpu().numpy())
    env.step()
    sc, _ = _actions(env)
    for m in range(G):
        lo, hi = first[m], first[m + 1]
        want = np.where(active[lo:hi], np.clip(bref.exact_forward(oi[lo:hi], nets[0][m])[:, :S], -1.0, 1.0), -1.0)
        assert np.array_equal(sc[lo:hi], want), m
    env.close()
