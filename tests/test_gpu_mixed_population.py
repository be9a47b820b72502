"""Mixed populations on the device (ranenv_set_population_policy_mixed ..., the ranenv_policy_mixed_* kernels, ranenv_gae_pop_kernel):
members of differing depth, width and activation against one-net twins bit for bit, the mixed path against the uniform one on equal
shapes, launch ranges that cut members, collect with fused and split critics and its float64 bound, per-member gamma / lambda,
rebinding a member to another architecture, launch counts, and one closed loop against the CPU oracle.

Every comparison against a twin handle is exact: a mixed workgroup runs its member's rows through the source lines of the one-net
kernel.  S 3 / Us 4, B 70, members of 5 / 32 / 33 envs (less than a tile of 32 rows, a tile, a tile and one row); the shapes are
those of tests/mixed_population_ref.py."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import collect_ref as cr
from tests import mixed_population_ref as mx
from tests import policy_ref as pr
from tests import population_ref as pop
from tests.common import OBS_TOL, REW_TOL
from tests.gpu_common import need_gpu, to_host
from tests.test_gpu_policy_network import _episode_table
from tests.test_gpu_policy_network_shapes import _inject, _outside_untouched, _sentinel, _snapshot, _workload
from tests.test_gpu_population import FIELDS, _env, _same_on

pytestmark = pytest.mark.gpu

SEED = 0x2468_ACE0_1357_9BDF
MODES = [False, True]
FIRST = mx.FIRST


def _bind_mixed(env, nets, stochastic, with_critics=True, precision="f32", intra=True, actors="mixed", critics="mixed", first=FIRST):
    """The grouping with the members' nets; ``actors`` / ``critics`` "uniform": the lists go through the uniform entries (their nets
    then have one shape)"""
    inters, intras, v_inters, v_intras = nets
    env.set_population(first)
    env.set_policy_network(inters, intras if intra else None, stochastic=stochastic, seed=SEED, precision=precision, mixed=actors == "mixed")
    if with_critics:
        env.set_value_network(v_inters, v_intras if intra else None, precision=precision, mixed=critics == "mixed")


def _bind_one(env, nets, m, stochastic, with_critics=True, precision="f32", intra=True, m_critic=None):
    """Member m's nets as the one pair of the whole batch, through the one-net path"""
    inters, intras, v_inters, v_intras = nets
    env.set_policy_network(inters[m], intras[m] if intra else None, stochastic=stochastic, seed=SEED, precision=precision)
    if with_critics:
        k = m if m_critic is None else m_critic
        env.set_value_network(v_inters[k], v_intras[k] if intra else None, precision=precision)


def _actions(env):
    """(scores, intra choices) of the last policy launch on the host; without an intra net: an empty array of choices"""
    torch.cuda.synchronize()
    pa = env.policy_actions()
    return pa["scores"].cpu().numpy().copy(), (np.zeros((env.B, 0), dtype=np.uint8) if pa["intra"] is None else pa["intra"].cpu().numpy().copy())


def _step_and_rollout(env, rng_seed, n=12):
    """reset, a step on injected observations, rollout(n): {name: host array [B, ...]} of the step's actions and every view afterwards"""
    env.reset()
    _inject(env, np.random.default_rng(rng_seed))
    env.step()
    out = dict(zip(("step_scores", "step_intra"), _actions(env)))
    env.rollout(n)
    out.update({"view_" + k: x for k, x in to_host(env.views()).items()})
    out.update({"out_" + k: getattr(env, k).cpu().numpy().copy() for k in ("obs_inter", "obs_intra", "reward", "done")})
    return out


def _twins_differ_across_boundaries(twins, key="step_scores"):
    for m in range(len(FIRST) - 2):
        e = FIRST[m + 1]
        for b in (e - 1, e):
            assert not np.array_equal(twins[m][key][b], twins[m + 1][key][b]), (m, b)


# ---- 1. every member is its own one-net twin, bit for bit ------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision,stochastic,intra", [("mixed", p, st, ia) for p in ("f32", "bf16") for st in MODES for ia in (False, True)] +
                         [("wide", "f32", True, True), ("wide", "bf16", False, True)])
def test_members_equal_their_own_one_net_twins_bit_for_bit(name, precision, stochastic, intra):
    """Several step()s and rollout(12): actions of the first step and every view and output afterwards, member by member.  "wide":
    member 2 is [512] with relu beside tanh members -- LDS sized from the largest member, not member 0, and an activation per member."""
    need_gpu()
    nets = mx.make_nets(name, 3100)

    def run(bind):
        wl, env = _env(mx.CASE, 310)
        bind(env)
        out = _step_and_rollout(env, 31)
        for _ in range(3):
            env.step()
        out.update(zip(("late_scores", "late_intra"), _actions(env)))
        env.close()
        return out
    got = run(lambda env: _bind_mixed(env, nets, stochastic, with_critics=False, precision=precision, intra=intra))
    twins = [run(lambda env, m=m: _bind_one(env, nets, m, stochastic, with_critics=False, precision=precision, intra=intra)) for m in range(mx.G)]
    _twins_differ_across_boundaries(twins)
    if intra:
        assert any(not np.array_equal(twins[m]["step_intra"][FIRST[m + 1] - 1:FIRST[m + 1] + 1], twins[m + 1]["step_intra"][FIRST[m + 1] - 1:FIRST[m + 1] + 1])
                   for m in range(mx.G - 1))
    for m in range(mx.G):
        _same_on(got, twins[m], FIRST[m], FIRST[m + 1], (name, precision, m))


# ---- 2. the mixed path on equal shapes is the uniform path -----------------------------------------------------------------------
@pytest.mark.parametrize("case", ["c-G1", "a-S3-32", "b-G64"])
def test_a_mixed_bind_of_equal_shapes_equals_the_uniform_bind_bit_for_bit(case):
    """G = 1, 3 and 64 distinct nets of one shape: actions, views and a collect(2) record"""
    need_gpu()
    first = pop.CASES[case][2]
    nets = pop.make_nets(case, 3200)
    runs = []
    for how in ("uniform", "mixed"):
        wl, env = _env(case, 320)
        _bind_mixed(env, nets, True, actors=how, critics=how, first=first)
        out = _step_and_rollout(env, 32)
        out.update({"rec_" + k: np.moveaxis(x, 1, 0) for k, x in to_host(env.collect(2)).items()})
        if how == "mixed":
            assert env.population_net("inter", len(first) - 2) == {"hidden": [32], "dims": [30, 32, 6], "activation": "tanh", "extent": 2112, "used": 2112}
        runs.append(out)
        env.close()
    assert np.any(runs[0]["rec_vf"][:, -1, 1:] != 0.0)
    _same_on(runs[1], runs[0], 0, None, case)


# ---- 3. launch ranges that cut members -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("se_mode", ["stream", "gather"])
def test_partitions_and_ranges_that_cut_members_equal_the_step_loop(se_mode):
    """rollout(9) over 3 partitions (edges 24 / 48, inside members 1 and 2) and step_async over two ranges (edge 36, inside member 1)
    against the unpartitioned step() loop, stochastic, across episode ends (episodes of 4 TTIs)."""
    need_gpu()
    n = 9
    nets = mx.make_nets("mixed", 3300)
    keys = ("pkt_effective_thr", "dropped_pkts", "queue_pkts", "queue_age_sum", "rb_start", "rb_count", "step_number", "episode_number",
            "policy_scores", "mask_inter", "mask_intra")

    def make():
        wl, env = _env(mx.CASE, 330, max_steps=4, se_mode=se_mode)
        _bind_mixed(env, nets, True, with_critics=False)
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
    env.reset()
    env.rollout(n)
    _same_on(state(env), want, 0, None, ("partitions", se_mode))
    env.close()

    env = make()
    ranges = env.set_ranges(2)
    assert ranges == [(0, 36), (36, 70)] and pop.owner(FIRST, 36) == pop.owner(FIRST, 35) == 1
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


# ---- 4. collect ------------------------------------------------------------------------------------------------------------------
def _collect_nets(how, seed):
    """The members' nets of a collect case: "both" mixed actors and mixed critics; "critics" actors of ONE shape (member 1's) bound
    through the uniform entry beside mixed critics; "actors" the reverse"""
    nets = list(mx.make_nets("mixed", seed))
    same = mx.make_nets("mixed", seed, members=[1, 1, 1])
    if how == "critics":
        nets[0], nets[1] = same[0], same[1]
    if how == "actors":
        nets[2], nets[3] = same[2], same[3]
    return tuple(nets)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("how", ["both", "critics", "actors"])
def test_collect_records_per_member_what_the_members_twin_records(how, split):
    """collect(3) across episode ends (episodes of 2 TTIs), stochastic: every field of the record on member m's slice is what a twin
    bound to member m's nets alone records there, and vf stays inside the float64 bound of the member's own critics."""
    need_gpu()
    T = 3
    nets = _collect_nets(how, 3400)

    def make(bind):
        wl, env = _env(mx.CASE, 340, max_steps=2)
        bind(env)
        _episode_table(env)
        env.set_option("collect_split", split)
        env.reset()
        rec = to_host(env.collect(T))
        slices = env.population_slices() if env._population is not None else None
        env.close()
        return rec, slices
    got, slices = make(lambda env: _bind_mixed(env, nets, True, actors="uniform" if how == "critics" else "mixed",
                                               critics="uniform" if how == "actors" else "mixed"))
    assert set(FIELDS) <= set(got) and got["done"].any() and np.any(got["vf"][-1][:, 1:] != 0.0) and np.any(got["logp"][:, :, 1:] != 0.0)
    assert [(s.start, s.stop) for s in slices] == list(zip(FIRST[:-1], FIRST[1:]))
    twins = [make(lambda env, m=m: _bind_one(env, nets, m, True))[0] for m in range(mx.G)]
    for m in range(mx.G - 1):                # adjacent twins differ either side of the boundary
        e = FIRST[m + 1]
        for b in (e - 1, e):
            assert not np.array_equal(twins[m]["action_inter"][0, b], twins[m + 1]["action_inter"][0, b]), (m, b)
            assert not np.array_equal(twins[m]["vf"][0, b], twins[m + 1]["vf"][0, b]), (m, b)
    for m, (want, sl) in enumerate(zip(twins, slices)):
        for k in FIELDS:
            a, b = got[k][:, sl], want[k][:, sl]
            assert np.array_equal(a, b), (how, m, k, int((a != b).sum()))
        for t in range(T):                   # ... and the member's own critics in float64, on the recorded rows
            worst = cr.check_values(got["vf"][t][sl], got["obs_inter"][t][sl], got["obs_intra"][t][sl], got["mask_intra"][t][sl], nets[2][m], nets[3][m],
                                    what=f"{how} member {m} slot {t}")
            assert worst <= 1.0


# ---- 5. GAE per member -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ends", [False, True])
def test_gae_uses_every_members_own_gamma_and_lambda(ends):
    """collect(4) with per-member sequences: adv / vtarg of member m's slice equal adapters.gae on that slice under (gamma[m], lam[m])
    and the twin's collect under those scalars, bit for bit; gae() with sequences gives the same, scalars give what they gave before."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd.adapters import gae
    T = 4
    nets = mx.make_nets("mixed", 3500)

    def make(bind, **kw):
        wl, env = _env(mx.CASE, 350, max_steps=2 if ends else 1000)
        bind(env)
        _episode_table(env)
        env.reset()
        return env, to_host(env.collect(T, **kw))
    env, got = make(lambda env: _bind_mixed(env, nets, True), gamma=mx.GAMMA, lam=mx.LAM)
    assert bool(got["done"][:-1].any()) == ends
    slices = env.population_slices()
    want = mx.gae_ref(got["reward"], got["vf"], got["done"], FIRST, mx.GAMMA, mx.LAM)
    for m, sl in enumerate(slices):
        a, v = gae(got["reward"][:, sl], got["vf"][:, sl], got["done"][:, sl], mx.GAMMA[m], mx.LAM[m])
        assert np.array_equal(got["adv"][:, sl], a) and np.array_equal(got["vtarg"][:, sl], v), m
        assert not np.array_equal(a, gae(got["reward"][:, sl], got["vf"][:, sl], got["done"][:, sl], mx.GAMMA[(m + 1) % 3], mx.LAM[(m + 1) % 3])[0])
    assert np.array_equal(got["adv"], want[0]) and np.array_equal(got["vtarg"], want[1])
    # the stand-alone pass: sequences, a scalar beside a sequence, scalars
    dev = {k: torch.from_numpy(got[k]).to(env.device) for k in ("reward", "vf", "done")}
    adv, vtarg = (x.cpu().numpy() for x in env.gae(dev["reward"], dev["vf"], dev["done"], gamma=mx.GAMMA, lam=mx.LAM))
    assert np.array_equal(adv, got["adv"]) and np.array_equal(vtarg, got["vtarg"])
    adv, vtarg = (x.cpu().numpy() for x in env.gae(dev["reward"], dev["vf"], dev["done"], gamma=0.9, lam=mx.LAM))
    w = mx.gae_ref(got["reward"], got["vf"], got["done"], FIRST, [0.9] * 3, mx.LAM)
    assert np.array_equal(adv, w[0]) and np.array_equal(vtarg, w[1])
    adv, vtarg = (x.cpu().numpy() for x in env.gae(dev["reward"], dev["vf"], dev["done"], gamma=0.9, lam=0.8))
    w = gae(got["reward"], got["vf"], got["done"], 0.9, 0.8)
    assert np.array_equal(adv, w[0]) and np.array_equal(vtarg, w[1])
    # scalars after sequences: the members' pairs are switched off again
    rec = to_host(env.collect(T, gamma=0.9, lam=0.8))
    w = gae(rec["reward"], rec["vf"], rec["done"], 0.9, 0.8)
    assert np.array_equal(rec["adv"], w[0]) and np.array_equal(rec["vtarg"], w[1])
    env.close()
    for m, sl in enumerate(slices):          # the twin's collect with the member's scalars
        twin, rec = make(lambda e, m=m: _bind_one(e, nets, m, True), gamma=mx.GAMMA[m], lam=mx.LAM[m])
        twin.close()
        assert np.array_equal(rec["adv"][:, sl], got["adv"][:, sl]) and np.array_equal(rec["vtarg"][:, sl], got["vtarg"][:, sl]), m


# ---- 6. rebinding a member to another architecture -------------------------------------------------------------------------------
def test_a_member_rebound_to_another_architecture_and_one_that_does_not_fit():
    need_gpu()
    from intent_radio_sched_multi_slice_amd._lib import RanEnvError
    from intent_radio_sched_multi_slice_amd.batched_env import packed_net_floats
    from tests.gpu_common import make_inter_net, make_net
    nets = mx.make_nets("mixed", 3600)
    inters, intras, v_inters, v_intras = nets
    copy = mx.make_nets("mixed", 3650, members=[2, 2, 2])     # other weights of member 2's architecture (critics: [64, 40])
    new = tuple(x[0] for x in copy)
    after_nets = tuple(lst[:1] + [n] + lst[2:] for lst, n in zip(nets, new))

    def run(env):
        env.reset()
        _inject(env, np.random.default_rng(36))
        env.step()
        out = dict(zip(("step_scores", "step_intra"), _actions(env)))
        out.update({"rec_" + k: np.moveaxis(x, 1, 0) for k, x in to_host(env.collect(2)).items()})
        return out

    def pop_run(rebind):
        wl, env = _env(mx.CASE, 360)        # (a fresh env per run: a reset keeps the history windows)
        _bind_mixed(env, nets, True)
        env.reset()
        env.rollout(2)                      # (rebinding in place behind launches that read the buffer and the table, on the same stream)
        info = rebind(env)
        out = run(env)
        env.close()
        return out, info

    def rebind_1(env):
        assert env.population_net("inter", 1)["hidden"] == [64, 40] and env.population_net("v_inter", 1)["hidden"] == [24]
        env.set_population_member(1, inter=new[0], intra=new[1], v_inter=new[2], v_intra=new[3])
        return [env.population_net(r, m) for r in ("inter", "intra", "v_inter", "v_intra") for m in range(3)]

    def rebind_0_too_large(env):
        wide = make_inter_net(mx.S, [512], "tanh", 1)
        extent = env.population_net("inter", 0)["extent"]
        assert packed_net_floats(wide) > extent == packed_net_floats(inters[2])
        with pytest.raises(RanEnvError, match=f"{packed_net_floats(wide)} floats.*extent {extent}"):
            env.set_population_member(0, inter=wide)
        with pytest.raises(RanEnvError, match="inter value net.*extent"):      # every role is checked in front of the first copy: the actor that fits stays out
            env.set_population_member(0, inter=new[0], v_inter=make_net([10 * mx.S, 512, 1], "tanh", 2))
        return [env.population_net(r, 0) for r in ("inter", "v_inter")]
    before, _ = pop_run(lambda env: None)
    after, info = pop_run(rebind_1)
    refused, info0 = pop_run(rebind_0_too_large)
    # what the getter reports: the new shape on member 1, the others as bound
    assert [i["hidden"] for i in info[:3]] == [[24], [33, 32, 96, 32], [33, 32, 96, 32]] and [i["hidden"] for i in info[6:9]] == [[33, 32, 96, 32], [64, 40], [64, 40]]
    assert info[1]["used"] == info[2]["used"] == info[1]["extent"] and info[0]["used"] < info[0]["extent"] and info[1]["dims"] == [30, 33, 32, 96, 32, 6]
    assert [i["hidden"] for i in info0] == [[24], [33, 32, 96, 32]]
    lo, hi = FIRST[1], FIRST[2]
    wl, twin = _env(mx.CASE, 360)
    _bind_one(twin, nets, 1, True)
    twin.reset()
    twin.rollout(2)
    _bind_one(twin, after_nets, 1, True)
    want = run(twin)
    twin.close()
    assert not np.array_equal(before["step_scores"][lo:hi], after["step_scores"][lo:hi]) and not np.array_equal(before["rec_vf"][lo:hi], after["rec_vf"][lo:hi])
    _same_on(after, want, lo, hi, "member 1 on member 2's architecture")
    for m in (0, 2):
        _same_on(after, before, FIRST[m], FIRST[m + 1], ("untouched", m))
    _same_on(refused, before, 0, None, "a refused rebind changes nothing")


# ---- 7. launch counts ------------------------------------------------------------------------------------------------------------
def test_step_launches_are_those_of_a_uniform_population():
    need_gpu()
    counts = []
    for how in ("uniform", "mixed"):
        nets = mx.make_nets("mixed", 3700, members=[1, 1, 1] if how == "uniform" else None)
        wl, env = _env(mx.CASE, 370)
        _bind_mixed(env, nets, True, actors=how, critics=how)
        env.set_partitions(3)
        env.reset()
        for _ in range(2):
            env.step()
        env.rollout(5)
        env.collect(3)
        torch.cuda.synchronize()
        counts.append(env.step_launches())
        env.close()
    assert counts[0] == counts[1] and sum(counts[0].values()) > 0, counts


# ---- 8. against the CPU oracle ---------------------------------------------------------------------------------------------------
def test_env_driven_by_its_mixed_populations_actions_matches_the_oracle():
    """20 TTIs, episodes of 8, stochastic: every TTI's actions against the float64 twin of the members' own nets, and the oracle fed
    those actions stays with the device (integers exact, observations and rewards within OBS_TOL / REW_TOL), across the episode ends."""
    need_gpu()
    from oracle import pyoracle
    S, Us, B, L, steps, trace_len = mx.S, mx.US, FIRST[-1], 8, 20, 16
    wl = _workload(S, Us, B, max_steps=L, seed=98, trace_len=trace_len)
    env, tabs = wl.env, wl.tables
    nets = mx.make_nets("mixed", 3000)           # (the set whose share of decidable rows the CPU tests hold)
    env.set_population(FIRST)
    env.set_policy_network(nets[0], nets[1], stochastic=True, seed=SEED, mixed=True)
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
    ends, choices, checked = 0, set(), 0
    for t in range(steps):
        snap = _snapshot(env)
        env.step()
        sc, ic = _actions(env)
        checked += pr.check_actions(mx.policy_ref(snap, nets[0], nets[1], FIRST, True, SEED), sc, ic, min_safe=0.9)
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
    assert ends == 2 * B and len(choices) > S and checked >= 0.9 * steps * B * S
    env.close()
