"""The policy-network kernel (RANENV_POLICY_NETWORK) against the float64 reference of tests/policy_ref.py: hidden widths that
are not multiples of 32 or that take the other LDS stride, 1 to 4 hidden layers and mixed stacks, both activations on both nets,
both intra layouts, row tails of both launches, env ranges and partitions, the Philox keying of the noise, rebinding nets on one
handle, and a seeded fuzz of architectures and shapes whose actions drive an env checked against the CPU oracle.

Inputs of the forward tests are injected: distinct dense values on several scales are written into obs_inter / obs_intra before
the step (the nets read those buffers before the step overwrites them), so a row mix-up or a wrong weight column shows."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import policy_ref as pr
from tests.common import OBS_TOL, REW_TOL
from tests.gpu_common import GRID, make_inter_net, make_net, need_gpu
from tests.gpu_common import shaped_workload as _workload

pytestmark = pytest.mark.gpu

STATS = {"pairs": 0}          # (config, row) pairs compared, reported at the end of the module


def _layers(net):
    from intent_radio_sched_multi_slice_amd.batched_env import policy_net_layers
    return policy_net_layers(net)


def _nets(env, cfg, seed):
    S, Us, B, iw, ia, aw, aa, layout, st = cfg
    n_in = env.W + (env.Us if layout == "mask_obs" else 0)
    return make_inter_net(env.S, iw, ia, seed), make_net([n_in] + list(aw) + [3], aa, seed + 1)


def _snapshot(env):
    v = env.views()
    return {k: v[k].cpu().numpy().copy() for k in ("mask_inter", "mask_intra", "episode_number", "step_number")} | {
        "obs_inter": env.obs_inter.cpu().numpy().copy(), "obs_intra": env.obs_intra.cpu().numpy().copy()}


def _inject(env, rng):
    oi, oa = pr.injected_inputs(rng, env.B, env.S, env.Us)
    env.obs_inter.copy_(torch.from_numpy(oi))
    env.obs_intra.copy_(torch.from_numpy(oa))


def _ref(snap, inter, intra, stochastic, seed, layout, env_id_base=0):
    B = snap["obs_inter"].shape[0]
    return pr.PolicyRef(snap["obs_inter"], snap["mask_inter"], _layers(inter), snap["obs_intra"], snap["mask_intra"],
                        None if intra is None else _layers(intra), stochastic=stochastic, seed=seed, layout=layout,
                        env_ids=env_id_base + np.arange(B), episode=snap["episode_number"], step=snap["step_number"])


def _check(env, ref, rows=None, min_safe=0.9):
    pa = env.policy_actions()
    n = pr.check_actions(ref, pa["scores"].cpu(), None if pa["intra"] is None else pa["intra"].cpu(), rows=rows, min_safe=min_safe)
    STATS["pairs"] += (ref.B if rows is None else len(rows)) + n
    return n


# ---- injected-input forward over the grid -------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(GRID)))
def test_injected_forward_matches_float64(k):
    need_gpu()
    cfg = GRID[k]
    S, Us, B, iw, ia, aw, aa, layout, st = cfg
    wl = _workload(S, Us, B, seed=20 + k)
    env = wl.env
    inter, intra = _nets(env, cfg, 100 + k)
    seed = 0x9E37_79B9_7F4A_7C15 + k
    env.set_policy_network(inter, intra, stochastic=st, seed=seed, intra_input=layout)
    env.reset()
    rng = np.random.default_rng(k)
    checked, active, noisy = 0, np.zeros(S, dtype=bool), 0
    for t in range(2):
        _inject(env, rng)
        snap = _snapshot(env)
        env.step()
        ref = _ref(snap, inter, intra, st, seed, layout)
        checked += _check(env, ref)
        assert torch.equal(env.views()["policy_scores"].cpu(), env.policy_actions()["scores"].cpu())   # what the step read
        active |= ref.active.any(axis=0)
        if st:     # the noise (and so log_std) moves scores that the mean alone leaves inside (-1, 1)
            mean = np.clip(ref.out[:, :S], -1, 1)
            noisy += int((ref.active & (np.abs(ref.scores - mean) > 1e-2)).sum())
    assert checked >= 0.9 * 2 * B * S
    assert active.all(), "some sorted position was never unmasked"
    if st:
        assert noisy > 0
    env.close()


# ---- ranges and partitions against the reference -------------------------------------------------------------------------
CFG_RANGES = (5, 10, 100, [33, 96], "tanh", [160, 7], "relu", "mask_obs", True)
SEED_RANGES = 0xABCDEF0123


def _sentinel(env):
    pa = env.policy_actions()
    pa["scores"].fill_(7.0)
    pa["intra"].fill_(9)
    torch.cuda.synchronize()


def _outside_untouched(env, lo, hi):
    pa = env.policy_actions()
    sc, ic = pa["scores"].cpu().numpy(), pa["intra"].cpu().numpy()
    out = np.ones(env.B, dtype=bool)
    out[lo:hi] = False
    assert np.all(sc[out] == 7.0) and np.all(ic[out] == 9)


def test_partitioned_rollout_matches_float64():
    need_gpu()
    wl = _workload(*CFG_RANGES[:3], seed=31)
    env = wl.env
    inter, intra = _nets(env, CFG_RANGES, 7)
    env.set_policy_network(inter, intra, stochastic=True, seed=SEED_RANGES, intra_input="mask_obs")
    env.set_partitions(3)
    lo, n = C.c_int32(), C.c_int32()
    cuts = []
    for p in range(3):
        assert env._lib.ranenv_get_partition(env._h, p, C.byref(lo), C.byref(n)) == 0
        cuts.append(lo.value)
    assert any(c % 32 for c in cuts[1:]), cuts
    env.reset()
    rng = np.random.default_rng(3)
    for t in range(3):
        _inject(env, rng)
        snap = _snapshot(env)
        env.rollout(1)
        torch.cuda.synchronize()
        _check(env, _ref(snap, inter, intra, True, SEED_RANGES, "mask_obs"))
    env.close()


def test_ranges_step_async_and_step_range_match_float64():
    need_gpu()
    wl = _workload(*CFG_RANGES[:3], seed=32)
    env = wl.env
    inter, intra = _nets(env, CFG_RANGES, 8)
    env.set_policy_network(inter, intra, stochastic=True, seed=SEED_RANGES, intra_input="mask_obs")
    ranges = env.set_ranges(2)
    env.reset()
    rng = np.random.default_rng(4)
    for k, (lo, hi) in enumerate(ranges):
        _sentinel(env)
        _inject(env, rng)
        snap = _snapshot(env)
        env.step_async(k)
        env.step_wait(k)
        torch.cuda.synchronize()
        _check(env, _ref(snap, inter, intra, True, SEED_RANGES, "mask_obs"), rows=np.arange(lo, hi))
        _outside_untouched(env, lo, hi)
    # a direct ranenv_step_range from env 37 on
    lo, hi = 37, 81
    _sentinel(env)
    _inject(env, rng)
    snap = _snapshot(env)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert env._lib.ranenv_step_range(env._h, lo, hi - lo, None, None, None, None, *env._p_out, stream) == 0
    torch.cuda.synchronize()
    _check(env, _ref(snap, inter, intra, True, SEED_RANGES, "mask_obs"), rows=np.arange(lo, hi))
    _outside_untouched(env, lo, hi)
    env.close()


# ---- noise keying --------------------------------------------------------------------------------------------------------
def test_noise_keyed_by_env_id_base_and_far_episode_numbers():
    need_gpu()
    cfg = (5, 10, 33, [64], "tanh", [96], "tanh", "obs", True)
    B, first, base, seed = 33, 0x5A5A_0000, 1000, 0xFEDC_BA98_7654_3210
    wl = _workload(5, 10, B, max_steps=4, seed=33)
    env = wl.env
    inter, intra = _nets(env, cfg, 9)
    eps = env.episodes
    env.set_episode_table(scenario=np.arange(B) % 8, se_base=eps["se_base"], se_len=eps["se_len"], se_offset=eps["se_offset"],
                          trf_base=eps["trf_base"], trf_len=eps["trf_len"], trf_offset=eps["trf_offset"], first_episode=first)
    env.enable_autoreset(first, first + B, episode_numbers=first + np.arange(B))
    env.set_traffic_generator(77, env_id_base=base)
    env.set_policy_network(inter, intra, stochastic=True, seed=seed)
    env.reset()
    rng = np.random.default_rng(5)
    for t in range(6):          # across an episode end: the next episodes' numbers key the draws
        if t == 3:
            env.set_traffic_generator(77, env_id_base=5, enable=False)
            assert env.env_id_base == base and env.traffic_seed is None     # the handle keeps its base: so does Python
        _inject(env, rng)
        snap = _snapshot(env)
        assert snap["episode_number"].min() >= first
        env.step()
        _check(env, _ref(snap, inter, intra, True, seed, "obs", env_id_base=base))
        wrong = _ref(snap, inter, intra, True, seed, "obs", env_id_base=0)
        pa = env.policy_actions()["scores"].cpu().numpy()
        assert np.abs(pa - wrong.scores)[wrong.active].max() > 1e-2          # a base of 0 would show
    assert np.all(env.views()["episode_number"].cpu().numpy() != first + np.arange(B))    # every env moved on
    env.close()


# ---- rebinding nets on one handle -------------------------------------------------------------------------------------------
def test_rebind_in_place_inter_only_and_larger():
    need_gpu()
    from intent_radio_sched_multi_slice_amd import _lib
    S, Us, B = 10, 10, 33
    wl = _workload(S, Us, B, seed=34)
    env = wl.env
    rng = np.random.default_rng(6)
    seq = [((10, 10, B, [512] * 3, "relu", [512, 1, 512], "relu", "obs", False), True),
           ((10, 10, B, [33], "relu", [33], "tanh", "mask_obs", True), True),      # in place: stale padding must not leak
           ((10, 10, B, [96, 7], "tanh", [], "tanh", "obs", False), False),        # inter only, after an intra net
           ((10, 10, B, [512, 7, 512, 512], "relu", [512, 1, 512, 512], "relu", "obs", True), True)]  # > capacity: new buffer
    env.reset()
    for i, (cfg, with_intra) in enumerate(seq):
        inter, intra = _nets(env, cfg, 40 + i)
        if not with_intra:
            intra = None
        seed = 1234 + i
        env.set_policy_network(inter, intra, stochastic=cfg[8], seed=seed, intra_input=cfg[7], fixed_intra=_lib.INTRA_MT)
        for t in range(2):
            _inject(env, rng)
            snap = _snapshot(env)
            env.step()
            _check(env, _ref(snap, inter, intra, cfg[8], seed, cfg[7]))
        if not with_intra:
            assert env.policy_actions()["intra"] is None
    env.close()


def test_rebind_right_after_partitioned_rollout():
    """set_policy_network issued behind a partitioned rollout without a host sync == the same sequence with a sync."""
    need_gpu()
    cfg_a = (5, 10, 100, [512, 512], "tanh", [512, 33], "relu", "obs", True)
    cfg_b = (5, 10, 100, [33], "relu", [7], "tanh", "obs", True)
    out = []
    for sync in (False, True):
        wl = _workload(5, 10, 100, seed=35)
        env = wl.env
        a, b = _nets(env, cfg_a, 50), _nets(env, cfg_b, 60)
        env.set_policy_network(*a, stochastic=True, seed=3)
        env.set_partitions(3)
        env.reset()
        env.rollout(4)
        if sync:
            torch.cuda.synchronize()
        env.set_policy_network(*b, stochastic=True, seed=3)
        env.rollout(4)
        torch.cuda.synchronize()
        pa = env.policy_actions()
        out.append([pa["scores"].cpu(), pa["intra"].cpu(), env.obs_inter.cpu(), env.reward.cpu(),
                    env.views()["pkt_effective_thr"].cpu()])
        env.close()
    for x, y in zip(*out):
        assert torch.equal(x, y)


# ---- network-policy fuzz against the oracle -----------------------------------------------------------------------------
WIDTHS = [1, 7, 32, 33, 64, 96, 100, 160, 255, 256, 480, 511, 512]
N_FUZZ = 12


def _draw_net_case(k):
    rng = np.random.default_rng(7000 + k)
    S, Us = int(rng.integers(1, 17)), int(rng.integers(1, 17))
    U = int(rng.integers(max(2, Us, S), min(256, S * Us + 16) + 1))
    G = int(rng.choice([1, 1, 2, 3, 5]))
    R = max(G, int(rng.integers(G, 64)))

    def arch():
        depth = int(rng.integers(1, 5))
        w = [int(rng.choice(WIDTHS)) for _ in range(depth)]
        if depth >= 3 and sum(w) > 1100:           # (deep and wide at once: the rigorous bound gets loose)
            w = [min(x, 96) for x in w]
        return w
    how = ["steps", "rollout", "autoreset"][k % 3]
    return dict(S=S, Us=Us, U=U, G=G, R=R, inter=arch(), intra=arch(), ia=str(rng.choice(["tanh", "relu"])),
                aa=str(rng.choice(["tanh", "relu"])), layout=str(rng.choice(["obs", "mask_obs"])), stochastic=bool(rng.integers(0, 2)),
                how=how, parts=int(rng.integers(1, 4)), B=int(rng.choice([7, 33])), steps=10)


@pytest.mark.parametrize("k", range(N_FUZZ))
def test_network_policy_fuzz_vs_oracle(k):
    need_gpu()
    from oracle import pyoracle
    c = _draw_net_case(k)
    S, Us, B, steps = c["S"], c["Us"], c["B"], c["steps"]
    L = 4 if c["how"] == "autoreset" else 1000
    trace_len = 16
    wl = _workload(S, Us, B, max_steps=L, seed=60 + k, U=c["U"], R=c["R"], G=c["G"], trace_len=trace_len)
    env, tabs = wl.env, wl.tables
    cfg = (S, Us, B, c["inter"], c["ia"], c["intra"], c["aa"], c["layout"], c["stochastic"])
    inter, intra = _nets(env, cfg, 200 + k)
    seed = 0x1357_9BDF_2468_ACE0 + k
    env.set_policy_network(inter, intra, stochastic=c["stochastic"], seed=seed, intra_input=c["layout"])
    eps = env.episodes
    n_ep, first = 8, 0x0100_0000 + 97 * k
    ep_no = np.arange(n_ep)
    env.set_episode_table(scenario=ep_no % 8, se_base=(ep_no % 8) * trace_len, se_len=trace_len, se_offset=(ep_no * 5) % trace_len,
                          trf_base=(ep_no % 8) * trace_len, trf_len=trace_len, trf_offset=(ep_no * 3) % trace_len, first_episode=first)
    start = first + np.arange(B) % n_ep
    env.enable_autoreset(first, first + n_ep, episode_numbers=start)
    if c["how"] != "steps":
        env.set_partitions(c["parts"])
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
    ends = 0
    for t in range(steps):
        snap = _snapshot(env)
        if c["how"] == "steps":
            env.step()
        else:
            env.rollout(1)
        torch.cuda.synchronize()
        _check(env, _ref(snap, inter, intra, c["stochastic"], seed, c["layout"]), min_safe=0.5)   # (real observations: ties)
        pa = env.policy_actions()
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
    assert (ends > 0) == (c["how"] == "autoreset")
    env.close()


def test_zz_report_pairs():
    """Not a check: prints how many (config, row) pairs this module compared with the float64 reference."""
    need_gpu()
    print(f"\npolicy-network shapes: {STATS['pairs']} (config, row) pairs compared")
