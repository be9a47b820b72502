"""PPO sample collection on the device (ranenv_collect, include/ranenv.h): the record against a step() loop, the rest of the handle
against rollout(), log-probabilities and values against the float64 reference of tests/collect_ref.py, GAE against adapters.gae
exactly, determinism, error paths, NULL fields."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import collect_ref as cr
from tests.gpu_common import LOOSE_WIN_SENT_AND_SE, assert_same_state, need_gpu, to_host

pytestmark = pytest.mark.gpu

T = 24
FIELDS = ("obs_inter", "obs_intra", "mask_inter", "mask_intra", "action_inter", "action_intra", "logp", "vf", "reward", "done", "adv", "vtarg")


def _layout(size):
    return "mask_obs" if size == "S5U25" else "obs"


@pytest.mark.parametrize("se_mode", ["stream", "gather"])
@pytest.mark.parametrize("autoreset", [False, True])
@pytest.mark.parametrize("stochastic", [False, True])
@pytest.mark.parametrize("size", list(cr.SIZES))
@pytest.mark.parametrize("net", list(cr.NETS))
def test_record_is_the_step_loop(net, size, stochastic, autoreset, se_mode):
    """collect(T) over 1 and 3 partitions records, TTI by TTI, what a step() loop on a twin env sees: observations and masks before
    the step, the actions it consumed, its reward and done -- bit for bit, every row."""
    need_gpu()
    B = 48
    kw = dict(stochastic=stochastic, autoreset=autoreset, se_mode=se_mode, intra_input=_layout(size))
    _, ref, _ = cr.make_env(size, net, B, **kw)
    want = {k: [] for k in ("obs_inter", "obs_intra", "mask_inter", "mask_intra", "scores", "action_intra", "reward", "done")}
    v = ref.views()
    for _ in range(T):
        for k, x in (("obs_inter", ref.obs_inter), ("obs_intra", ref.obs_intra), ("mask_inter", v["mask_inter"]), ("mask_intra", v["mask_intra"])):
            want[k].append(x.clone())
        ref.step()
        pa = ref.policy_actions()
        for k, x in (("scores", pa["scores"]), ("action_intra", pa["intra"]), ("reward", ref.reward), ("done", ref.done)):
            want[k].append(x.clone())
    want = {k: torch.stack(x) for k, x in want.items()}
    if autoreset:      # the case is what it claims: ends at different TTIs in different envs, several at the call's last TTI
        d = want["done"].cpu().numpy()
        assert d[-1].any() and not d[-1].all() and len({int(np.argmax(d[:, b])) for b in range(B) if d[:, b].any()}) >= 4
    for parts in (1, 3):
        _, env, _ = cr.make_env(size, net, B, parts=parts, **kw)
        rec = env.collect(T)
        torch.cuda.synchronize()
        for k in ("obs_inter", "obs_intra", "mask_inter", "mask_intra", "action_intra", "reward", "done"):
            assert rec[k].shape == want[k].shape, k
            assert torch.equal(rec[k], want[k]), (k, parts, int((rec[k] != want[k]).sum()))
        assert torch.equal(rec["action_inter"].clamp(-1.0, 1.0), want["scores"]), parts
        env.close()
    ref.close()


@pytest.mark.parametrize("autoreset", [False, True])
@pytest.mark.parametrize("size", list(cr.SIZES))
@pytest.mark.parametrize("net", list(cr.NETS))
def test_nothing_else_moved(net, size, autoreset):
    """After collect(T): every view, the caller's outputs and policy_actions() are those after rollout(T) on the twin; one more
    step() on both keeps them equal (the host's shadow of the step counters and the done buffer it belongs to)."""
    need_gpu()
    B = 48
    for parts in (1, 3):
        kw = dict(stochastic=True, autoreset=autoreset, parts=parts, intra_input=_layout(size))
        wl, a, _ = cr.make_env(size, net, B, **kw)
        _, b, _ = cr.make_env(size, net, B, **kw)
        a.collect(T)
        b.rollout(T)
        for extra in (0, 1):
            if extra:
                a.step()
                b.step()
            assert_same_state(a, b, wl.tables, (parts, extra), loose=LOOSE_WIN_SENT_AND_SE, actions=("scores", "intra"))
        a.close()
        b.close()


@pytest.mark.parametrize("stochastic", [False, True])
@pytest.mark.parametrize("size", list(cr.SIZES))
@pytest.mark.parametrize("net", list(cr.NETS))
def test_logp_and_values_within_the_float64_bounds(net, size, stochastic):
    """Every slot's vf, logp and unclamped action_inter against the float64 nets on the RECORDED observations (bounds: collect_ref);
    vf[T] against the critics on the observation buffers as they stand after the call."""
    need_gpu()
    B, seed = 64, 0x1234_5678_9ABC
    layout = _layout(size)
    _, env, (a_inter, a_intra, v_inter, v_intra) = cr.make_env(size, net, B, stochastic=stochastic, seed=seed, intra_input=layout)
    v = env.views()
    episode, step0 = v["episode_number"].cpu().numpy().copy(), v["step_number"].cpu().numpy().copy()
    rec = to_host(env.collect(T))
    worst, n_all_masked = {}, 0
    for t in range(T):
        r, n = cr.check_actor_record(rec, t, a_inter, a_intra, stochastic, seed, episode, step0 + t, layout)
        n_all_masked += n
        r["vf"] = cr.check_values(rec["vf"][t], rec["obs_inter"][t], rec["obs_intra"][t], rec["mask_intra"][t], v_inter, v_intra, layout, f"vf[{t}]")
        for k, x in r.items():
            worst[k] = max(worst.get(k, 0.0), x)
    worst["vf_T"] = cr.check_values(rec["vf"][T], env.obs_inter, env.obs_intra, env.views()["mask_intra"], v_inter, v_intra, layout, "vf[T]")
    print(f"worst error / bound: {worst}; all-masked rows: {n_all_masked}")
    env.close()


def test_values_without_an_intra_critic_and_without_intra_nets():
    """No intra critic: columns 1..S of vf are 0; no intra actor: columns 1..S of logp are 0 too and the intra fields stay untouched."""
    need_gpu()
    B = 32
    _, env, (a_inter, a_intra, v_inter, _) = cr.make_env("S5U25", "64x64", B, intra_critic=False)
    rec = to_host(env.collect(6))
    for t in range(6):
        cr.check_values(rec["vf"][t], rec["obs_inter"][t], None, None, v_inter, None)
    assert np.any(rec["logp"][:, :, 1:] != 0.0)
    env.close()
    _, env, (a_inter, _, v_inter, _) = cr.make_env("S5U25", "64x64", B, intra=False)
    out = env.collect(6)
    out["obs_intra"].fill_(7.0)
    out["action_intra"].fill_(9)
    rec = to_host(env.collect(6))
    assert np.all(rec["logp"][:, :, 1:] == 0.0) and np.all(rec["vf"][:, :, 1:] == 0.0)
    assert np.all(rec["obs_intra"] == 7.0) and np.all(rec["action_intra"] == 9)
    cr.check_values(rec["vf"][6], env.obs_inter, None, None, v_inter, None)
    env.close()


GAMMA_LAMBDA = [(0.99, 0.95), (0.6, 0.95), (0.999, 1.0), (0.9, 0.0)]


@pytest.mark.parametrize("autoreset", [False, True])
@pytest.mark.parametrize("size", list(cr.SIZES))
def test_gae_equals_the_numpy_statement_exactly(size, autoreset):
    """adv / vtarg of the call, and of ranenv_gae with other (gamma, lambda) on the same record, equal adapters.gae bit for bit."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd import adapters
    _, env, _ = cr.make_env(size, "64x64", 48, autoreset=autoreset, parts=3, intra_input=_layout(size))
    out = env.collect(T, gamma=0.99, lam=0.95)
    rec = to_host(out)
    assert bool(rec["done"].any()) == autoreset
    adv, vtarg = adapters.gae(rec["reward"], rec["vf"], rec["done"], 0.99, 0.95)
    assert np.array_equal(rec["adv"], adv) and np.array_equal(rec["vtarg"], vtarg)
    assert np.all(np.isfinite(adv)) and np.any(adv != 0.0)
    for gamma, lam in GAMMA_LAMBDA:
        a, vt = env.gae(out["reward"], out["vf"], out["done"], gamma, lam)
        want_a, want_v = adapters.gae(rec["reward"], rec["vf"], rec["done"], gamma, lam)
        assert np.array_equal(a.cpu().numpy(), want_a), (gamma, lam)
        assert np.array_equal(vt.cpu().numpy(), want_v), (gamma, lam)
    env.close()


@pytest.mark.parametrize("autoreset", [False, True])
def test_determinism_and_partitions(autoreset):
    """The same seed twice gives identical buffers; 1 against 3 partitions gives identical buffers; another seed does not."""
    need_gpu()
    runs = {}
    for key, (parts, seed) in {"a": (1, 11), "a2": (1, 11), "p3": (3, 11), "other": (1, 12)}.items():
        _, env, _ = cr.make_env("S10U100", "64x64", 48, seed=seed, autoreset=autoreset, parts=parts)
        runs[key] = to_host(env.collect(T))
        env.close()
    for k in FIELDS:
        assert np.array_equal(runs["a"][k], runs["a2"][k]), k
        assert np.array_equal(runs["a"][k], runs["p3"][k]), k
    assert not np.array_equal(runs["a"]["action_inter"], runs["other"]["action_inter"])


@pytest.mark.parametrize("net", list(cr.NETS))
def test_fused_and_split_critic_launches_agree(net):
    """Option collect_split changes a schedule, never a result: the critic fused into its actor's launch, as a launch of its own, and
    the library's own choice give identical records."""
    need_gpu()
    runs = []
    for split in (0, 1, -1):
        _, env, _ = cr.make_env("S5U25", net, 48, autoreset=True, parts=3)
        assert env.get_option("collect_split") == -1
        env.set_option("collect_split", split)
        runs.append(to_host(env.collect(T)))
        env.close()
    for k in FIELDS:
        assert np.array_equal(runs[0][k], runs[1][k]) and np.array_equal(runs[0][k], runs[2][k]), k


def test_a_critic_wider_and_deeper_than_its_actor():
    """Actors [48] (padded to 64: the other branch of the LDS row stride) under critics [96, 96], so that the workgroup's LDS buffers are
    sized by the critic and not by the actor; B = 40 (two workgroups of env rows with a tail of 8, 200 intra rows), T = 3 with
    episodes ending at its last TTI.  Fused and split give one record; vf (intra columns and the bootstrap slot included) and logp
    lie within the float64 bounds of collect_ref."""
    need_gpu()
    B, n, seed, layout = 40, 3, 0x1234_5678_9ABC, "mask_obs"
    lengths = np.asarray((3, 2, 5, 1), dtype=np.int32)[np.arange(B) % 4]

    def make():
        _, env, _ = cr.make_env("S5U25", "64x64", B, stochastic=True, seed=seed, autoreset=True, intra_input=layout)
        a_inter, a_intra, _, _ = cr.nets(env.S, env.Us, [48], layout, seed=31)
        _, _, v_inter, v_intra = cr.nets(env.S, env.Us, [96, 96], layout, seed=31)
        env.set_policy_network(a_inter, a_intra, stochastic=True, seed=seed, intra_input=layout)
        env.set_value_network(v_inter, v_intra)
        env.set_max_steps(lengths)
        env.reset()
        return env, (a_inter, a_intra, v_inter, v_intra)

    ref, _ = make()                # the Philox counters of every TTI, from a step() loop
    counters = []
    for _ in range(n):
        v = ref.views()
        counters.append((v["episode_number"].cpu().numpy().copy(), v["step_number"].cpu().numpy().copy()))
        ref.step()
    ref.close()
    runs = []
    for split in (0, 1):
        env, (a_inter, a_intra, v_inter, v_intra) = make()
        env.set_option("collect_split", split)
        rec = to_host(env.collect(n))
        runs.append(rec)
        assert rec["done"][-1].any() and not rec["done"][-1].all()
        worst = {}
        for t in range(n):
            r, _ = cr.check_actor_record(rec, t, a_inter, a_intra, True, seed, counters[t][0], counters[t][1], layout)
            r["vf"] = cr.check_values(rec["vf"][t], rec["obs_inter"][t], rec["obs_intra"][t], rec["mask_intra"][t], v_inter, v_intra, layout, f"vf[{t}]")
            for k, x in r.items():
                worst[k] = max(worst.get(k, 0.0), x)
        worst["vf_T"] = cr.check_values(rec["vf"][n], env.obs_inter, env.obs_intra, env.views()["mask_intra"], v_inter, v_intra, layout, "vf[T]")
        print(f"split {split}: worst error / bound: {worst}")
        env.close()
    for k in FIELDS:
        assert np.array_equal(runs[0][k], runs[1][k]), k


def test_null_fields_are_skipped():
    """A call that records only reward / vf / done / adv / vtarg gives the same five arrays as the full call."""
    need_gpu()
    five = ("reward", "vf", "done", "adv", "vtarg")
    _, a, _ = cr.make_env("S5U25", "64x64", 48, autoreset=True, parts=3)
    _, b, _ = cr.make_env("S5U25", "64x64", 48, autoreset=True, parts=3)
    full, part = to_host(a.collect(T)), to_host(b.collect(T, record=five))
    assert set(part) == set(five)
    for k in five:
        assert np.array_equal(full[k], part[k]), k
    assert torch.equal(a.obs_inter, b.obs_inter) and torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done)
    a.close()
    b.close()


def test_error_paths():
    need_gpu()
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd._lib import RanEnvError
    _, env, _ = cr.make_env("S5U25", "64x64", 16, critics=False)
    _, _, v_inter, v_intra = cr.nets(env.S, env.Us, cr.NETS["64x64"])
    lib, h = env._lib, env._h
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs = [C.c_void_p(x.data_ptr()) for x in (env.obs_inter, env.obs_intra, env.reward, env.done)]

    def alive():
        env.step()
        torch.cuda.synchronize()

    with pytest.raises(RanEnvError, match=r"\(-3\)"):       # no critic bound
        env.collect(4)
    alive()
    env.set_value_network(v_inter, v_intra)
    env.set_policy(_lib.POLICY_MAPF, _lib.INTRA_PF)          # policy not NETWORK
    with pytest.raises(RanEnvError, match=r"\(-3\)"):
        env.collect(4)
    alive()
    env.set_policy(_lib.POLICY_NETWORK, _lib.INTRA_PER_SLICE)
    with pytest.raises(RanEnvError, match=r"\(-1\)"):       # n_steps < 1
        env.collect(0)
    alive()
    assert lib.ranenv_collect(h, 4, None, 0.99, 0.95, *outs, stream) == -1      # NULL traj
    alive()
    good = env.collect(4)
    for missing in ("reward", "vf", "done"):                 # adv requested without what GAE reads
        tr = _lib.Trajectory()
        for k in ("reward", "vf", "done", "adv"):
            if k != missing:
                setattr(tr, k, good[k].data_ptr())
        assert lib.ranenv_collect(h, 4, C.byref(tr), 0.99, 0.95, *outs, stream) == -1, missing
        alive()
    assert lib.ranenv_collect(h, 4, C.byref(_lib.Trajectory()), 0.99, 0.95, None, outs[1], outs[2], outs[3], stream) == -1      # the nets read obs_inter
    alive()
    with pytest.raises(ValueError):                          # a critic of the wrong shape: refused before the library sees it ...
        env.set_value_network(cr.mlp([10 * env.S, 64, 2], "tanh", 1))
    bad = _lib.Mlp()                                         # ... and by the library itself
    bad.n_hidden, bad.activation, bad.input_layout = 1, _lib.ACT_TANH, _lib.NET_IN_OBS
    bad.dims[0], bad.dims[1], bad.dims[2] = 10 * env.S, 64, 2
    for i in range(2):
        bad.weight[i] = bad.bias[i] = env.obs_inter.data_ptr()
    assert lib.ranenv_set_value_network(h, C.byref(bad), None, stream) == -1
    env.collect(4)
    env.close()
    # an intra critic without an intra actor
    _, env, _ = cr.make_env("S5U25", "64x64", 16, intra=False, critics=False)
    with pytest.raises(RanEnvError, match=r"\(-1\)"):
        env.set_value_network(v_inter, v_intra)
    env.step()
    env.set_value_network(v_inter)
    env.collect(4)
    torch.cuda.synchronize()
    env.close()
