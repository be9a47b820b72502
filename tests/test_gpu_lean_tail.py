"""The last TTI's tail (option "lean_tail"): inside a launch of several TTIs only an env's last TTI of the launch computes
and stores the observation rows, the rewards, `done` and the raw per-UE outputs -- and, with the episode metrics off, the intent
drift, the per-slice means and the reward arithmetic.  Nothing can read those buffers in between, so after EVERY call every buffer
and every view holds, bit for bit, what one launch per TTI (fuse = 1, persist = 0: always the whole tail) leaves: for launches per
chunk of 2, 3 and 7 TTIs and persistent launches whose envs change hands at every chunk of 1, 2 or 3 TTIs; row widths 8 / 10 / 16, two
envs per wave, one to four waves per env; both SE modes, member lines on and off, MARR + RR and MAPF + PF; with the episode metrics
on (the reward arithmetic stays, the rows go) and off; through device auto-resets with per-env episode lengths of 5..13 TTIs (calls
end inside an episode, on an episode end, one TTI behind one); and with lean_tail = 0 under the same schedules.

Every view is compared whole, except the mean SE: at the UEs in a slice only (LOOSE_SE_MEAN, tests/gpu_common.py -- a compact step does
not keep it up for a UE outside every slice, nothing reads it there, and the schedules differ in which of their launches step
compactly)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from intent_radio_sched_multi_slice_amd import _lib
from tests.gpu_common import OUTPUTS, in_slice_mask, launches_since, make_inter_net, need_gpu

pytestmark = pytest.mark.gpu

CALLS = (1, 2, 3, 7, 10, 4, 15)
N_SCEN, N_TRACES, TRACE_LEN, N_EP = 12, 6, 20, 12
# name -> (batch, workload shape, options every handle of the shape gets)
SHAPES = {
    # row width 8, one wave per env, one env per wave (packed waves off)
    "s3u12": (24, dict(n_slices=3, n_ues=12, n_rbs=12, rbs_per_rbg=1, max_ues_slice=4, min_slices=2, min_ues=2), dict(pack=0)),
    # row width 10, the headline's shape: envs of one wave (<= 64 slice members) and of two
    "s10u100": (16, dict(), dict()),
    # row width 16, four waves per env
    "s16u256": (8, dict(n_slices=16, n_ues=256, n_rbs=48, rbs_per_rbg=1, max_ues_slice=16, min_slices=8, min_ues=1), dict()),
    # row width 8, two envs per wave
    "s5u25": (32, dict(n_slices=5, n_ues=25, n_rbs=135, rbs_per_rbg=5, max_ues_slice=5, min_slices=3, min_ues=2), dict()),
}
POLICIES = {"marr-rr": (_lib.POLICY_MARR, _lib.INTRA_RR), "mapf-pf": (_lib.POLICY_MAPF, _lib.INTRA_PF)}
REFERENCE = dict(fuse=1, persist=0)


def _schedules(shape, se_mode):
    """The runs under test of one case: (name, options)."""
    out = []
    if se_mode == "stream":
        # the lean build of several TTIs, reading whole tiles and the member-lines copy; the small-batch build
        for fuse in (2, 3, 7):
            for ml in (0, 1):
                out.append((f"fuse{fuse}-lines{ml}", dict(fuse=fuse, persist=0, small_batch=0, member_lines=ml)))
        out.append(("fuse3-small", dict(fuse=3, persist=0, small_batch=1)))
    else:
        for fuse in (2, 3, 7):
            out.append((f"fuse{fuse}", dict(fuse=fuse, persist=0)))
    if shape in ("s10u100", "s16u256"):             # (two waves per env and more: whole-batch launches as mixed blocks)
        out.append(("fuse3-mixed", dict(fuse=3, persist=0, small_batch=0, mix=2, compact=1)))
    for chunk in (1, 2, 3):
        out.append((f"persist-chunk{chunk}", dict(persist=1, persist_chunk=chunk, persist_grid=4)))
    # every TTI the whole tail, under the same schedules
    out.append(("fuse3-full-tail", dict(fuse=3, persist=0, lean_tail=0)))
    out.append(("persist-chunk2-full-tail", dict(persist=1, persist_chunk=2, persist_grid=4, lean_tail=0)))
    return out


def _make(shape, se_mode, policy, variant, options):
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    B, kw, shape_opts = SHAPES[shape]
    wl = make_mult_slice_workload(B, torch.device("cuda", 0), policy=POLICIES[policy][0], intra=POLICIES[policy][1], n_scenarios=N_SCEN,
                                  n_traces=N_TRACES, trace_len=TRACE_LEN, max_steps=1000, **kw)
    env = wl.env
    env.set_se_mode(se_mode)
    for k, v in dict(shape_opts, **options).items():
        env.set_option(k, v)
    if "autoreset" in variant:
        ep = np.arange(N_EP)
        env.set_episode_table(scenario=(ep * 5) % N_SCEN, se_base=(ep % N_TRACES) * TRACE_LEN, se_len=TRACE_LEN, se_offset=ep % TRACE_LEN,
                              trf_base=((ep * 5) % N_SCEN) * TRACE_LEN, trf_len=TRACE_LEN, trf_offset=(ep * 7) % TRACE_LEN)
        env.set_max_steps(5 + np.arange(B) % 9)                      # 5..13 TTIs
        env.enable_autoreset(0, N_EP, episode_numbers=np.arange(B) % N_EP)
    if "metrics" in variant:
        env.enable_metrics(16)
    env.reset()
    return wl


def _snap(wl, variant):
    torch.cuda.synchronize()
    env = wl.env
    d = {"view:" + k: v.clone() for k, v in env.views().items()}
    d["view:se_mean"] = torch.where(in_slice_mask(wl.tables, env), d["view:se_mean"], torch.zeros_like(d["view:se_mean"]))
    for k in OUTPUTS:
        d[k] = getattr(env, k).clone()
    if "metrics" in variant:
        for k, v in env.episode_metrics().items():
            d["metrics:" + k] = v.clone()
    return d


def _walk(wl, variant):
    """The snapshots after every call of the sequence and after one further step(), and per call the counters of the call."""
    env = wl.env
    snaps, calls = [], []
    for k in CALLS:
        env.profile_begin()
        env.rollout(k)
        prof = env.profile_end()
        snaps.append(_snap(wl, variant))
        calls.append(dict(k=k, lean=env.get_option("last_rollout_lean_ttis"), prof=prof, persistent=env.get_option("last_rollout_persistent")))
    env.set_option("mix", 0)            # (the further step is COMMON: the same one-TTI launch in every run, not a launch of mixed blocks in one of them)
    env.step()
    snaps.append(_snap(wl, variant))
    return snaps, calls


_reference = {}


def _reference_of(shape, se_mode, policy, variant):
    """One launch per TTI, computed once per case and shared by the schedules that are compared with it."""
    key = (shape, se_mode, policy, variant)
    if key not in _reference:
        wl = _make(shape, se_mode, policy, variant, REFERENCE)
        if shape == "s10u100":
            members = (wl.tables.ue_slice[wl.scenario] >= 0).sum(axis=1)
            assert (members > 64).any() and (members <= 64).any(), members
        snaps, calls = _walk(wl, variant)
        assert all(c["lean"] == 0 and c["persistent"] == 0 for c in calls), calls       # one TTI per launch: no lean TTI
        if "autoreset" in variant:
            # calls end at TTI 1, 3, 6, 13, 23, 27, 42: on an episode end (6, 13 TTIs), one TTI behind one (5, 12), inside episodes
            lengths = set((5 + np.arange(SHAPES[shape][0]) % 9).tolist())
            assert {5, 6, 12}.issubset(lengths) and int(wl.env.views()["episode_number"].max()) >= 3
        wl.env.close()
        _reference[key] = snaps
    return _reference[key]


@pytest.mark.parametrize("variant", ["plain", "metrics", "autoreset", "autoreset+metrics"])
@pytest.mark.parametrize("policy", sorted(POLICIES))
@pytest.mark.parametrize("se_mode", ["stream", "gather"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_lean_launches_leave_what_one_launch_per_tti_leaves(shape, se_mode, policy, variant):
    need_gpu()
    ref = _reference_of(shape, se_mode, policy, variant)
    for name, options in _schedules(shape, se_mode):
        wl = _make(shape, se_mode, policy, variant, options)
        snaps, calls = _walk(wl, variant)
        for i, (got, want) in enumerate(zip(snaps, ref)):
            assert got.keys() == want.keys()
            for k in want:
                assert torch.equal(got[k], want[k]), (name, "call", i, k)
        lean = options.get("lean_tail", 1) != 0
        for c in calls:
            # every launch of n TTIs enqueues n - 1 without the tail (the profile counts the launches and their TTIs; a reset is one of one)
            assert c["lean"] == (c["prof"]["n_ttis"] - c["prof"]["n_launches"] if lean else 0), (name, c)
            assert c["persistent"] == (1 if "persist" in options and options["persist"] == 1 else 0), (name, c)
        if lean and "autoreset" not in variant:
            assert sum(c["lean"] for c in calls) > 0, (name, calls)                     # the lean path ran
        if options.get("persist") == 1:
            assert wl.env.get_option("persist_errors") == 0
            if "autoreset" not in variant:
                assert wl.env.get_option("persist_stat_push") > 0, name                  # envs changed hands
        wl.env.close()


def _persist_batch(env_threads):
    """Just above 2 waves per SIMD (8 per CU): the smallest even batch whose rollouts the streaming work-queue build takes, not the
    whole-row one (as tests/test_gpu_member_lines.py computes it)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return (8 * cus // (env_threads // 64) + 2) // 2 * 2


@pytest.mark.parametrize("metrics", [False, True])
def test_the_streaming_work_queue_builds_at_the_headline_shape(metrics):
    """ranenv_persist_kernel<false, 10> and ranenv_persist_kernel_members<10> -- the headline's persistent builds -- need a batch
    beyond 2 waves per SIMD: the smallest one, envs changing hands every 3 TTIs, against one launch per TTI."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    B = _persist_batch(128)
    variant = "metrics" if metrics else "plain"
    outs = []
    for options in (REFERENCE, dict(persist=1, persist_chunk=3, persist_grid=192, small_batch=0, member_lines=0),
                    dict(persist=1, persist_chunk=3, persist_grid=192, small_batch=0, member_lines=1)):
        wl = make_mult_slice_workload(B, torch.device("cuda", 0), n_scenarios=N_SCEN, n_traces=N_TRACES, trace_len=TRACE_LEN, max_steps=1000)
        env = wl.env
        env.set_se_mode("stream")
        for k, v in options.items():
            env.set_option(k, v)
        if metrics:
            env.enable_metrics(0)
        env.reset()
        before = launches_since(env)
        snaps = []
        for k in (1, 7, 10):
            env.rollout(k)
            snaps.append(_snap(wl, variant))
            if options is not REFERENCE:
                n_launches = env.get_option("last_rollout_launches")
                assert env.get_option("last_rollout_lean_ttis") == n_launches * (k - 1), (options, k)
                assert env.get_option("last_rollout_member_lines") == options["member_lines"], (options, k)
        env.step()
        snaps.append(_snap(wl, variant))
        if options is not REFERENCE:
            d = launches_since(env, before)
            assert d["persist"] > 0 and d["persist_tiny"] == 0 and env.get_option("persist_stat_push") > 0, d
            assert env.get_option("persist_errors") == 0
        outs.append(snaps)
        env.close()
    for other in outs[1:]:
        for i, (got, want) in enumerate(zip(other, outs[0])):
            for k in want:
                assert torch.equal(got[k], want[k]), (i, k)


def test_the_counter_of_lean_ttis():
    """last_rollout_lean_ttis: n_tti - 1 per step launch of the last rollout call; 0 for launches of one TTI, with lean_tail = 0 and for
    a call that a policy net forces to one TTI per launch.  Both options have their defaults."""
    need_gpu()
    wl = _make("s5u25", "stream", "mapf-pf", "plain", {})
    env = wl.env
    assert env.get_option("lean_tail") == 1 and env.get_option("last_rollout_lean_ttis") == 0
    env.set_option("persist", 0); env.set_option("fuse", 3)
    env.rollout(10)                                                  # one partition: launches of 3 + 3 + 3 + 1 TTIs
    assert (env.get_option("last_rollout_launches"), env.get_option("last_rollout_lean_ttis")) == (4, 6)
    env.rollout(1)
    assert env.get_option("last_rollout_lean_ttis") == 0
    env.set_option("persist", 1)
    env.rollout(10)                                                  # one class (one wave per env): one launch of 10 TTIs
    assert (env.get_option("last_rollout_persistent"), env.get_option("last_rollout_launches"), env.get_option("last_rollout_lean_ttis")) == (1, 1, 9)
    env.set_option("lean_tail", 0)
    assert env.get_option("lean_tail") == 0
    env.rollout(10)
    assert env.get_option("last_rollout_lean_ttis") == 0
    env.set_option("persist", 0)
    env.rollout(10)
    assert (env.get_option("last_rollout_launches"), env.get_option("last_rollout_lean_ttis")) == (4, 0)
    env.set_option("lean_tail", 7)                                   # (any value but 0 is on)
    assert env.get_option("lean_tail") == 1
    env.set_option("fuse", 1)
    env.rollout(10)
    assert (env.get_option("last_rollout_launches"), env.get_option("last_rollout_lean_ttis")) == (10, 0)
    env.set_option("fuse", 3)
    env.set_policy_network(make_inter_net(env.S, [32], "tanh", 1), fixed_intra=_lib.INTRA_RR)
    env.rollout(6)                                                   # the net runs in front of every TTI: one TTI per launch
    assert (env.get_option("last_rollout_launches"), env.get_option("last_rollout_lean_ttis")) == (6, 0)
    torch.cuda.synchronize()
    env.close()


def test_the_environment_variable_presets_the_option(monkeypatch):
    need_gpu()
    monkeypatch.setenv("RANENV_LEAN_TAIL", "0")
    wl = _make("s5u25", "stream", "mapf-pf", "plain", {})
    assert wl.env.get_option("lean_tail") == 0
    wl.env.close()
