"""The state of a launch's inner TTIs (option "lean_state"): inside a launch of several TTIs only an env's last TTI before
it can go cold -- the launch's last, a persistent chunk's last -- stores the per-UE state that the next TTI of the same workgroup holds in
registers (StepCarry) or never reads, and that TTI does not load it back; every build but the packed-waves one hands the rest of the
state (queue_age_sum, front, front_rem, fifo, win_dropped) over the same way.  Nothing can read the state in between, so after EVERY call
every buffer and every view holds, bit for bit, what one launch per TTI (fuse = 1, persist = 0: every TTI stores and loads everything)
leaves -- and so do the per-UE fields no view shows (front, front_rem, fifo, last_push), read here straight from the handle's slab.

The workload's UEs expire packets after 3..6 TTIs (ue_max_age lowered in this file), so that inside the 42 TTIs of a run the age list is
popped by expiry as well as by sending; the reference run of every case asserts that its inputs reach the UE step's branches: a full
window, a UE with two age-list entries or more, a UE with a queue age sum, a UE that dropped packets by expiry.

Every view is compared whole, except the mean SE and the four hidden fields: at the UEs in a slice only (LOOSE_SE_MEAN, tests/gpu_common.py
-- a compact step touches nothing of a UE outside every slice, and the schedules differ in which of their launches step compactly)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from intent_radio_sched_multi_slice_amd import _lib
from intent_radio_sched_multi_slice_amd.batched_env import _DevArray
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
# the per-UE fields no view shows: their index in the handle's slab of 4-byte per-UE fields, which starts at queue_pkts (ranenv_internal.h: ST_*)
HIDDEN = {"front": 1, "front_rem": 2, "fifo": 3, "last_push": 10}


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
    for chunk in (1, 2, 3):                         # (a grid of 4 wave slots: envs change hands at every chunk)
        out.append((f"persist-chunk{chunk}", dict(persist=1, persist_chunk=chunk, persist_grid=4)))
    # every TTI stores and loads everything, under a fused and a persistent schedule; and the state kept while every TTI runs the whole tail
    out.append(("fuse3-full-state", dict(fuse=3, persist=0, lean_state=0)))
    out.append(("persist-chunk2-full-state", dict(persist=1, persist_chunk=2, persist_grid=4, lean_state=0)))
    out.append(("fuse3-full-tail", dict(fuse=3, persist=0, lean_tail=0, lean_state=1)))
    out.append(("persist-chunk2-full-tail", dict(persist=1, persist_chunk=2, persist_grid=4, lean_tail=0, lean_state=1)))
    return out


def _make(shape, se_mode, policy, variant, options):
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    B, kw, shape_opts = SHAPES[shape]
    wl = make_mult_slice_workload(B, torch.device("cuda", 0), policy=POLICIES[policy][0], intra=POLICIES[policy][1], n_scenarios=N_SCEN,
                                  n_traces=N_TRACES, trace_len=TRACE_LEN, max_steps=1000, **kw)
    env = wl.env
    # packets expire after 3..6 TTIs (the templates' 20..400 would never expire one inside a run of 43 TTIs); the slices' own
    # buffer_latency -- the latency intent's denominator -- stays
    t = wl.tables
    short = 3 + (np.arange(t.ue_max_age.shape[1]) % 4)[None, :]
    t.ue_max_age[...] = np.where(t.ue_slice >= 0, np.minimum(t.ue_max_age, short), t.ue_max_age)
    env.load_scenarios(t)
    env.set_se_mode(se_mode)
    for k, v in dict(shape_opts, **options).items():
        env.set_option(k, v)
    if "autoreset" in variant:
        # scenarios change from episode to episode: a UE that comes back into a slice catches its window up on a cold TTI, warm TTIs follow
        ep = np.arange(N_EP)
        env.set_episode_table(scenario=(ep * 5) % N_SCEN, se_base=(ep % N_TRACES) * TRACE_LEN, se_len=TRACE_LEN, se_offset=ep % TRACE_LEN,
                              trf_base=((ep * 5) % N_SCEN) * TRACE_LEN, trf_len=TRACE_LEN, trf_offset=(ep * 7) % TRACE_LEN)
        env.set_max_steps(5 + np.arange(B) % 9)                      # 5..13 TTIs
        env.enable_autoreset(0, N_EP, episode_numbers=np.arange(B) % N_EP)
    if "metrics" in variant:
        env.enable_metrics(16)
    env.reset()
    return wl


def _hidden(env):
    base, n = env.views()["queue_pkts"].data_ptr(), env.B * env.U
    return {k: torch.as_tensor(_DevArray(base + i * n * 4, (env.B, env.U), "i4", env), device=env.device) for k, i in HIDDEN.items()}


def _snap(wl, variant):
    torch.cuda.synchronize()
    env = wl.env
    members = in_slice_mask(wl.tables, env)
    d = {"view:" + k: v.clone() for k, v in env.views().items()}
    d["view:se_mean"] = torch.where(members, d["view:se_mean"], torch.zeros_like(d["view:se_mean"]))
    for k, v in _hidden(env).items():
        d["hidden:" + k] = torch.where(members, v, torch.zeros_like(v))
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
        calls.append(dict(k=k, kept=env.get_option("last_rollout_kept_state_ttis"), prof=prof, persistent=env.get_option("last_rollout_persistent")))
    env.set_option("mix", 0)            # (the further step is COMMON: the same one-TTI launch in every run, not a launch of mixed blocks in one of them)
    env.step()
    snaps.append(_snap(wl, variant))
    return snaps, calls


def _reached(snaps, env):
    """Which of the UE step's branches the run's inputs reach, seen at the compared call boundaries."""
    D = env.hist_depth
    full = any(bool((s["view:hist_len"] == D).any()) for s in snaps)
    two = any(bool(((s["hidden:fifo"] >> 16) >= 2).any()) for s in snaps)
    aged = any(bool((s["view:queue_age_sum"] > 0).any()) for s in snaps)
    # an overflowing buffer drops at most what came in: more dropped than came in is packets that expired
    expired = any(bool((s["view:dropped_pkts"] > s["view:pkt_incoming"]).any()) for s in snaps)
    return dict(window_full=full, two_entries=two, age_sum=aged, expired=expired)


_reference = {}


def _reference_of(shape, se_mode, policy, variant):
    """One launch per TTI, computed once per case and shared by the schedules that are compared with it."""
    key = (shape, se_mode, policy, variant)
    if key not in _reference:
        wl = _make(shape, se_mode, policy, variant, REFERENCE)
        if shape == "s10u100":
            members = (wl.tables.ue_slice[wl.scenario] >= 0).sum(axis=1)
            assert (members > 64).any() and (members <= 64).any(), members       # envs of one wave and of two
        snaps, calls = _walk(wl, variant)
        assert all(c["kept"] == 0 and c["persistent"] == 0 for c in calls), calls       # one TTI per launch: every TTI flushes
        reached = _reached(snaps, wl.env)
        print("lean_state reference", key, reached)
        assert all(reached.values()), (key, reached)
        if "autoreset" in variant:
            lengths = set((5 + np.arange(SHAPES[shape][0]) % 9).tolist())
            assert {5, 6, 12}.issubset(lengths) and int(wl.env.views()["episode_number"].max()) >= 3
        wl.env.close()
        _reference[key] = snaps
    return _reference[key]


@pytest.mark.parametrize("variant", ["plain", "metrics", "autoreset"])
@pytest.mark.parametrize("policy", sorted(POLICIES))
@pytest.mark.parametrize("se_mode", ["stream", "gather"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_kept_state_leaves_what_one_launch_per_tti_leaves(shape, se_mode, policy, variant):
    need_gpu()
    ref = _reference_of(shape, se_mode, policy, variant)
    for name, options in _schedules(shape, se_mode):
        wl = _make(shape, se_mode, policy, variant, options)
        snaps, calls = _walk(wl, variant)
        for i, (got, want) in enumerate(zip(snaps, ref)):
            assert got.keys() == want.keys()
            for k in want:
                assert torch.equal(got[k], want[k]), (name, "call", i, k)
        on = options.get("lean_state", 1) != 0
        for c in calls:
            # every launch of n TTIs enqueues n - 1 that keep the state (the profile counts the launches and their TTIs; a reset is one of one)
            assert c["kept"] == (c["prof"]["n_ttis"] - c["prof"]["n_launches"] if on else 0), (name, c)
            assert c["persistent"] == (1 if options.get("persist") == 1 else 0), (name, c)
        if on and "autoreset" not in variant:
            assert sum(c["kept"] for c in calls) > 0, (name, calls)                     # the path ran
        if options.get("persist") == 1:
            assert wl.env.get_option("persist_errors") == 0
            if "autoreset" not in variant:
                assert wl.env.get_option("persist_stat_push") > 0, name                  # envs changed hands
        wl.env.close()


def _persist_batch(env_threads):
    """Just above 2 waves per SIMD (8 per CU): the smallest even batch whose rollouts the streaming work-queue build takes, not the
    whole-row one (as tests/test_gpu_lean_tail.py computes it)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return (8 * cus // (env_threads // 64) + 2) // 2 * 2


def test_the_streaming_work_queue_builds_at_the_headline_shape():
    """ranenv_persist_kernel<false, 10> and ranenv_persist_kernel_members<10> -- the headline's persistent builds -- need a batch
    beyond 2 waves per SIMD: the smallest one, envs changing hands every 3 TTIs, against one launch per TTI."""
    need_gpu()
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    B = _persist_batch(128)
    outs = []
    for options in (REFERENCE, dict(persist=1, persist_chunk=3, persist_grid=192, small_batch=0, member_lines=0),
                    dict(persist=1, persist_chunk=3, persist_grid=192, small_batch=0, member_lines=1)):
        wl = make_mult_slice_workload(B, torch.device("cuda", 0), n_scenarios=N_SCEN, n_traces=N_TRACES, trace_len=TRACE_LEN, max_steps=1000)
        env = wl.env
        env.set_se_mode("stream")
        for k, v in options.items():
            env.set_option(k, v)
        env.reset()
        before = launches_since(env)
        snaps = []
        for k in (1, 7, 10):
            env.rollout(k)
            snaps.append(_snap(wl, "plain"))
            if options is not REFERENCE:
                n_launches = env.get_option("last_rollout_launches")
                assert env.get_option("last_rollout_kept_state_ttis") == n_launches * (k - 1), (options, k)
                assert env.get_option("last_rollout_member_lines") == options["member_lines"], (options, k)
        env.step()
        snaps.append(_snap(wl, "plain"))
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


def test_the_counter_of_kept_state_ttis():
    """last_rollout_kept_state_ttis: n_tti - 1 per step launch of the last rollout call; 0 for launches of one TTI, with lean_state = 0
    and for a call that a policy net forces to one TTI per launch.  The option has its default."""
    need_gpu()
    wl = _make("s5u25", "stream", "mapf-pf", "plain", {})
    env = wl.env
    assert env.get_option("lean_state") == 1 and env.get_option("last_rollout_kept_state_ttis") == 0
    env.set_option("persist", 0); env.set_option("fuse", 3)
    env.rollout(10)                                                  # one partition: launches of 3 + 3 + 3 + 1 TTIs
    assert (env.get_option("last_rollout_launches"), env.get_option("last_rollout_kept_state_ttis")) == (4, 6)
    env.rollout(1)
    assert env.get_option("last_rollout_kept_state_ttis") == 0
    env.set_option("persist", 1)
    env.rollout(10)                                                  # one class (one wave per env): one launch of 10 TTIs
    assert (env.get_option("last_rollout_persistent"), env.get_option("last_rollout_launches"), env.get_option("last_rollout_kept_state_ttis")) == (1, 1, 9)
    env.set_option("lean_state", 0)
    assert env.get_option("lean_state") == 0
    env.rollout(10)
    assert env.get_option("last_rollout_kept_state_ttis") == 0 and env.get_option("last_rollout_lean_ttis") == 9      # (the tail's option is its own)
    env.set_option("persist", 0)
    env.rollout(10)
    assert (env.get_option("last_rollout_launches"), env.get_option("last_rollout_kept_state_ttis")) == (4, 0)
    env.set_option("lean_state", 7)                                  # (any value but 0 is on)
    assert env.get_option("lean_state") == 1
    env.set_option("fuse", 1)
    env.rollout(10)
    assert (env.get_option("last_rollout_launches"), env.get_option("last_rollout_kept_state_ttis")) == (10, 0)
    env.set_option("fuse", 3)
    env.set_policy_network(make_inter_net(env.S, [32], "tanh", 1), fixed_intra=_lib.INTRA_RR)
    env.rollout(6)                                                   # the net runs in front of every TTI: one TTI per launch
    assert (env.get_option("last_rollout_launches"), env.get_option("last_rollout_kept_state_ttis")) == (6, 0)
    torch.cuda.synchronize()
    env.close()


def test_the_environment_variable_presets_the_option(monkeypatch):
    need_gpu()
    monkeypatch.setenv("RANENV_LEAN_STATE", "0")
    wl = _make("s5u25", "stream", "mapf-pf", "plain", {})
    assert wl.env.get_option("lean_state") == 0
    wl.env.close()
