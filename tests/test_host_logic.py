"""CPU-only checks of the host layer: scenario tables, bundled plugins against the golden vectors
captured from the reference, the C-ABI library's exports, and the multi-process metrics gather."""
import ctypes
import os
import re
import socket

import numpy as np
import pytest

from intent_radio_sched_multi_slice_amd import plugins, scenario
from intent_radio_sched_multi_slice_amd.scenario import ScenarioTables
from tests.common import load_golden, tables_from

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_generator_reproduces_reference_scenarios():
    """generate_reference_scenario consumes the rng like MultSliceAssociation's generator mode
    (associations/mult_slice.py:359-423): seed 10, episodes 0..9 (gen_assoc_mult_slice.py:14)."""
    fx = load_golden("assoc_traffic")
    rng = np.random.default_rng(10)
    for ep in range(10):
        bua, bsa, sua, req, slices = scenario.generate_reference_scenario(rng, 5, 25)
        assert np.array_equal(bsa, fx["assoc_bsa"][ep])
        assert np.array_equal(sua, fx["assoc_sua"][ep])
        types = [scenario.SLICE_TYPE_NAMES.index(req[f"slice_{s}"]["name"]) if req[f"slice_{s}"] else -1 for s in range(5)]
        assert types == list(fx["assoc_types"][ep])
        assert np.sum(sua.sum(axis=0) > 1) == 0                       # gen_assoc_mult_slice.py:194-195
        assert sua.sum() == bua.sum()                                 # :197-200


def test_tables_from_reference_objects_match_golden_tables():
    fx = load_golden("assoc_traffic")
    gold = tables_from(fx, "assoc_tab_")
    rng = np.random.default_rng(10)
    t = ScenarioTables.empty(10, 5, 25, 5)
    for ep in range(10):
        bua, bsa, sua, req, _ = scenario.generate_reference_scenario(rng, 5, 25)
        t.set_from_reference(ep, bsa, sua, req, True)
    for name, arr in gold.arrays().items():
        got = getattr(t, name)
        if name in ("ue_pkt_size", "ue_max_pkts", "ue_max_age"):
            mask = gold.ue_slice >= 0                                  # idle UEs: defaults differ by design
            assert np.array_equal(got[mask], arr[mask]), name
        else:
            assert np.array_equal(got, arr), name


def test_tables_roundtrip_and_validation():
    t = scenario.generate_scaled_scenarios(5, seed=3)
    for i in range(t.n_scenarios):
        bua, bsa, sua, req = t.to_reference(i)
        t2 = ScenarioTables.empty(1, t.n_slices, t.n_ues, t.max_ues_slice)
        t2.set_from_reference(0, bsa, sua, req, True)
        for name in ("slice_active", "slice_nues", "slice_ues", "param_metric", "param_op", "param_value",
                     "sorted_slices", "ue_slice", "ue_pos", "ue_pkt_size", "ue_max_pkts", "ue_max_age"):
            assert np.array_equal(getattr(t2, name)[0], getattr(t, name)[i]), name
        assert 6 <= int(t.slice_active[i].sum()) <= 10
        n = t.slice_nues[i][t.slice_active[i] == 1]
        assert n.min() >= 4 and n.max() <= 10
    t.validate(400, 135, 100e6)
    with pytest.raises(ValueError):
        t.validate(100, 135, 100e6)            # uav_app_case_1 needs 400 TTIs
    bad = np.zeros((10, 100)); bad[0, 3] = bad[1, 3] = 1
    with pytest.raises(ValueError):
        t.set_from_reference(0, np.ones((1, 10)), bad, {f"slice_{s}": {} for s in range(10)})


def test_mult_slice_traffic_draw_order_matches_reference():
    """traffics/mult_slice.py:24-32 for seeds 10 and 15 (simu.py:203-204)."""
    fx = load_golden("assoc_traffic")
    tabs = tables_from(fx, "assoc_tab_")
    bua, bsa, sua, req = tabs.to_reference(0)
    for seed in (10, 15):
        tr = plugins.MultSliceTraffic(25, np.random.default_rng(seed))
        got = np.array([tr.step(sua, req, t, 0) for t in range(20)])
        assert np.array_equal(got, fx[f"traffic_seed{seed}"])


def test_simple_plugins():
    assert np.array_equal(plugins.SimpleTraffic(4, None).step(None, None, 0, 0), np.full(4, 4.0))
    se = plugins.FixedSE(4, 1, np.array([25]), None).step(0, 0, None)
    assert se.shape == (1, 4, 25) and np.all(se == 2.0)
    assert plugins.SimpleMobility(4, None).step(0, 0).shape == (4, 2)
    ues = plugins.UEs(5, np.repeat(100, 5), np.repeat(1024, 5), np.repeat(100, 5))
    ues.update_ues(np.array([1, 3]), np.array([20, 20]), np.array([10, 10]), np.array([8, 8]))
    assert ues.buffers[1].max_packets_age == 20 and ues.max_buffer_pkts[3] == 10 and ues.pkt_sizes[0] == 100
    se_q = plugins.quadriga_se_from_power(np.array([[1e-12]]), 135)
    assert np.isclose(se_q[0, 0], np.log2(1 + (100 / 135) * 1e-12 / 1e-13))


def test_c_abi_library_exports_every_declared_symbol():
    """The HIP library must load on a CPU-only host and export what include/ranenv.h declares."""
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.csrc import build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "ranenv.h")).read()
    declared = set(re.findall(r"\b(ranenv_[a-z_]+)\s*\(", header))
    declared -= {"ranenv_config", "ranenv_handle"}
    assert declared, "no declarations parsed"
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name
    assert lib.ranenv_abi_version() == _lib.ABI_VERSION
    assert ctypes.sizeof(_lib.Episode) == 40 and ctypes.sizeof(_lib.Config) == 96


def test_product_path_never_imports_the_oracle():
    pkg = os.path.join(REPO, "intent_radio_sched_multi_slice_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(root, f)).read()
                assert "pyoracle" not in text and "from oracle" not in text and "import oracle" not in text, f
                assert "libranenv_oracle" not in text, f


def test_shard_range_partitions_the_batch():
    from intent_radio_sched_multi_slice_amd.dist import shard_range
    for total in (1, 7, 4096, 32768, 32771):
        for world in (1, 2, 3, 8):
            spans = [shard_range(total, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == total
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [hi - lo for lo, hi in spans]
            assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        shard_range(10, 2, 2)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _gather_worker(rank, world, port, out):
    import torch
    import torch.distributed as dist
    from intent_radio_sched_multi_slice_amd.dist import gather_metrics, local_metrics, shard_range, summarize
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lo, hi = shard_range(10, rank, world)
    b = hi - lo
    reward = torch.full((b, 3), -0.5 if rank == 0 else 0.25, dtype=torch.float64)
    views = {k: torch.full((b, 4), rank + 1, dtype=torch.int32) for k in
             ("pkt_effective_thr", "dropped_pkts", "pkt_incoming", "queue_pkts")}
    g = gather_metrics(local_metrics(reward, views, torch.zeros(b, dtype=torch.uint8), 5))
    out.put((rank, summarize(g), tuple(g.shape)))
    dist.barrier(); dist.destroy_process_group()


def test_metrics_gather_world_size_2_gloo():
    """The only collective of the build: all ranks end with every rank's
    accumulator vector; on GPUs the same call runs over RCCL."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in procs]
    res = sorted(q.get(timeout=120) for _ in range(2))
    [p.join(60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    for rank, summ, shape in res:
        assert shape == (2, 8)
        assert summ["env_steps"] == 10 * 5
        assert summ["violations"] == 5                       # rank 0's five envs have negative reward
        assert summ["pkts_sent"] == 5 * 4 * 1 + 5 * 4 * 2
        assert np.isclose(summ["reward_inter_sum"], 5 * -0.5 + 5 * 0.25)


def test_scenario_file_roundtrip_and_replay(tmp_path):
    """ep_N.npz in the schema of gen_assoc_mult_slice.py:229-237: writer -> reader -> scenario tables equal
    the tables made from the objects directly; MultSliceAssociation in replay mode serves them per step."""
    from intent_radio_sched_multi_slice_amd.plugins import MultSliceAssociation, UEs
    from intent_radio_sched_multi_slice_amd.scenario import (ScenarioTables, generate_reference_scenario,
                                                           load_episode_npz, save_episode_npz,
                                                           tables_from_episode_files)
    S, U, Us = 5, 25, 5
    root = tmp_path / "associations" / "data" / "mult_slice"
    root.mkdir(parents=True)
    direct = ScenarioTables.empty(3, S, U, Us)
    objs = []
    for n in range(3):
        rng = np.random.default_rng(100 + n)
        bua, bsa, sua, req, slices = generate_reference_scenario(rng, S, U, 3)
        save_episode_npz(str(root / f"ep_{n}.npz"), bua, bsa, sua, req, slices, n_steps=4)
        direct.set_from_reference(n, bsa, sua, req, True)
        objs.append((bua, bsa, sua, req, slices))
    ep = load_episode_npz(str(root / "ep_1.npz"))
    assert ep["hist_slice_ue_assoc"].shape == (4, S, U) and ep["hist_slice_req"][2] == objs[1][3]
    got = tables_from_episode_files([str(root / f"ep_{n}.npz") for n in range(3)], S, U, Us)
    for k, a in direct.arrays().items():
        assert np.array_equal(a, got.arrays()[k]), k
    # replay mode of the association plugin (associations/mult_slice.py:424-442)
    ues = UEs(U, np.repeat(1, U), np.repeat(1, U), np.repeat(1, U))
    assoc = MultSliceAssociation(ues, U, 1, S, np.random.default_rng(0), str(tmp_path), generator_mode=False)
    z = (np.zeros((1, U)), np.zeros((1, S)), np.zeros((S, U)), {})
    for episode in (0, 1, 202):                      # 202 % 200 = 2
        for step in range(3):
            bua, bsa, sua, req = assoc.step(*z, step, episode)
            want = objs[episode % 200]
            assert np.array_equal(sua, want[2]) and np.array_equal(bsa, want[1]) and req == want[3]
        s0 = int(want[4][0])
        members = np.nonzero(want[2][s0])[0]
        assert np.all(ues.pkt_sizes[members] == want[3][f"slice_{s0}"]["ues"]["message_size"])
    with pytest.raises(ValueError, match="not a scenario file"):
        np.savez(str(tmp_path / "bad.npz"), x=np.zeros(3))
        load_episode_npz(str(tmp_path / "bad.npz"))


def test_quadriga_channel_plugin_with_a_fake_hdf5_file(tmp_path, monkeypatch):
    """channels/quadriga.py:38-87 and quadriga_seq.py:28-39: which file is opened for which episode, the
    per-step slice, the log2(1 + SNR) transform and the (1, U, R) orientation.  h5py is absent here, so the
    file object is a stand-in with the two calls the plugin makes (File(path, "r").get(name)[...])."""
    from intent_radio_sched_multi_slice_amd import plugins
    U, R, T = 6, 9, 4
    rng = np.random.default_rng(3)
    store, opened = {}, []

    class FakeFile:
        def __init__(self, path):
            self.path = path
            opened.append(path)
            store.setdefault(path, 10.0 ** rng.uniform(-14, -9, size=(T, R, 1, 1, U)))   # [step][R][1][1][U]

        def get(self, name):
            assert name == "target_cell_power"
            return store[self.path]

        def close(self):
            pass

    monkeypatch.setattr(plugins.QuadrigaChannel, "_open", lambda self, path: FakeFile(path))
    ch = plugins.QuadrigaChannel(U, 1, np.array([R]), np.random.default_rng(0), str(tmp_path), "whatever")
    for episode, step in ((0, 0), (0, 3), (2, 1)):
        se = ch.step(step, episode, None)
        path = f"{tmp_path}/mult_slice_channel_generation/results/mult_slice/freq_channel/assoc_{episode}/ep_0/target_cell_power.mat"
        assert opened[-1] == path and se.shape == (1, U, R)
        g = store[path][step, :, 0, 0, :]                                   # (R, U)
        want = np.log2(1 + (100 / R) * g / (0 + 10e-14)).T
        np.testing.assert_array_equal(se[0], want)
    assert len(opened) == 2                                                 # one open per episode change
    seq = plugins.QuadrigaChannelSeq(U, 1, np.array([R]), np.random.default_rng(0), str(tmp_path), "x")
    seq.step(0, 205, None)
    assert opened[-1].endswith("assoc_2/ep_5/target_cell_power.mat")
    # without h5py the real opener fails loudly
    monkeypatch.undo()
    try:
        import h5py  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="needs h5py"):
            plugins.QuadrigaChannel(U, 1, np.array([R]), None, str(tmp_path), "x").step(0, 0, None)


def test_create_rejects_row_lengths_the_pairwise_plan_cannot_follow():
    """numpy's pairwise sum splits a row until every leaf is <= 128; the kernel follows two levels, so R in [489, 512]
    with a quarter above 128 (e.g. 500 -> 120/128/120/132) must be refused at create, not summed in another order."""
    import ctypes as C
    from intent_radio_sched_multi_slice_amd import _lib
    lib = _lib.load()

    def create(R):
        cfg = _lib.Config(_lib.ABI_VERSION, 0, 4, 5, 25, R, 1, 5, 10, 400, 100, 1, 0, 0, 100e6, 0.2, 120.0, 5.0, 40.0)
        h = C.c_void_p()
        st = lib.ranenv_create(C.byref(cfg), C.byref(h))
        msg = (lib.ranenv_last_error(None) or b"").decode() if st != 0 else ""     # (on success the last error is an earlier call's)
        if st == 0:
            lib.ranenv_destroy(h)
        return st, msg

    for R in (490, 500, 511):
        st, msg = create(R)
        assert st == -1 and "pairwise" in msg, (R, st, msg)
    for R in (488, 512):                       # valid plans: fail later (no GPU here) or succeed, but not on the size check
        st, msg = create(R)
        assert "pairwise" not in msg, (R, msg)


def test_create_rejects_unknown_flag_bits():
    """Flags are create-time switches of what is computed (RANENV_F_SCALE_PER_ELEMENT changes a rounding): a bit this library
    does not know must not be ignored silently."""
    import ctypes as C
    from intent_radio_sched_multi_slice_amd import _lib
    lib = _lib.load()
    for flags, bad in ((0x10, True), (0x8 | 0x40, True), (_lib.F_SCALE_PER_ELEMENT | _lib.F_NO_RAW_OUTPUT, False)):
        cfg = _lib.Config(_lib.ABI_VERSION, 0, 4, 5, 25, 135, 1, 5, 10, 400, 100, 1, flags, 0, 100e6, 0.2, 120.0, 5.0, 40.0)
        h = C.c_void_p()
        st = lib.ranenv_create(C.byref(cfg), C.byref(h))
        msg = (lib.ranenv_last_error(None) or b"").decode() if st != 0 else ""     # (on success the last error is an earlier call's)
        if st == 0:
            lib.ranenv_destroy(h)
        assert ("unknown bits in flags" in msg) == bad, (hex(flags), st, msg)


def test_options_table_of_the_library_matches_the_header_and_the_environment_is_read_in_one_place():
    """VERDICT r3 hygiene: every knob of the launch schedule is an option documented in include/ranenv.h ("Options"); the keys
    of the library's options table (csrc/ranenv_host.cpp) are exactly the documented ones, every settable key but the test hook is
    preset from RANENV_<KEY>, and the host side reads the process environment in ONE function; no other translation unit reads it at all."""
    import re
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(repo, "include", "ranenv.h")).read()
    csrc = os.path.join(repo, "intent_radio_sched_multi_slice_amd", "csrc")
    src = open(os.path.join(csrc, "ranenv_host.cpp")).read()
    for other in ("ranenv_step.hip", "ranenv_step_body.hpp", "ranenv_numeric.hpp", "ranenv_aux.hip", "ranenv_internal.h"):
        assert "getenv(" not in open(os.path.join(csrc, other)).read(), other
    table = hdr[hdr.index("/* Options:"):hdr.index("int ranenv_set_option")]
    documented = set(re.findall(r'^ \*\s+(?:\.\.\. )?"(\w+)"', table, flags=re.M))
    # the options table of the host side: one row per key, {"key", preset from RANENV_<KEY>?, setter, getter}
    rows_src = src[src.index("const Option options[]"):src.index("\n};", src.index("const Option options[]"))]
    rows = dict(re.findall(r'\{"(\w+)", (true|false),', rows_src))
    assert len(rows) == len(re.findall(r'\{"\w+"', rows_src))
    accepted = set(rows)
    setter = src[src.index("int set_option(ranenv_handle h"):src.index("void apply_env_options")]
    if "fuse_first_index(k)" in setter:
        accepted |= {"fuse_first0", "fuse_first9"}
    read_only = {"persist_errors", "persist_stat_keep", "last_rollout_persistent"}          # (answered by ranenv_get_option only)
    no_env = {"persist_inject_abort"}                            # (a test hook: set per handle only)
    assert accepted <= documented, accepted - documented
    assert documented - accepted <= read_only, documented - accepted - read_only
    accepted -= no_env
    assert {k for k, env in rows.items() if env == "false"} == no_env
    # every documented env variable is RANENV_<KEY>, and getenv appears inside apply_env_options only
    env_fn = src[src.index("void apply_env_options"):src.index("}  // namespace", src.index("void apply_env_options"))]
    assert src.count("getenv(") == env_fn.count("getenv(") == 2
    # the launch counters ("step_launches_<build>") are answered by ranenv_get_option alone: no row of the table (so no setter and no
    # RANENV_ variable), and no step launch whose result is thrown away
    assert not any(k.startswith("step_launches") for k in rows) and 'k.rfind("step_launches_", 0) == 0' in src
    assert "step_launches" not in setter and not re.search(r"\(void\)\s*launch_step", src) and src.count("launch_step_counted(h, ") == 2
    assert "for (const Option &o : options)" in env_fn and '"RANENV_"' in env_fn and '"RANENV_FUSE_FIRST"' in env_fn
    for key in accepted - {"fuse_first0", "fuse_first9"}:
        assert rows[key] == "true", key
        assert "RANENV_" + key.upper() in table, key


def test_packed_waves_are_refused_where_a_32_bit_row_offset_could_wrap():
    """packed waves (two envs per wave) address a per-env row as array base + a 32-bit offset; the guard must cover every
    array addressed that way by its ACTUAL allocation -- the intent-parameter tables are two blocks of NS * S * 24 bytes, the per-UE
    state slabs 11 / 4 fields of B * U elements, the score rows B * S * 8.  Pure host arithmetic (ranenv_packed_step_fits): no GPU."""
    import ctypes as C
    from intent_radio_sched_multi_slice_amd import _lib
    lib = _lib.load()

    def fits(B=16384, S=5, U=25, Us=5, NS=200, D=10, trf=200_000, tiles=200_000):
        cfg = _lib.Config(_lib.ABI_VERSION, 0, B, S, U, 135, 5, Us, D, 400, 1000, NS, 0, 0, 100e6, 0.2, 120.0, 5.0, 40.0)
        r = lib.ranenv_packed_step_fits(C.byref(cfg), trf, tiles)
        assert r in (0, 1)
        return bool(r)

    lim = 1 << 32
    assert fits()                                                # the reference's own size at the bench batch
    # the by-metric block of the parameter tables: 2 * NS * S * 24 bytes (the round-5 guard checked NS * S * 32 only)
    ns_edge = lim // (2 * 5 * 24)                                # 2 * ns_edge * 5 * 24 <= lim < 2 * (ns_edge + 1) * 5 * 24
    assert 2 * ns_edge * 5 * 24 < lim or 2 * ns_edge * 5 * 24 == lim
    assert not fits(NS=ns_edge + 1, U=1, Us=1)                   # (U = 1: the per-UE tables, 12 * NS * U * 4, stay below the bound)
    assert fits(NS=ns_edge - 1, U=1, Us=1)
    # the 4-byte state slab: 11 fields of B * U elements
    b_edge = lim // (11 * 25 * 4)
    assert not fits(B=b_edge + 1) and fits(B=b_edge - 2)
    # the traffic pool and the sidecar of means
    assert not fits(trf=lim // (25 * 4) + 1) and fits(trf=lim // (25 * 4) - 1)
    assert not fits(tiles=lim // (25 * 8) + 1) and fits(tiles=lim // (25 * 8) - 1)
    assert lib.ranenv_packed_step_fits(None, 0, 0) < 0


def test_xcd_aware_env_mapping_is_a_permutation():
    """The index arithmetic of the XCD-aware env mapping (csrc/ranenv_step_body.hpp: step_loop's b_perm, the mixed launches' wide / narrow
    positions, persist_try_fresh's contiguous shards), restated: every env of a launch is stepped by exactly one workgroup, and workgroup
    8 i + k -- XCD k -- gets a contiguous run.  (The kernels themselves are covered by the GPU parity tests: a wrong mapping steps an env
    twice or not at all.)"""
    import random

    def plain(nb):                       # step_loop: workgroup b of nb -> position in the launch's env range
        q, r = nb >> 3, nb & 7
        return [(b & 7) * q + min(b & 7, r) + (b >> 3) for b in range(nb)]

    def narrow_positions(n_wide, n_narrow):
        nbn, o = (n_narrow + 1) >> 1, n_wide & 7

        def cnt(x):
            hi = o + nbn - 1
            return 0 if hi < x else ((hi - x) >> 3) + 1 - (1 if x < o else 0)
        out = []
        for b in range(n_wide, n_wide + nbn):
            k8, c = b & 7, b - n_wide + o
            assert c & 7 == k8
            out.append(sum(cnt(x) for x in range(k8)) + (c >> 3) - (1 if k8 < o else 0))
        return out, nbn

    def shards(n):                       # persist_try_fresh: shard x = [x * per, min((x + 1) * per, n))
        per = (n + 7) >> 3
        return [x * per + j for x in range(8) for j in range(per) if x * per + j < n]

    rng = random.Random(5)
    cases = [(0, 0), (0, 1), (5, 0), (1023, 3073), (1366, 0), (7, 9), (8, 16)] + [(rng.randint(0, 70), rng.randint(0, 300)) for _ in range(400)]
    for n_wide, n_narrow in cases:
        p = plain(n_wide)
        assert sorted(p) == list(range(n_wide))
        for k in range(8):               # XCD k's workgroups, in id order, walk a contiguous ascending run
            run = [p[b] for b in range(k, n_wide, 8)]
            assert run == list(range(run[0], run[0] + len(run))) if run else True
        pos, nbn = narrow_positions(n_wide, n_narrow)
        assert sorted(pos) == list(range(nbn))
        assert sorted(shards(n_narrow)) == list(range(n_narrow))
