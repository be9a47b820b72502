"""Device traces, the parts that need no GPU: header and bindings agree, DeviceTrace's host side (cutting recorded rows into
episodes, restarting single columns, writing history files) on synthetic numpy rows, the row-to-dict function of DeviceTrace.write
and HistoryRecorder.flush pinned against a restatement of what HistoryRecorder.flush did when it was the only producer, and a
planted slip: rows whose SE is one TTI late are caught by
the file comparison of tests/test_gpu_trace.py -- under that test's conditions on its inputs, and not without them."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, U, R, Us = 3, 12, 10, 4
W = 2 * Us + 9


def _tables():
    from intent_radio_sched_multi_slice_amd.scenario import generate_scaled_scenarios
    return generate_scaled_scenarios(3, seed=4, n_slices=S, n_ues=U, max_ues_slice=Us, min_slices=2, min_ues=2)


def _rows(T, n, seed=0, done_at=()):
    """Synthetic ring contents [T, n, ...] of the dtypes the device writes; done_at: (row, column) pairs with the flag set."""
    rng = np.random.default_rng(seed)
    i4 = lambda *sh, hi=50: rng.integers(0, hi, sh).astype(np.int32)
    rows = {k: i4(T, n, U) for k in ("pkt_incoming", "pkt_throughputs", "pkt_effective_thr", "dropped_pkts", "queue_pkts")}
    rows["queue_pkts"][rng.random((T, n, U)) < 0.3] = 0                       # empty queues: the latency's other branch
    rows["queue_age_sum"] = rng.integers(0, 10 ** 6, (T, n, U)).astype(np.int64)
    rows["rb_start"], rows["rb_count"] = i4(T, n, U, hi=R), i4(T, n, U, hi=4)
    rows["se"] = (rng.random((T, n, R, U)) * 20).astype(np.float32)
    rows["reward"], rows["scores"] = rng.standard_normal((T, n, S + 1)), rng.standard_normal((T, n, S))
    rows["intra"] = rng.integers(0, 3, (T, n, S)).astype(np.uint8)
    rows["obs_inter"] = rng.standard_normal((T, n, 10 * S)).astype(np.float32)
    rows["obs_intra"] = rng.standard_normal((T, n, S, W)).astype(np.float32)
    rows["step_number"], rows["episode_number"], rows["scenario"] = (np.zeros((T, n), dtype=np.int32) for _ in range(3))
    rows["done"] = np.zeros((T, n), dtype=np.uint8)
    for t, i in done_at:
        rows["done"][t, i] = 1
    return rows


def _trace(rows, count, envs, tables, lost=None):
    from intent_radio_sched_multi_slice_amd.history import DeviceTrace
    count = np.asarray(count, dtype=np.int32)               # (an int32 array is kept as it is: the caller plays the device on it)
    lost = np.zeros_like(count) if lost is None else lost

    def reset(columns=None):
        sel = slice(None) if columns is None else list(columns)
        count[sel] = 0
        lost[sel] = 0

    return DeviceTrace(envs, len(rows["done"]), rows, lambda: (count, lost), tables, R, Us, reset_fn=reset)


def _flush_before_the_refactor(host, k, T, tables, scen, marl):
    """HistoryRecorder.flush's body for slot k as it stood when it was the only producer (env.S / U / R / Us / tables spelled out)."""
    bua, bsa, sua, req = tables.to_reference(scen)
    max_pkts = tables.ue_max_pkts[scen].astype(np.float64)
    q = host["queue_pkts"][:T, k].astype(np.float64)
    age = host["queue_age_sum"][:T, k].astype(np.float64)
    lat = np.where(q > 0, age / np.maximum(q, 1.0), 0.0)
    st, cn = host["rb_start"][:T, k], host["rb_count"][:T, k]
    r = np.arange(R)[None, None, :]
    sched = ((r >= st[:, :, None]) & (r < (st + cn)[:, :, None])).astype(np.float64)[:, None]
    se = np.swapaxes(host["se"][:T, k], 1, 2).astype(np.float64)[:, None]
    mask_inter = np.asarray(tables.slice_active[scen], dtype=np.int8)
    nues = tables.slice_nues[scen]
    obs, rew, act = [], [], []
    for t in range(T):
        if marl:
            o = {"player_0": {"observations": host["obs_inter"][t, k].astype(np.float64), "action_mask": mask_inter}}
            for s in range(S):
                o[f"player_{s + 1}"] = {"observations": host["obs_intra"][t, k, s].astype(np.float64),
                                        "action_mask": (np.arange(Us) < nues[s]).astype(np.int8)}
            obs.append(o)
            rew.append({f"player_{j}": float(host["reward"][t, k, j]) for j in range(S + 1)})
            a = {"player_0": host["scores"][t, k].copy()}
            a.update({f"player_{s + 1}": int(host["intra"][t, k, s]) for s in range(S)})
            act.append(a)
        else:
            obs.append(host["obs_inter"][t, k].astype(np.float64))
            rew.append(float(host["reward"][t, k, 0]))
            act.append(host["scores"][t, k].copy())
    rep = lambda a: np.repeat(np.asarray(a)[None], T, axis=0)
    return {
        "pkt_incoming": host["pkt_incoming"][:T, k].astype(np.float64),
        "pkt_throughputs": host["pkt_throughputs"][:T, k].astype(np.float64),
        "pkt_effective_thr": host["pkt_effective_thr"][:T, k].astype(np.float64),
        "buffer_occupancies": q / max_pkts[None, :], "buffer_latencies": lat,
        "dropped_pkts": host["dropped_pkts"][:T, k].astype(np.float64),
        "mobility": np.ones((T, U, 2)), "spectral_efficiencies": se,
        "basestation_ue_assoc": rep(bua), "basestation_slice_assoc": rep(bsa), "slice_ue_assoc": rep(sua),
        "sched_decision": sched, "reward": rew, "slice_req": [req] * T, "obs": obs, "agent_action": act,
    }


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    return type(a) is type(b) and a == b


# ---- header and bindings ------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_library_agree():
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.batched_env import BatchedRanEnv
    from intent_radio_sched_multi_slice_amd.csrc import build
    header = open(os.path.join(REPO, "include", "ranenv.h")).read()
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for fn in ("ranenv_bind_trace", "ranenv_get_trace_counts", "ranenv_reset_trace"):
        assert re.search(r"\bint\s+" + fn + r"\s*\(", header), fn
        assert fn in _lib.FUNCTIONS and fn in _lib.EXPORTS and hasattr(raw, fn), fn
    assert int(re.search(r"#define\s+RANENV_TRACE_BYTES\s+(\d+)", header).group(1)) == ctypes.sizeof(_lib.Trace) == 160
    # the struct's members in the header's order: n_envs, capacity, envs, then the buffers of TRACE_FIELDS
    body = re.search(r"typedef struct \{([^}]*)\} ranenv_trace;", header).group(1)
    members = re.findall(r"\*?\s*(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body))
    assert members == [n for n, _ in _lib.Trace._fields_] == ["n_envs", "capacity", "envs"] + [n for n, _, _ in _lib.TRACE_FIELDS]
    assert re.search(r"#define\s+RANENV_ABI_VERSION\s+%d\b" % _lib.ABI_VERSION, header) and raw.ranenv_abi_version() == _lib.ABI_VERSION
    for method in ("bind_trace", "unbind_trace"):
        assert callable(getattr(BatchedRanEnv, method))


# ---- cutting rows into episodes -----------------------------------------------------------------------------------------------------
def test_episodes_cut_at_done_with_a_trailing_partial_episode():
    from intent_radio_sched_multi_slice_amd.history import TraceEpisode
    tables = _tables()
    # column 0 (env 9): episodes 4, 5 of 3 and 2 rows, then 2 rows of episode 6; column 1 (env 2): episode 5 alone, ending at the
    # last recorded row -- the same numbers in both columns, interleaved in time
    rows = _rows(8, 2, done_at=[(2, 0), (4, 0), (5, 1)])
    rows["episode_number"][:, 0] = [4, 4, 4, 5, 5, 6, 6, 99]
    rows["episode_number"][:, 1] = [5, 5, 5, 5, 5, 5, 99, 99]
    rows["scenario"][:, 0] = [1, 1, 1, 0, 0, 2, 2, 0]
    rows["scenario"][:, 1] = 2
    tr = _trace(rows, [7, 6], [9, 2], tables)               # rows at and behind `count` were never written: not looked at
    assert tr.counts()["count"].tolist() == [7, 6] and tr.counts()["lost"].tolist() == [0, 0]
    assert tr.episodes() == [[TraceEpisode(0, 3, 4, 1, True), TraceEpisode(3, 5, 5, 0, True), TraceEpisode(5, 7, 6, 2, False)],
                             [TraceEpisode(0, 6, 5, 2, True)]]
    assert _trace(rows, [0, 0], [9, 2], tables).episodes() == [[], []]
    assert {k: v.shape[0] for k, v in tr.rows().items()} == {k: 7 for k in rows}


def test_write_names_files_by_the_recorded_episode_number(tmp_path):
    from intent_radio_sched_multi_slice_amd.history import HIST_KEYS, ROW_KEYS, rows_to_hist
    tables = _tables()
    rows = _rows(8, 2, seed=1, done_at=[(2, 0), (4, 0), (5, 1)])
    rows["episode_number"][:, 0] = [4, 4, 4, 5, 5, 6, 6, 0]
    rows["episode_number"][:, 1] = 7
    rows["scenario"][:, 0] = [1, 1, 1, 0, 0, 2, 2, 0]
    rows["scenario"][:, 1] = 2
    tr = _trace(rows, [7, 6], [9, 2], tables)
    paths = tr.write(str(tmp_path), "mult_slice", "mapf")
    assert [os.path.relpath(p, tmp_path) for p in paths] == [os.path.join("hist", "mult_slice", "mapf", f"ep_{n}.npz") for n in (4, 5, 7)]
    assert tr.written == paths                                          # the partial episode 6 is not written
    for path, (lo, hi, col, scen) in zip(paths, [(0, 3, 0, 1), (3, 5, 0, 0), (0, 6, 1, 2)]):
        data = np.load(path, allow_pickle=True)
        assert set(data.files) == set(HIST_KEYS)
        want = rows_to_hist({k: rows[k][lo:hi, col] for k in ROW_KEYS}, tables, scen, R, Us)
        assert data["spectral_efficiencies"].shape == (hi - lo, 1, U, R)
        assert np.array_equal(data["spectral_efficiencies"], want["spectral_efficiencies"])
        assert np.array_equal(data["slice_ue_assoc"][0], tables.to_reference(scen)[2])
        assert [data["reward"][t]["player_0"] for t in range(hi - lo)] == [float(x) for x in rows["reward"][lo:hi, col, 0]]
        assert data["agent_action"][hi - lo - 1]["player_2"] == int(rows["intra"][hi - 1, col, 1])
    # record()'s numbering, for runs without device auto-reset: first number per recorded env, + 1 per complete episode
    paths = tr.write(str(tmp_path / "n"), "mult_slice", "mapf", marl=False, episode_numbers=[20, 30])
    assert [os.path.basename(p) for p in paths] == ["ep_20.npz", "ep_21.npz", "ep_30.npz"]
    assert np.load(paths[0], allow_pickle=True)["reward"].dtype == np.float64          # single-agent files: plain rewards
    # a trace without tiles cannot write
    with pytest.raises(ValueError):
        _trace({k: v for k, v in rows.items() if k != "se"}, [7, 6], [9, 2], tables).write(str(tmp_path / "x"))


# ---- the shared row-to-dict function ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("marl", [True, False])
def test_rows_to_hist_is_what_flush_did(marl):
    from intent_radio_sched_multi_slice_amd.history import HIST_KEYS, ROW_KEYS, rows_to_hist
    tables = _tables()
    host = _rows(6, 3, seed=2)
    for k, T, scen in ((0, 6, 0), (2, 4, 2), (1, 0, 1)):
        want = _flush_before_the_refactor(host, k, T, tables, scen, marl)
        got = rows_to_hist({name: host[name][:T, k] for name in ROW_KEYS}, tables, scen, R, Us, marl)
        assert set(got) == set(want) == set(HIST_KEYS)
        for key in HIST_KEYS:
            assert _same(got[key], want[key]), (k, key)
    assert (host["queue_pkts"] == 0).any() and (host["queue_pkts"] > 0).any()       # both branches of the latency


def test_recorder_and_trace_write_identical_bytes(tmp_path):
    """HistoryRecorder.flush over a numpy-backed DeviceTrace (a stub env hands it out of bind_trace) and DeviceTrace.write on the same
    rows.  The ring's counters stay at zero: flush goes by the recorder's host mirror `t` and reads neither."""
    pytest.importorskip("torch")
    from intent_radio_sched_multi_slice_amd.history import HistoryRecorder
    tables = _tables()
    T, envs = 5, [3, 1]
    rows = _rows(T, 2, seed=3, done_at=[(T - 1, 0), (T - 1, 1)])
    rows["episode_number"][:, 0], rows["episode_number"][:, 1], rows["scenario"][:] = 8, 9, [2, 1]

    class Env:
        B, max_steps, device = 4, T, "cpu"

        def bind_trace(self, which, capacity):
            assert capacity == T
            return _trace(rows, [0, 0], which, tables)

    env = Env()
    env.tables, env.R, env.Us = tables, R, Us
    pb = _trace(rows, [T, T], envs, tables).write(str(tmp_path / "b"), "mult_slice", "mapf")
    # device auto-reset: the ring's episode_number names the file; without: episode_numbers, advanced by one after the write
    for autoreset, first, after in ((True, [0, 0], [0, 0]), (False, [8, 9], [9, 10])):
        env._autoreset = autoreset
        rec = HistoryRecorder(env, envs, str(tmp_path / f"a{autoreset:d}"), "mult_slice", "mapf", episode_numbers=first)
        assert rec.T == T and rec.envs == envs and rec.t.tolist() == [0, 0] and rec.flush() == []
        rec.t[:] = T
        pa = rec.flush()
        assert rec.written == pa and rec.episode_numbers == after
        assert [os.path.basename(p) for p in pa] == [os.path.basename(p) for p in pb] == ["ep_8.npz", "ep_9.npz"]
        for x, y in zip(pa, pb):
            assert open(x, "rb").read() == open(y, "rb").read()


def test_reset_of_one_column_leaves_the_others(tmp_path):
    """DeviceTrace.reset(columns): three columns with 4, 2 and 3 rows, column 1 restarted, two more rows recorded in every column
    (the test plays the device: a row goes to row count[i] of column i)."""
    from intent_radio_sched_multi_slice_amd.history import ROW_KEYS, TraceEpisode, rows_to_hist
    tables = _tables()
    rows = _rows(8, 3, seed=6, done_at=[(3, 0), (2, 2)])
    more = _rows(2, 3, seed=7, done_at=[(1, 1), (1, 2)])
    rows["episode_number"][:], rows["scenario"][:] = [4, 6, 7], [1, 0, 2]
    more["episode_number"][:], more["scenario"][:] = [5, 9, 8], [0, 2, 1]
    before = {k: v.copy() for k, v in rows.items()}
    count, lost = np.asarray([4, 2, 3], dtype=np.int32), np.asarray([0, 5, 1], dtype=np.int32)
    tr = _trace(rows, count, [7, 3, 5], tables, lost=lost)
    tr.reset([1])
    assert tr.counts()["count"].tolist() == [4, 0, 3] and tr.counts()["lost"].tolist() == [0, 0, 1]
    assert tr.episodes()[1] == []
    for j in range(2):
        for i in range(3):
            for k in rows:
                rows[k][count[i], i] = more[k][j, i]
            count[i] += 1
    assert tr.counts()["count"].tolist() == [6, 2, 5]
    assert tr.episodes() == [[TraceEpisode(0, 4, 4, 1, True), TraceEpisode(4, 6, 5, 0, False)],
                             [TraceEpisode(0, 2, 9, 2, True)],
                             [TraceEpisode(0, 3, 7, 2, True), TraceEpisode(3, 5, 8, 1, True)]]
    for k in rows:                                         # columns 0 and 2 kept what they had; column 1 starts again at row 0
        assert np.array_equal(rows[k][:4, 0], before[k][:4, 0]) and np.array_equal(rows[k][:3, 2], before[k][:3, 2]), k
        assert np.array_equal(rows[k][:2, 1], more[k][:, 1]), k
    paths = tr.write(str(tmp_path), "mult_slice", "mapf")
    assert [os.path.basename(p) for p in paths] == ["ep_4.npz", "ep_9.npz", "ep_7.npz", "ep_8.npz"]
    for path, src, scen in zip(paths, ({k: before[k][:4, 0] for k in ROW_KEYS}, {k: more[k][:, 1] for k in ROW_KEYS},
                                       {k: before[k][:3, 2] for k in ROW_KEYS}, {k: more[k][:, 2] for k in ROW_KEYS}), (1, 2, 2, 1)):
        data, want = np.load(path, allow_pickle=True), rows_to_hist(src, tables, scen, R, Us)
        for key in ("spectral_efficiencies", "pkt_incoming", "sched_decision", "slice_ue_assoc"):
            assert np.array_equal(data[key], want[key]), (path, key)
        assert [data["reward"][t]["player_0"] for t in range(len(want["reward"]))] == [r["player_0"] for r in want["reward"]]
    tr.reset()                                             # no columns: everything, as before
    assert tr.counts()["count"].tolist() == [0, 0, 0] and tr.counts()["lost"].tolist() == [0, 0, 0]


# ---- a planted slip -----------------------------------------------------------------------------------------------------------------
def test_a_tile_one_tti_late_fails_the_file_comparison(tmp_path):
    """tests/test_gpu_trace.py compares the files of the two producers key by key.  Rows whose SE is the NEXT TTI's tile must fail
    that comparison -- which they do because consecutive tiles differ, the condition that test asserts on its reference files; with
    one tile repeated (a channel trace of length 1) the same slip would pass unseen."""
    pytest.importorskip("torch")
    from tests.test_gpu_trace import _assert_same_files
    tables = _tables()
    T = 6
    rows = _rows(T, 1, seed=5, done_at=[(T - 1, 0)])
    good = _trace(rows, [T], [0], tables).write(str(tmp_path / "good"))[0]
    assert _assert_same_files(good, _trace(dict(rows), [T], [0], tables).write(str(tmp_path / "again"))[0]) is not None
    late = dict(rows, se=np.roll(rows["se"], -1, axis=0))
    with pytest.raises(AssertionError, match="spectral_efficiencies"):
        _assert_same_files(good, _trace(late, [T], [0], tables).write(str(tmp_path / "late"))[0])
    blank = dict(rows, dropped_pkts=np.zeros_like(rows["dropped_pkts"]))
    with pytest.raises(AssertionError, match="dropped_pkts"):
        _assert_same_files(good, _trace(blank, [T], [0], tables).write(str(tmp_path / "blank"))[0])
    # without the condition: every TTI the same tile
    flat = dict(rows, se=np.repeat(rows["se"][:1], T, axis=0))
    same = _trace(flat, [T], [0], tables).write(str(tmp_path / "flat"))[0]
    late = dict(flat, se=np.roll(flat["se"], -1, axis=0))
    _assert_same_files(same, _trace(late, [T], [0], tables).write(str(tmp_path / "flat_late"))[0])
