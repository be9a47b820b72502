"""History files: ``hist/{scenario}/{agent}/ep_{n}.npz`` with the 16 keys the reference's result scripts read
(results/gen_results.py:88-108: ``np.load(..., allow_pickle=True)`` then ``data[key]`` for every key below; per-step
arrays are indexed ``[step, ...]``, ``spectral_efficiencies`` and ``sched_decision`` carry the base-station axis
``(steps, 1, U, R)`` (:262-265, :629), ``slice_ue_assoc`` is ``(steps, S, U)`` (:279), ``reward[idx]["player_0"]`` for
multi-agent runs (:162), ``slice_req[step]["slice_k"]`` dicts (:422-426)).

Two producers: the B = 1 facade (comm_env.MARLCommEnv, ``save_hist=True``), and DeviceTrace, the ring a kernel of the library fills
behind every step of whatever call steps selected envs of a BatchedRanEnv (``rollout``, ``evaluate``, ``collect*``, ``step``), cut
into episodes and written afterwards by ``write()`` -- or, under ``step()`` only, at the TTI an episode ends by HistoryRecorder
(``BatchedRanEnv.record``), which paces such a ring from the host.  Both ways the recorded rows of one env's episode become the
16-key dict in ``rows_to_hist``.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence

import numpy as np

HIST_KEYS = ("pkt_incoming", "pkt_throughputs", "pkt_effective_thr", "buffer_occupancies", "buffer_latencies",
             "dropped_pkts", "mobility", "spectral_efficiencies", "basestation_ue_assoc", "basestation_slice_assoc",
             "slice_ue_assoc", "sched_decision", "reward", "slice_req", "obs", "agent_action")
OBJECT_KEYS = ("slice_req", "obs", "reward", "agent_action")


def hist_path(root_path: str, simu_name: str, agent_name: str, episode: int) -> str:
    return os.path.join(root_path, "hist", simu_name, agent_name, f"ep_{episode}.npz")


def write_episode_npz(path: str, hist: Dict[str, Sequence]) -> str:
    """``hist[key]`` = one entry per step.  Dict-valued keys go into object arrays (one dict per step), the rest
    become dense arrays ``(steps, ...)``."""
    missing = [k for k in HIST_KEYS if k not in hist]
    if missing:
        raise ValueError(f"history is missing {missing}")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    out = {}
    for k in HIST_KEYS:
        v = hist[k]
        if k in OBJECT_KEYS and len(v) and isinstance(v[0], dict):
            a = np.empty(len(v), dtype=object)
            for i, x in enumerate(v):
                a[i] = x
            out[k] = a
        else:
            out[k] = np.asarray(v)
    np.savez_compressed(path, **out)
    return path


# what a history file takes from a recorded row of DeviceTrace's ring (the ring adds DeviceTrace.BOOKKEEPING)
ROW_KEYS = ("pkt_incoming", "pkt_throughputs", "pkt_effective_thr", "dropped_pkts", "queue_pkts", "queue_age_sum", "rb_start",
            "rb_count", "se", "reward", "scores", "intra", "obs_inter", "obs_intra")


def rows_to_hist(rows: Dict[str, np.ndarray], tables, scen: int, R: int, Us: int, marl: bool = True) -> Dict[str, Sequence]:
    """The 16-key history dict (``write_episode_npz``'s input) of ONE env's episode from its recorded rows on the host:
    ``rows[k]`` = ``[T, ...]`` for every k of ROW_KEYS (``se`` RB-major ``[T, R, U]``), played on scenario-pool row ``scen`` of
    ``tables``."""
    T = len(rows["reward"])
    S, U = tables.n_slices, tables.n_ues
    bua, bsa, sua, req = tables.to_reference(scen)
    max_pkts = tables.ue_max_pkts[scen].astype(np.float64)
    q = rows["queue_pkts"][:T].astype(np.float64)
    age = rows["queue_age_sum"][:T].astype(np.float64)
    lat = np.where(q > 0, age / np.maximum(q, 1.0), 0.0)
    st, cn = rows["rb_start"][:T], rows["rb_count"][:T]
    r = np.arange(R)[None, None, :]
    sched = ((r >= st[:, :, None]) & (r < (st + cn)[:, :, None])).astype(np.float64)[:, None]   # (T, 1, U, R)
    se = np.swapaxes(rows["se"][:T], 1, 2).astype(np.float64)[:, None]                           # (T, 1, U, R)
    mask_inter = np.asarray(tables.slice_active[scen], dtype=np.int8)
    nues = tables.slice_nues[scen]
    obs, rew, act = [], [], []
    for t in range(T):
        if marl:
            o = {"player_0": {"observations": rows["obs_inter"][t].astype(np.float64), "action_mask": mask_inter}}
            for s in range(S):
                o[f"player_{s + 1}"] = {"observations": rows["obs_intra"][t, s].astype(np.float64),
                                        "action_mask": (np.arange(Us) < nues[s]).astype(np.int8)}
            obs.append(o)
            rew.append({f"player_{j}": float(rows["reward"][t, j]) for j in range(S + 1)})
            a = {"player_0": rows["scores"][t].copy()}
            a.update({f"player_{s + 1}": int(rows["intra"][t, s]) for s in range(S)})
            act.append(a)
        else:
            obs.append(rows["obs_inter"][t].astype(np.float64))
            rew.append(float(rows["reward"][t, 0]))
            act.append(rows["scores"][t].copy())
    rep = lambda a: np.repeat(np.asarray(a)[None], T, axis=0)
    return {
        "pkt_incoming": rows["pkt_incoming"][:T].astype(np.float64),
        "pkt_throughputs": rows["pkt_throughputs"][:T].astype(np.float64),
        "pkt_effective_thr": rows["pkt_effective_thr"][:T].astype(np.float64),
        "buffer_occupancies": q / max_pkts[None, :], "buffer_latencies": lat,
        "dropped_pkts": rows["dropped_pkts"][:T].astype(np.float64),
        "mobility": np.ones((T, U, 2)), "spectral_efficiencies": se,
        "basestation_ue_assoc": rep(bua), "basestation_slice_assoc": rep(bsa), "slice_ue_assoc": rep(sua),
        "sched_decision": sched, "reward": rew, "slice_req": [req] * T, "obs": obs, "agent_action": act,
    }


class HistoryRecorder:
    """``BatchedRanEnv.record``: the host pacer of a DeviceTrace of the listed envs (bound here, one ring row per TTI of the longest
    episode among them when recording starts).  Under ``step()`` it reads the recorded envs' ``done`` every TTI, writes a
    reference-format history file at the TTI an env's episode ends and restarts that env's column of the ring.

    Every recorded env has its own step counter ``t`` (a host mirror of the ring's row count): envs may be reset under a mask, run
    episodes of different lengths (``set_max_steps``) or move on to their next episode on the device (``enable_autoreset``: the
    file is then named by the episode number the ring recorded).  ``episode_numbers[i]`` is the episode number env ``envs[i]`` is
    playing when recording starts; without device auto-reset it names the file and is advanced by one after every write.
    Association / intent columns come from the scenario pool row the ring recorded; the agent action recorded is the inter-slice
    score vector and the intra-slice schedulers the step used.
    """

    def __init__(self, env, envs: Sequence[int], root_path: str = ".", simu_name: str = "mult_slice",
                 agent_name: str = "agent", episode_numbers: Optional[Sequence[int]] = None, marl: bool = True):
        import torch
        self.env = env
        self.envs = [int(e) for e in envs]
        if any(e < 0 or e >= env.B for e in self.envs):
            raise ValueError("recorded env index outside the batch")
        self.root_path, self.simu_name, self.agent_name, self.marl = root_path, simu_name, agent_name, marl
        self.episode_numbers = list(episode_numbers) if episode_numbers is not None else [0] * len(self.envs)
        me = getattr(env, "max_steps_env", None)
        self.T = int(env.max_steps if me is None else np.asarray(me)[self.envs].max())
        self.trace = env.bind_trace(self.envs, capacity=self.T)
        self.idx = torch.as_tensor(self.envs, dtype=torch.int64, device=env.device)
        self.t = np.zeros(len(self.envs), dtype=np.int64)    # steps recorded of every slot's current episode
        self.written: List[str] = []

    def _restart(self, slots: Sequence[int]):
        if len(slots):
            self.trace.reset(slots)
            self.t[slots] = 0

    def on_reset(self, env_mask=None):
        """Called by BatchedRanEnv.reset: the masked envs (all without a mask) start an episode; what was recorded of
        their unfinished one is dropped."""
        m = np.ones(len(self.envs)) if env_mask is None else env_mask.index_select(0, self.idx).cpu().numpy()
        self._restart(np.nonzero(m)[0].tolist())

    def on_step(self, done):
        """Called by BatchedRanEnv.step after the launch (and before an auto-reset is enqueued)."""
        if (self.t >= self.T).any():
            raise RuntimeError("recorder: an env ran past the longest episode length known when recording started "
                               "(set_max_steps after record()?)")
        self.t += 1
        which = np.nonzero(done.index_select(0, self.idx).cpu().numpy())[0].tolist()      # recording is a diagnostic mode: one small sync
        if which:
            self.flush(which)
            self._restart(which)

    def flush(self, which: Optional[Sequence[int]] = None) -> List[str]:
        """Write the steps recorded so far of the current episode of recorder slots ``which`` (all by default; a slot with none
        is passed over)."""
        env = self.env
        which = [k for k in (range(len(self.envs)) if which is None else which) if self.t[k] > 0]
        rows = self.trace.rows(n=int(self.t[which].max(initial=0)))
        paths = []
        for k in which:
            T = int(self.t[k])
            number = int(rows["episode_number"][T - 1, k]) if env._autoreset else self.episode_numbers[k]
            hist = rows_to_hist({name: rows[name][:T, k] for name in ROW_KEYS}, env.tables, int(rows["scenario"][T - 1, k]), env.R, env.Us,
                                self.marl)
            paths.append(write_episode_npz(hist_path(self.root_path, self.simu_name, self.agent_name, number), hist))
            if not env._autoreset:
                self.episode_numbers[k] += 1
        self.written += paths
        return paths


class TraceEpisode(NamedTuple):
    """Rows [start, stop) of one recorded env's column: one episode, or -- ``complete`` False -- what was recorded of one that had
    not ended (the rows behind the last ``done``)."""
    start: int
    stop: int
    episode_number: int
    scenario: int
    complete: bool


def cut_episodes(done: np.ndarray, episode_number: np.ndarray, scenario: np.ndarray) -> List[TraceEpisode]:
    """One env's recorded rows cut at ``done``: every row with the flag set ends an episode, which takes its number and scenario
    from that row (the finished episode's: the device installs the next one behind it)."""
    out, start = [], 0
    for t in np.nonzero(np.asarray(done))[0]:
        out.append(TraceEpisode(start, int(t) + 1, int(episode_number[t]), int(scenario[t]), True))
        start = int(t) + 1
    if start < len(done):
        out.append(TraceEpisode(start, len(done), int(episode_number[start]), int(scenario[start]), False))
    return out


class DeviceTrace:
    """The ring of ``BatchedRanEnv.bind_trace``: ``buffers[k]`` = ``[capacity, n_envs, ...]`` (torch tensors the library's trace
    kernel writes; numpy arrays work as well: the host side below only reads them), column i = env ``envs[i]``, row k = that env's
    k-th recorded TTI.  ``counts_fn() -> (count, lost)``: rows written / rows that did not fit, per recorded env."""

    BOOKKEEPING = ("step_number", "episode_number", "scenario", "done")

    def __init__(self, envs: Sequence[int], capacity: int, buffers: Dict[str, object], counts_fn: Callable, tables, R: int, Us: int,
                 guard: Optional[Dict[str, object]] = None, reset_fn: Optional[Callable] = None):
        self.envs = [int(e) for e in envs]
        self.capacity = int(capacity)
        self.buffers, self.guard = buffers, guard or {}
        self._counts_fn, self._reset_fn = counts_fn, reset_fn
        self.tables, self.R, self.Us = tables, int(R), int(Us)
        self.written: List[str] = []

    def counts(self) -> Dict[str, np.ndarray]:
        """``{"count", "lost"}``: int32 [n_envs] on the host (one small device-to-host copy)."""
        count, lost = self._counts_fn()
        return {"count": np.asarray(count, dtype=np.int32), "lost": np.asarray(lost, dtype=np.int32)}

    def reset(self, columns: Optional[Sequence[int]] = None) -> None:
        """Start again at row 0 of every column, or of the listed ones only (count and lost zeroed on the device, in stream order;
        the rows stay until overwritten)."""
        if self._reset_fn is None:
            raise RuntimeError("this trace has no device ring to reset")
        self._reset_fn(columns)

    def rows(self, names: Optional[Sequence[str]] = None, n: Optional[int] = None) -> Dict[str, np.ndarray]:
        """Host copies of the first ``n`` rows (default: max(count), one more small copy to learn it) of the named buffers (all by
        default)."""
        n = int(self.counts()["count"].max(initial=0)) if n is None else n
        out = {}
        for k in (self.buffers if names is None else names):
            b = self.buffers[k][:n]
            out[k] = b.cpu().numpy() if hasattr(b, "cpu") else np.asarray(b)
        return out

    def episodes(self, rows: Optional[Dict[str, np.ndarray]] = None) -> List[List[TraceEpisode]]:
        """Per recorded env the row ranges of its episodes, cut at ``done``; a trailing unfinished one has ``complete=False``."""
        missing = [k for k in self.BOOKKEEPING[1:] if k not in self.buffers]
        if missing:
            raise ValueError(f"the trace does not record {missing}")
        rows = self.rows(self.BOOKKEEPING[1:]) if rows is None else rows
        count = self.counts()["count"]
        return [cut_episodes(rows["done"][:count[i], i], rows["episode_number"][:count[i], i], rows["scenario"][:count[i], i])
                for i in range(len(self.envs))]

    def write(self, root_path: str = ".", simu_name: str = "mult_slice", agent_name: str = "agent", marl: bool = True,
              episode_numbers: Optional[Sequence[int]] = None) -> List[str]:
        """One reference-format npz per COMPLETE recorded episode, ``hist/{simu_name}/{agent_name}/ep_{episode_number}.npz`` with
        the number the device recorded.  ``episode_numbers`` (as ``record()``'s, for runs without device auto-reset, where the
        device's episode counter does not move): recorded env i's j-th complete episode is named ``episode_numbers[i] + j``
        instead.  Returns the paths, per env in episode order (also appended to ``.written``)."""
        missing = [k for k in ROW_KEYS if k not in self.buffers]
        if missing:
            raise ValueError(f"the trace does not record {missing}: no history file can be written from it")
        rows = self.rows()
        paths = []
        for i, eps in enumerate(self.episodes(rows)):
            for j, ep in enumerate(x for x in eps if x.complete):
                number = ep.episode_number if episode_numbers is None else int(episode_numbers[i]) + j
                hist = rows_to_hist({k: rows[k][ep.start:ep.stop, i] for k in ROW_KEYS}, self.tables, ep.scenario, self.R, self.Us, marl)
                paths.append(write_episode_npz(hist_path(root_path, simu_name, agent_name, number), hist))
        self.written += paths
        return paths
