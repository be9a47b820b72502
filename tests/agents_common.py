"""Agents that speak the reference's IBSched protocol with the oracle's agent-side arithmetic, and the replay of
tests/golden/agents_on_facade.npz through the facade: shared by the GPU modules (the HIP env step under the facade) and the CPU
ones (a CPU stand-in under it).  Numpy only."""
import json

import numpy as np

from tests.common import OBS_TOL, REW_TOL, load_golden


class OracleIBSched:
    """IBSched (agents/ib_sched.py) with the oracle's agent-side functions behind the reference's method names."""

    def __init__(self, env, max_number_ues, max_number_slices, max_number_basestations, num_available_rbs, seed=0,
                 max_ues_slice=5, rbs_per_rbg=1):
        from oracle import pyoracle
        self.env = env
        self.max_number_ues, self.max_number_slices = max_number_ues, max_number_slices
        self.max_number_basestations, self.num_available_rbs = max_number_basestations, num_available_rbs
        ce = env.comm_env
        self.S, self.U, self.R, self.Us = max_number_slices, max_number_ues, int(num_available_rbs[0]), max_ues_slice
        self.cfg = pyoracle.make_cfg(self.S, self.U, self.R, rbs_per_rbg, self.Us, bandwidth_hz=float(ce.bandwidths[0]),
                                     max_steps=ce.max_number_steps)
        self.orc = pyoracle.OracleEnv(self.cfg)
        self._scenario_key = None
        self.last_sched = np.zeros((1, self.U, self.R))

    def _sync_scenario(self, raw):
        """slice_req / associations come with the raw observation; buffer parameters are read off
        env.comm_env.ues (agents/common.py:581-582,591)."""
        from intent_radio_sched_multi_slice_amd.scenario import ScenarioTables
        ues = self.env.comm_env.ues
        key = (raw["slice_ue_assoc"].tobytes(), ues.pkt_sizes.tobytes(), ues.max_buffer_pkts.tobytes())
        if key != self._scenario_key:
            t = ScenarioTables.empty(1, self.S, self.U, self.Us)
            t.set_from_reference(0, raw["basestation_slice_assoc"], raw["slice_ue_assoc"], raw["slice_req"], True,
                                 (ues.pkt_sizes, ues.max_buffer_pkts, np.array([b.max_packets_age for b in ues.buffers])))
            self.tables = t
            self.orc.set_scenario(t, 0)
            self._scenario_key = key

    def obs_space_format(self, raw):
        self._sync_scenario(raw)
        self.orc.agent_observe(raw["pkt_effective_thr"], raw["dropped_pkts"], raw["buffer_occupancies"],
                               raw["buffer_latencies"], raw["spectral_efficiencies"][0].astype(np.float32),
                               raw["sched_decision"][0].sum(axis=1))
        o = self.orc.obs()
        out = {"player_0": {"observations": o["obs_inter"], "action_mask": o["mask_inter"]}}
        for s in range(self.S):
            out[f"player_{s + 1}"] = {"observations": o["obs_intra"][s], "action_mask": o["mask_intra"][s]}
        self._last = o
        return out

    def calculate_reward(self, obs):
        return {f"player_{i}": float(self._last["reward"][i]) for i in range(self.S + 1)}

    def action_format(self, action):
        scores = np.asarray(action["player_0"], dtype=np.float64)
        intra = np.array([int(action[f"player_{s + 1}"]) for s in range(self.S)], dtype=np.int32)
        _, _, dense = self.orc.action_format(scores, intra, want_dense=True)
        return dense[None].astype(np.float64)

    def step(self, obs, t):
        """A policy: MAPF scores (agents/mapf.py:41-111), intra-slice scheduler cycling through RR / PF / MT."""
        a = {"player_0": self.orc.policy_mapf()}
        a.update({f"player_{s + 1}": (s + t) % 3 for s in range(self.S)})
        return a


class _Agent(OracleIBSched):
    """IBSched's protocol; ``sort`` = enable_sort_slices (MARR / MAPF wrap an IBSched built with it off, agents/marr.py:30-37)."""

    def __init__(self, *a, sort=True, **k):
        super().__init__(*a, **k)
        self._sort = sort

    def _sync_scenario(self, raw):
        from intent_radio_sched_multi_slice_amd.scenario import ScenarioTables
        ues = self.env.comm_env.ues
        key = (raw["slice_ue_assoc"].tobytes(), ues.pkt_sizes.tobytes(), ues.max_buffer_pkts.tobytes())
        if key != self._scenario_key:
            t = ScenarioTables.empty(1, self.S, self.U, self.Us)
            t.set_from_reference(0, raw["basestation_slice_assoc"], raw["slice_ue_assoc"], raw["slice_req"], self._sort,
                                 (ues.pkt_sizes, ues.max_buffer_pkts, np.array([b.max_packets_age for b in ues.buffers])))
            self.tables = t
            self.orc.set_scenario(t, 0)
            self._scenario_key = key


def replay_fixture(name, tmp_path):
    """The fixture's actions through the facade, whatever env core is under it (tests/test_gpu_reference_agents.py: the HIP
    step; tests/test_reference_agents_cpu.py: the CPU stand-in)."""
    from intent_radio_sched_multi_slice_amd import plugins
    from intent_radio_sched_multi_slice_amd.comm_env import DEFAULT_CONFIGS, MARLCommEnv
    fx = load_golden("agents_on_facade")
    S, U, R, G, Us, seed, steps = (int(x) for x in fx["cfg"])
    cfg = dict(DEFAULT_CONFIGS["mult_slice"], max_number_steps=steps)
    env = MARLCommEnv(plugins.MimicQuadriga, plugins.MultSliceTraffic, plugins.SimpleMobility, plugins.MultSliceAssociation,
                      "mult_slice", name, seed, root_path=str(tmp_path), config=cfg, max_episode_number=2, max_ues_slice=Us)
    ce = env.comm_env
    marl = name == "ib_sched"
    agent = _Agent(env, ce.max_number_ues, ce.max_number_slices, ce.max_number_basestations, ce.num_available_rbs,
                   max_ues_slice=Us, rbs_per_rbg=G, sort=marl)
    env.set_agent_functions(agent.obs_space_format, agent.action_format, agent.calculate_reward, None, None)
    fixed = {"ib_sched": None, "marr": 0, "mapf": 1}[name]      # MARR: fixed_intra "rr" (marr.py:62-70), MAPF: "pf" (mapf.py:126-134)

    def flat(o):
        if marl:
            return (np.concatenate([o["player_0"]["observations"]] + [o[f"player_{s + 1}"]["observations"] for s in range(S)]),
                    np.concatenate([o["player_0"]["action_mask"]] + [o[f"player_{s + 1}"]["action_mask"] for s in range(S)]))
        return np.asarray(o["player_0"]["observations"]), None

    obs, _ = env.reset(seed=seed, options={"initial_episode": 0})
    assert np.array_equal(ce.slice_ue_assoc, fx[f"{name}_slice_ue_assoc"])
    assert {k: (v["name"] if v else None) for k, v in ce.slice_req.items()} == json.loads(str(fx[f"{name}_slice_names"]))
    assert np.array_equal(np.stack([ce.ues.pkt_sizes, ce.ues.max_buffer_pkts, ce.ues.max_buffer_latencies]), fx[f"{name}_ues"])
    o, m = flat(obs)
    np.testing.assert_allclose(o, fx[f"{name}_reset_obs"], rtol=0, atol=OBS_TOL)
    if marl:
        assert np.array_equal(m, fx[f"{name}_reset_mask"])
    for t in range(steps):
        a = fx[f"{name}_action"][t]
        action = {"player_0": a[:S].copy()}
        action.update({f"player_{s + 1}": int(a[S + s]) if marl else fixed for s in range(S)})
        obs, reward, term, trunc, info = env.step(action)
        raw = env._last_raw
        sched = np.asarray(raw["sched_decision"])[0]
        cnt = sched.sum(axis=1).astype(np.int32)
        assert np.array_equal(cnt, fx[f"{name}_rb_count"][t]), (name, t)
        st = np.array([int(np.nonzero(sched[u])[0][0]) if cnt[u] else 0 for u in range(U)])
        assert np.array_equal(st, fx[f"{name}_rb_start"][t]), (name, t)
        assert np.array_equal(env._last_traffic, fx[f"{name}_traffic"][t]), (name, t)
        np.testing.assert_array_equal(np.asarray(raw["spectral_efficiencies"])[0].sum(axis=1), fx[f"{name}_se_sum"][t])
        for k in ("pkt_incoming", "pkt_throughputs", "pkt_effective_thr", "dropped_pkts", "buffer_occupancies", "buffer_latencies"):
            assert np.array_equal(raw[k], fx[f"{name}_{k}"][t]), (name, t, k)
        o, m = flat(obs)
        np.testing.assert_allclose(o, fx[f"{name}_obs"][t], rtol=0, atol=OBS_TOL, err_msg=str((name, t)))
        if marl:
            assert np.array_equal(m, fx[f"{name}_mask"][t])
            rw = np.array([reward[f"player_{i}"] for i in range(S + 1)])
        else:
            rw = np.array([reward["player_0"]])
        np.testing.assert_allclose(rw, fx[f"{name}_reward"][t], rtol=0, atol=REW_TOL, err_msg=str((name, t)))
    assert term["__all__"]
    env.close()
