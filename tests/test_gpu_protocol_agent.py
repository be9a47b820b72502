"""INTEGRATION.md section 2 as a test: an agent that speaks the reference's IBSched protocol (dict observations
keyed ``player_i``, ``action_format(action)`` returning the dense ``(1, U, R)`` sched_decision, PF reading the UE
buffer parameters off ``env.comm_env.ues``; agents/ib_sched.py:60-63,206,223, simu.py:405-418) attaches to
MARLCommEnv unchanged and, over two episodes, produces bit for bit what a pure CPU closed loop produces.

The agent's arithmetic is the oracle's agent side (oracle/ranenv_oracle.c, pinned by the reference-produced
goldens); the env core under the facade is the HIP kernel.  A second oracle env runs the whole loop on the CPU."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.agents_common import OracleIBSched
from tests.gpu_common import need_gpu

pytestmark = pytest.mark.gpu


def test_ibsched_protocol_agent_through_the_facade_matches_a_cpu_closed_loop(tmp_path):
    need_gpu()
    from intent_radio_sched_multi_slice_amd import plugins
    from intent_radio_sched_multi_slice_amd.comm_env import DEFAULT_CONFIGS, MARLCommEnv
    from intent_radio_sched_multi_slice_amd.history import HIST_KEYS
    from oracle import pyoracle
    steps = 40
    cfg = dict(DEFAULT_CONFIGS["mult_slice"], max_number_steps=steps)
    env = MARLCommEnv(plugins.MimicQuadriga, plugins.MultSliceTraffic, plugins.SimpleMobility, plugins.MultSliceAssociation,
                      "mult_slice", "oracle_ib_sched", 10, root_path=str(tmp_path), config=cfg, max_episode_number=3,
                      max_ues_slice=5, save_hist=True)
    ce = env.comm_env
    agent = OracleIBSched(env, ce.max_number_ues, ce.max_number_slices, ce.max_number_basestations, ce.num_available_rbs)
    env.set_agent_functions(agent.obs_space_format, agent.action_format, agent.calculate_reward, None, None)   # simu.py:405-411
    ref = pyoracle.OracleEnv(agent.cfg)                     # the pure CPU loop: env core + agent side in one oracle env
    for episode in range(2):
        obs, _ = env.reset(seed=10) if episode == 0 else env.reset()
        # IBSched never clears its 10-TTI deque (agents/ib_sched.py:51): the CPU loop keeps its window too
        ref.set_scenario(agent.tables, 0)
        ref.reset(env._last_se32)
        ro = ref.obs()
        assert np.array_equal(obs["player_0"]["observations"], ro["obs_inter"])
        terminated, t = False, 0
        while not terminated:
            action = agent.step(obs, t)
            obs, reward, term, trunc, info = env.step(action)
            terminated = term["__all__"]
            intra = np.array([action[f"player_{s + 1}"] for s in range(agent.S)], dtype=np.int32)
            ref.step(action["player_0"], intra, env._last_se32, env._last_traffic)
            rr, ro = ref.raw(), ref.obs()
            raw = env._last_raw
            for k in ("pkt_incoming", "pkt_throughputs", "pkt_effective_thr", "dropped_pkts", "buffer_occupancies",
                      "buffer_latencies"):
                assert np.array_equal(raw[k], rr[k]), (episode, t, k)
            assert np.array_equal(obs["player_0"]["observations"], ro["obs_inter"]), (episode, t)
            assert np.array_equal(obs["player_0"]["action_mask"], ro["mask_inter"])
            for s in range(agent.S):
                assert np.array_equal(obs[f"player_{s + 1}"]["observations"], ro["obs_intra"][s]), (episode, t, s)
                assert np.array_equal(obs[f"player_{s + 1}"]["action_mask"], ro["mask_intra"][s])
            assert [reward[f"player_{i}"] for i in range(agent.S + 1)] == ro["reward"].tolist(), (episode, t)
            assert set(term) == set(reward) | {"__all__"}
            t += 1
        assert t == steps
        # save_hist=True wrote the episode in the reference's schema (results/gen_results.py:88-108)
        data = np.load(tmp_path / "hist" / "mult_slice" / "oracle_ib_sched" / f"ep_{ce.episode_number}.npz", allow_pickle=True)
        assert set(data.files) == set(HIST_KEYS)
        assert data["pkt_effective_thr"].shape == (steps, ce.max_number_ues)
        assert data["spectral_efficiencies"].shape == (steps, 1, ce.max_number_ues, 135)
        assert data["sched_decision"].shape == (steps, 1, ce.max_number_ues, 135)
        assert data["slice_ue_assoc"].shape == (steps, ce.max_number_slices, ce.max_number_ues)
        assert data["reward"][steps - 1]["player_0"] == reward["player_0"]
        assert data["slice_req"][3]["slice_0"] == ce.slice_req["slice_0"] or data["slice_req"][3]["slice_0"] == {}
        assert np.array_equal(data["agent_action"][steps - 1]["player_0"], action["player_0"])
    env.close()
