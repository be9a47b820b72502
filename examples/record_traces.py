"""Per-TTI history files (hist/{scenario}/{agent}/ep_N.npz, the 16 keys every plot of results/gen_results.py reads) taken from a
run that never returns to the host between two TTIs:

    python examples/record_traces.py [--batch 1024] [--episodes 2] [--steps 100] [--traced 8] [--out /tmp/traces]

MAPF + proportional fairness plays --episodes episodes per env in ONE evaluate(); a device trace (BatchedRanEnv.bind_trace) records
--traced of the envs behind every step, the device's auto-reset included.  Afterwards the ring is cut into episodes at the recorded
`done` flags and written in the reference's format, and two quantities are recomputed from the files the way gen_results.py does
-- the inter-slice agent's episode return (reward[t]["player_0"], :162) and the packets sent (pkt_effective_thr over the UEs of
the slices, calc_total_throughput :791-809, before the message sizes) -- and compared with the episode sums the device kept
itself (evaluate()'s "reward" and "pkts_sent").  Synthetic scenarios / channels of the reference's laws: the real datasets are not
shipped.
"""
import argparse
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from intent_radio_sched_multi_slice_amd import _lib
from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--episodes", type=int, default=2)
    ap.add_argument("--steps", type=int, default=100, help="TTIs per episode")
    ap.add_argument("--traced", type=int, default=8, help="envs whose history is recorded")
    ap.add_argument("--out", default=None, help="root of the hist/ tree (default: a temporary directory)")
    args = ap.parse_args()
    B, n_ep, T = args.batch, args.episodes, args.steps
    wl = make_mult_slice_workload(B, torch.device("cuda", 0), policy=_lib.POLICY_MAPF, intra=_lib.INTRA_PF, n_scenarios=64, n_traces=64,
                                  trace_len=T, max_steps=T)
    env = wl.env
    eps = env.episodes
    env.set_episode_table(scenario=eps["scenario"], se_base=eps["se_base"], se_len=eps["se_len"], se_offset=eps["se_offset"],
                          trf_base=eps["trf_base"], trf_len=eps["trf_len"], trf_offset=eps["trf_offset"])
    env.enable_autoreset(0, B, episode_numbers=np.arange(B, dtype=np.int32))
    env.enable_metrics(n_ep)
    # (env e plays episodes e, e + 1, ...: traced envs at least --episodes apart, and none that wraps around the table, name every file once)
    traced = sorted({int(e) for e in np.linspace(0, max(0, B - 1 - n_ep), args.traced).round()})
    trace = env.bind_trace(traced, n_ep * T)
    res = env.evaluate(n_ep)
    counts = trace.counts()
    root = args.out or tempfile.mkdtemp(prefix="traces_")
    paths = trace.write(root, "mult_slice", "mapf")
    ring_mb = sum(b.numel() * b.element_size() for b in trace.buffers.values()) / 2 ** 20
    print(f"{B} envs x {n_ep} episodes of {T} TTIs; {len(traced)} envs traced into a ring of {ring_mb:.1f} MiB "
          f"(rows written {counts['count'].tolist()}, lost {counts['lost'].tolist()})")
    print(f"{len(paths)} history files under {os.path.join(root, 'hist', 'mult_slice', 'mapf')}")
    worst = 0.0
    per_env = trace.episodes()
    for i, e in enumerate(traced):
        for j, ep in enumerate(x for x in per_env[i] if x.complete):
            data = np.load(os.path.join(root, "hist", "mult_slice", "mapf", f"ep_{ep.episode_number}.npz"), allow_pickle=True)
            ret = sum(r["player_0"] for r in data["reward"])
            sent = sum(float(np.sum(data["pkt_effective_thr"] * data["slice_ue_assoc"][:, s, :])) for s in range(env.S))
            print(f"  env {e:5d} episode {ep.episode_number:5d} (scenario {ep.scenario:3d}): {len(data['reward'])} TTIs, return {ret:10.4f} "
                  f"(device {res['reward'][e, j]:10.4f}), packets sent {sent:12.0f} (device {res['pkts_sent'][e, j]:12.0f})")
            worst = max(worst, abs(ret - res["reward"][e, j]))
    print(f"largest difference between a file's return and the device's episode sum: {worst:.3e} (the same addends, summed in another order)")
    env.close()


if __name__ == "__main__":
    main()
