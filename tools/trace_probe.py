"""What a device trace costs, under rollout() and paced by the host under record(): B 4096, S 10 / U 100 / R 100 under MAPF + PF (workloads.make_mult_slice_workload),
16 envs traced.

Writes one JSON record to profiles/trace_probe.json (and prints it).  Every block in a child process of its own, the blocks
ALTERNATED inside one job (--alternations rounds), medians over all samples of a block:
  (a) trace_ms        rollout(K) with the trace bound (BatchedRanEnv.bind_trace: one TTI per launch + one small launch per TTI)
  (b) recorder_ms     the step() loop under record() (HistoryRecorder: the same trace, and one done.cpu() per TTI to write an env's
                      file at the TTI its episode ends); episodes longer than the loop, so that no file is written inside the timing.
                      With --baseline-repo (a checkout of the parent commit with its library built) the parent's record() as
                      well, twice per round: `recorder_parent_ms`, `recorder_parent_vs_parent` (the spread of its two series) and
                      `recorder_not_slower`: recorder_ms / recorder_parent_ms - 1 <= that spread
  (c) plain_this_ms   rollout(K) with nothing bound, this build
  (d) plain_parent_ms the same with the parent commit's library (--baseline-lib, loaded through RANENV_LIB), measured twice per
                      round: `parent_vs_parent` is the spread of the two parent series (ratio of their medians)
and the ratios a/b and c/d (`untaxed_within_spread`: |c/d - 1| <= that spread).  No threshold is attached to (a).

    python tools/trace_probe.py [--steps 200] [--reps 3] [--alternations 3] [--baseline-lib parent.so] [--baseline-repo parent_checkout]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SIZE = dict(batch=4096, n_slices=10, n_ues=100, n_rbs=100, rbs_per_rbg=1, max_ues_slice=10)
TRACED = 16
OUT = os.path.join(REPO, "profiles", "trace_probe.json")


def measure(block, steps, reps):
    """One block -> the list of its samples in ms."""
    import ctypes
    import numpy as np
    import torch
    from intent_radio_sched_multi_slice_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.FUNCTIONS if not hasattr(raw, n)]:      # (the parent commit's library lacks the three new functions)
        _lib.FUNCTIONS.pop(name)
    from intent_radio_sched_multi_slice_amd.workloads import make_mult_slice_workload
    warm = 8
    # (the recorder sizes its buffers by the episode length: episodes just longer than what the block steps)
    max_steps = warm + steps * reps + 1 if block == "recorder" else 100000
    wl = make_mult_slice_workload(device=torch.device("cuda", 0), policy=_lib.POLICY_MAPF, intra=_lib.INTRA_PF, n_scenarios=64, n_traces=64,
                                  trace_len=256, max_steps=max_steps, **SIZE)
    env = wl.env
    traced = [int(e) for e in np.linspace(0, SIZE["batch"] - 1, TRACED).round()]
    trace = None
    if block == "trace":
        trace = env.bind_trace(traced, steps)
    elif block == "recorder":
        env.record(traced, root_path=os.devnull, agent_name="probe")      # (no episode ends: nothing is written)

    def step_loop(n):
        for _ in range(n):
            env.step()

    fn = (lambda: step_loop(steps)) if block == "recorder" else (lambda: env.rollout(steps))
    env.reset()
    step_loop(warm) if block == "recorder" else env.rollout(warm)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        if trace is not None:
            trace.reset()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1))
    info = {"ms": out, "device": torch.cuda.get_device_name(0)}
    if block != "recorder":
        info["persistent"] = env.get_option("last_rollout_persistent")
        info["launches"] = env.get_option("last_rollout_launches")
    if trace is not None:
        c = trace.counts()
        info["rows"] = [int(c["count"].min()), int(c["count"].max())]
        info["lost"] = int(c["lost"].max())
        info["ring_bytes"] = int(sum(b.numel() * b.element_size() for b in trace.buffers.values()))
    env.close()
    return info


def _child(block, steps, reps, lib, repo=REPO):
    env = dict(os.environ)
    if lib:
        env["RANENV_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.join(os.path.abspath(repo), "tools", "trace_probe.py"), "--child", block, "--steps", str(steps),
           "--reps", str(reps)]
    res = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=600)
    out = json.loads(res.stdout.strip().splitlines()[-1])
    print(f"{block} ({'parent library' if lib else 'parent checkout' if repo != REPO else 'this build'}): {out['ms']}", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--baseline-repo", default=None)
    ap.add_argument("--child", default=None, choices=("plain", "trace", "recorder"))
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.child, args.steps, args.reps)))
        return
    # every measurement in a process of its own: the parent of them all never opens the GPU
    record = {"probe": "trace", "size": SIZE, "traced_envs": TRACED, "steps": args.steps, "reps": args.reps, "alternations": args.alternations}
    series = {"plain_this": [], "parent_a": [], "parent_b": [], "trace": [], "recorder": [], "recorder_parent_a": [], "recorder_parent_b": []}
    sched = {}
    for _ in range(args.alternations):
        if args.baseline_lib:
            series["parent_a"] += _child("plain", args.steps, args.reps, args.baseline_lib)["ms"]
        r = _child("plain", args.steps, args.reps, None)
        series["plain_this"] += r["ms"]
        sched["plain"] = {"persistent": r["persistent"], "launches": r["launches"]}
        record["device"] = r["device"]
        if args.baseline_lib:
            series["parent_b"] += _child("plain", args.steps, args.reps, args.baseline_lib)["ms"]
        r = _child("trace", args.steps, args.reps, None)
        series["trace"] += r["ms"]
        sched["trace"] = {k: r[k] for k in ("persistent", "launches", "rows", "lost", "ring_bytes")}
        if args.baseline_repo:
            series["recorder_parent_a"] += _child("recorder", args.steps, 1, None, args.baseline_repo)["ms"]
        series["recorder"] += _child("recorder", args.steps, 1, None)["ms"]
        if args.baseline_repo:
            series["recorder_parent_b"] += _child("recorder", args.steps, 1, None, args.baseline_repo)["ms"]
    med = {k: statistics.median(x) for k, x in series.items() if x}
    B = SIZE["batch"]
    record.update({"samples_ms": series, "schedule": sched, "trace_ms": med["trace"], "recorder_ms": med["recorder"],
                   "plain_this_ms": med["plain_this"], "a_over_b": med["trace"] / med["recorder"],
                   "trace_over_plain": med["trace"] / med["plain_this"],
                   "trace_extra_us_per_tti": (med["trace"] - med["plain_this"]) * 1e3 / args.steps,
                   "env_steps_per_s": {k: B * args.steps / (med[k] * 1e-3) for k in ("plain_this", "trace", "recorder")}})
    if args.baseline_lib:
        parent = statistics.median(series["parent_a"] + series["parent_b"])
        spread = abs(med["parent_a"] / med["parent_b"] - 1.0)
        record.update({"plain_parent_ms": parent, "parent_vs_parent": spread, "c_over_d": med["plain_this"] / parent,
                       "untaxed_within_spread": abs(med["plain_this"] / parent - 1.0) <= spread})
    if args.baseline_repo:
        parent = statistics.median(series["recorder_parent_a"] + series["recorder_parent_b"])
        spread = abs(med["recorder_parent_a"] / med["recorder_parent_b"] - 1.0)
        record.update({"recorder_parent_ms": parent, "recorder_parent_vs_parent": spread, "recorder_over_parent": med["recorder"] / parent,
                       "recorder_not_slower": med["recorder"] / parent - 1.0 <= spread})
    line = json.dumps(record)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
