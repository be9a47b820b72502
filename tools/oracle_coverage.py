#!/usr/bin/env python3
"""Which branches of the spec does a set of test inputs reach?  CPU only.

Builds oracle/ranenv_oracle.c with `gcc --coverage` into a temporary directory (its own compiler line: oracle/Makefile and
oracle/_build stay as they are), replays the oracle half of a named input set in a child process bound to that library,
runs `gcov -b -c` and prints the branches of the spec functions that were never taken.

    python tools/oracle_coverage.py fuzz                  # the oracle half of tests/test_gpu_fuzz.py: 24 cases, both roundings
    python tools/oracle_coverage.py templates             # fuzz + the other oracle-backed GPU files' inputs (below)
    python tools/oracle_coverage.py directed              # tests/directed_intents.py (cases, heads, the range intent)
    python tools/oracle_coverage.py templates directed    # the union

`templates` replays, next to the fuzz cases, the scenario generators of the remaining oracle-backed GPU files at their shapes
and policies: tests/test_gpu_parity.py (the two batch sizes x four policies; the six shapes x external / device),
tests/test_gpu_flags_and_errors.py (the degenerate tables; the alternative heads at window depths 10 and 5) and the
short-episode scenario changes of tests/test_gpu_se_gather_and_ranges.py's compact steps.  Same generators, seeds, shapes,
policies and step counts; the random scores are drawn here, not bit-identical to the tests' own.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC_FUNCTIONS = ("apply_op", "orc_round_int_equal_sum", "orc_scores_to_rbs", "round_robin", "throughput_available",
                  "proportional_fairness", "max_throughput", "orc_action_format", "get_metric_value", "intent_drift_into",
                  "obs_space_format", "calculate_reward", "buffer_receive", "buffer_send", "orc_env_core_step", "orc_env_get_heads")
SETS = ("fuzz", "templates", "directed")


def build_instrumented(tmp: str) -> str:
    for f in ("ranenv_oracle.c", "ranenv_oracle.h"):
        shutil.copy(os.path.join(REPO, "oracle", f), tmp)
    so = os.path.join(tmp, "libranenv_oracle.so")
    cc = os.environ.get("CC", "gcc")           # (compiled and linked in two steps: the notes file is then ranenv_oracle.gcno, which gcov looks for)
    subprocess.run([cc, "-O0", "-g", "--coverage", "-std=c11", "-fPIC", "-fopenmp", "-ffp-contract=off", "-fno-fast-math",
                    "-c", "ranenv_oracle.c", "-o", "ranenv_oracle.o"], check=True, cwd=tmp)
    subprocess.run([cc, "--coverage", "-fopenmp", "-shared", "-o", so, "ranenv_oracle.o", "-lm"], check=True, cwd=tmp)
    return so


# ----------------------------------------------------------------------------------------------------------------------
# the child: replay input sets on the instrumented library
# ----------------------------------------------------------------------------------------------------------------------
def _generic(tabs, S, U, R, G, Us, steps, B, policy, intra, seed, D=10, heads=False, scen=None, reset_at=None):
    import numpy as np
    from oracle import pyoracle
    from tests.common import poisson_traffic_rows
    from tests.synth import se_tile
    rng = np.random.default_rng(seed)
    scen = rng.integers(0, tabs.n_scenarios, B) if scen is None else np.asarray(scen)
    cfg = pyoracle.make_cfg(S, U, R, G, Us, max_steps=steps, hist_depth=D)
    uc = rng.integers(0, 4, S).astype(np.int32)
    for b in range(B):
        o = pyoracle.OracleEnv(cfg); o.set_scenario(tabs, int(scen[b])); o.reset(se_tile(seed, 0, U, R))
        trf = poisson_traffic_rows(tabs, int(scen[b]), rng, steps)
        for t in range(steps):
            if reset_at and t and t % reset_at == 0:            # a scenario change in the middle: the deque survives
                scen[b] = (scen[b] + 1) % tabs.n_scenarios
                o.set_scenario(tabs, int(scen[b])); o.reset(se_tile(seed, t, U, R))
                trf = poisson_traffic_rows(tabs, int(scen[b]), rng, steps)
            if policy == 0:
                sc = rng.uniform(-1, 1, S); ic = rng.integers(0, 3, S).astype(np.int32) if intra == 255 else np.full(S, intra, dtype=np.int32)
            else:
                sc = o.policy_marr() if policy == 1 else o.policy_mapf(); ic = np.full(S, intra, dtype=np.int32)
            o.step(sc, ic, se_tile(seed, b * steps + t + 1, U, R), trf[t])
            if heads:
                o.heads(uc)


def replay_set(name: str) -> None:
    import numpy as np
    sys.path.insert(0, REPO)
    from tests import directed_intents as di
    from tests import intent_census as ic
    if name in ("fuzz", "templates"):
        for k in range(24):
            for per_element in (False, True):
                ic.replay_fuzz_case(k, per_element)
    if name == "templates":
        from intent_radio_sched_multi_slice_amd.scenario import ScenarioTables, generate_scaled_scenarios, slice_template_dict
        ref = generate_scaled_scenarios(6, seed=3, n_slices=5, n_ues=25, max_ues_slice=10, min_slices=3, min_ues=2)
        scaled = generate_scaled_scenarios(6, seed=4, n_slices=10, n_ues=100, max_ues_slice=16, min_slices=6, min_ues=4)
        for policy, intra in ((1, 0), (2, 1), (0, 255), (2, 2)):                      # test_batch_vs_oracle
            _generic(ref, 5, 25, 135, 5, 10, 20, 8, policy, intra, 11)
            _generic(scaled, 10, 100, 135, 5, 16, 20, 8, policy, intra, 12)
        for sh in (dict(S=3, U=7, R=5, G=1, Us=4), dict(S=4, U=37, R=100, G=5, Us=12), dict(S=16, U=128, R=300, G=3, Us=16),
                   dict(S=6, U=64, R=408, G=8, Us=11), dict(S=16, U=256, R=64, G=1, Us=16), dict(S=5, U=30, R=48, G=2, Us=8, D=3)):
            S, U, R, G, Us = (sh[k] for k in ("S", "U", "R", "G", "Us"))              # test_shapes_vs_oracle
            tabs = generate_scaled_scenarios(3, seed=5, n_slices=S, n_ues=U, max_ues_slice=Us, min_slices=max(1, S // 2), min_ues=max(1, Us // 3))
            for policy, intra in ((0, 255), (2, 1)):
                _generic(tabs, S, U, R, G, Us, 14, 6, policy, intra, 7, D=sh.get("D", 10))
        S, U, R, G, Us = 5, 25, 135, 5, 5                                             # test_degenerate_scenarios_vs_oracle
        tabs = ScenarioTables.empty(4, S, U, Us)
        bsa = np.zeros((1, S)); sua = np.zeros((S, U)); bsa[0, 2] = 1
        req = {f"slice_{s}": {} for s in range(S)}; req["slice_2"] = slice_template_dict(1)
        tabs.set_from_reference(1, bsa, sua, req, True)
        bsa = np.zeros((1, S)); sua = np.zeros((S, U)); bsa[0, 4] = 1; sua[4, 7] = 1
        req = {f"slice_{s}": {} for s in range(S)}; req["slice_4"] = slice_template_dict(5)
        tabs.set_from_reference(2, bsa, sua, req, True)
        ordinary = generate_scaled_scenarios(1, seed=9, n_slices=S, n_ues=U, max_ues_slice=Us, min_slices=3, min_ues=2)
        for k, v in ordinary.arrays().items():
            getattr(tabs, k)[3] = v[0]
        for policy, intra in ((1, 0), (2, 1), (2, 2), (0, 255)):
            _generic(tabs, S, U, R, G, Us, 8, 4, policy, intra, 2, scen=np.arange(4))
        for D in (10, 5):                                                             # test_alternative_heads_vs_oracle
            _generic(ref, 5, 25, 135, 5, 10, 16, 6, 0, 0, 9, D=D, heads=True)
        for steps in (4, 13):                                                         # compact steps through scenario changes
            _generic(ref, 5, 25, 135, 5, 10, 3 * steps, 6, 2, 1, 21, reset_at=steps)
    if name == "directed":
        for c in di.CASES:
            ic.replay(c, keep=False)
        ic.replay(di.RANGE_INTENT_CASE, keep=False)
        for nm in ("ref-all-scalars", "packable"):
            case = di.CASE_BY_NAME[nm]
            for D in (10, 5):
                uc = np.random.default_rng(3).integers(0, 4, case["S"]).astype(np.int32)
                ic.replay(dict(case, D=D, intra=0), keep=False, extra=lambda o, b: o.heads(uc))


def child(lib: str, names) -> None:
    sys.path.insert(0, REPO)
    from oracle import pyoracle
    pyoracle._SO = lib
    pyoracle.build = lambda force=False: lib
    for n in names:
        replay_set(n)


# ----------------------------------------------------------------------------------------------------------------------
def untaken(tmp: str):
    """[(function, line, source text, [branch numbers never taken], n branches)] of the spec functions, from gcov -b -c."""
    subprocess.run(["gcov", "-b", "-c", "ranenv_oracle.c"], check=True, cwd=tmp, stdout=subprocess.DEVNULL)
    out, fn, cur = [], None, None
    totals = {}
    for line in open(os.path.join(tmp, "ranenv_oracle.c.gcov"), errors="replace"):
        m = re.match(r"function (\w+) called (\d+)", line)
        if m:
            fn = m.group(1); totals[fn] = int(m.group(2)); continue
        m = re.match(r"\s*([\d#=\-]+)\*?:\s*(\d+):(.*)", line)
        if m:
            cur = [fn, int(m.group(2)), m.group(3).strip(), [], 0]
            out.append(cur); continue
        m = re.match(r"branch\s+(\d+) (taken (\d+)|never executed)", line)
        if m and cur is not None:
            cur[4] += 1
            if m.group(2) == "never executed" or int(m.group(3)) == 0:
                cur[3].append(int(m.group(1)))
    return [tuple(c) for c in out if c[0] in SPEC_FUNCTIONS and c[3]], totals


def main(argv) -> int:
    if argv and argv[0] == "--child":
        child(argv[1], argv[2:]); return 0
    names = [a for a in argv if a in SETS]
    if not names or len(names) != len(argv):
        print(__doc__); return 2
    tmp = tempfile.mkdtemp(prefix="oracle_cov_")
    try:
        lib = build_instrumented(tmp)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, *names], check=True, cwd=REPO)
        rows, totals = untaken(tmp)
        print(f"input sets: {' + '.join(names)}")
        print("calls: " + ", ".join(f"{f} {totals.get(f, 0)}" for f in SPEC_FUNCTIONS))
        print(f"never-taken branches of the spec functions: {sum(len(r[3]) for r in rows)} on {len(rows)} lines")
        for fn, ln, text, br, n in rows:
            print(f"  {fn}:{ln}  branches {br} of {n}  | {text[:110]}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
