"""Per-slice episode metrics, the parts that need no GPU: header and bindings agree, the report by slice type, the fixture
tests/golden/slice_metrics.npz against eval_metrics.npz, and the conditions on the inputs of the device's oracle test
(tests/test_gpu_slice_metrics.py, tests/slice_metrics_ref.py) that keep a green device run from being vacuous."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

from tests import slice_metrics_ref as smr
from tests.common import load_golden, tables_from

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- header and bindings ------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_names_agree():
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.batched_env import BatchedRanEnv
    header = open(os.path.join(REPO, "include", "ranenv.h")).read()
    assert re.search(r"#define\s+RANENV_ABI_VERSION\s+10\b", header) and _lib.ABI_VERSION == 10
    assert int(re.search(r"#define\s+RANENV_SLICE_METRIC_COLS\s+(\d+)", header).group(1)) == 10 == _lib.SLICE_METRIC_COLS
    names = BatchedRanEnv.SLICE_METRIC_NAMES
    assert len(names) == 10 and len(set(names)) == 10
    for fn in ("ranenv_enable_slice_metrics", "ranenv_get_slice_metrics"):
        assert re.search(r"\bint\s+" + fn + r"\s*\(", header), fn
        assert fn in _lib.EXPORTS and fn in _lib.FUNCTIONS
    # the header's column table: "[k] name", in the binding's order
    for k, name in enumerate(names):
        assert re.search(r"\[%d\]\s+%s\b" % (k, name), header), (k, name)
    for method in ("enable_slice_metrics", "disable_slice_metrics", "slice_episode_metrics"):
        assert callable(getattr(BatchedRanEnv, method))


def test_library_exports_the_two_functions():
    import ctypes
    from intent_radio_sched_multi_slice_amd import _lib
    from intent_radio_sched_multi_slice_amd.csrc import build
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "ranenv_enable_slice_metrics") and hasattr(raw, "ranenv_get_slice_metrics")
    assert raw.ranenv_abi_version() == 10


# ---- report -------------------------------------------------------------------------------------------------------------------------
def _two_scenarios():
    """Two scenario rows of S = 3: type 2 (robotic_surgery_case_1, priority 1) at index 0 in row 0 and at index 2 in row 1; type 1
    (monitoring_case_1, priority 0) at index 1 in both; the third slot empty (no request) in row 0, type 9 in row 1."""
    from intent_radio_sched_multi_slice_amd.scenario import ScenarioTables, slice_template_dict, slice_type_from_req
    S, U, Us = 3, 6, 2
    tabs = ScenarioTables.empty(2, S, U, Us)
    reqs = ({"slice_0": slice_template_dict(2), "slice_1": slice_template_dict(1), "slice_2": {}},
            {"slice_0": slice_template_dict(9), "slice_1": slice_template_dict(1), "slice_2": slice_template_dict(2)})
    for i, req in enumerate(reqs):
        sua = np.zeros((S, U))
        for s in range(S):
            sua[s, 2 * s:2 * s + 2] = 1
        tabs.set_from_reference(i, np.ones((1, S)), sua, req, True)
    st = np.stack([slice_type_from_req(r, S) for r in reqs])
    return tabs, st


def test_slice_type_report_on_a_hand_made_log():
    from intent_radio_sched_multi_slice_amd.scenario import SLICE_TYPE_NAMES, slice_type_report
    tabs, st = _two_scenarios()
    assert st.tolist() == [[2, 1, -1], [9, 1, 2]]
    log = np.zeros((2, 2, 3, 10))          # [env, episode, S, 10]
    scen = np.array([[0, 1], [1, -1]])     # env 1 finished one episode only
    # columns: active, violations, thr, rel, lat, distance, incoming, capacity, sent, dropped
    log[0, 0, 0] = [50, 7, 4, 0, 5, -1.5, 100, 90, 80, 3]       # surgery at index 0 of row 0
    log[0, 0, 1] = [50, 0, 0, 0, 0, 0.0, 10, 20, 10, 0]         # monitoring: a zero row -> absent from both dicts
    log[0, 0, 2] = [50, 9, 9, 9, 9, -9.0, 5, 5, 5, 5]           # no request there: no type, counted nowhere by type
    log[0, 1, 2] = [50, 2, 0, 2, 0, -0.5, 40, 30, 20, 1]        # surgery at index 2 of row 1
    log[0, 1, 0] = [50, 3, 3, 0, 0, -0.2, 7, 6, 5, 0]           # video_streaming_4k
    log[1, 0, 2] = [50, 1, 1, 0, 0, -0.1, 1, 1, 1, 0]           # surgery again (env 1, row 1)
    log[1, 1, 0] = [9, 9, 9, 9, 9, -9, 9, 9, 9, 9]              # an empty slot of the log (scenario -1): ignored
    rep = slice_type_report(log, scen, st, tabs)
    assert rep["violations_per_slice_type"] == {"robotic_surgery_case_1": 10, "video_streaming_4k": 3}
    assert rep["violations_slice_metric"] == {"robotic_surgery_case_1": {"throughput": 5, "reliability": 2, "latency": 5},
                                              "video_streaming_4k": {"throughput": 3}}
    assert "monitoring_case_1" not in rep["violations_per_slice_type"] and "monitoring_case_1" not in rep["violations_slice_metric"]
    msg = {n: t[5] for n, t in zip(SLICE_TYPE_NAMES, __import__("intent_radio_sched_multi_slice_amd.scenario", fromlist=["x"]).SLICE_TEMPLATES)}
    np.testing.assert_allclose(rep["served_mbit"]["robotic_surgery_case_1"], (80 + 20 + 1) * msg["robotic_surgery_case_1"] / 1e6, rtol=1e-15)
    np.testing.assert_allclose(rep["capacity_mbit"]["monitoring_case_1"], 20 * msg["monitoring_case_1"] / 1e6, rtol=1e-15)
    np.testing.assert_allclose(rep["requested_mbit"]["video_streaming_4k"], 7 * msg["video_streaming_4k"] / 1e6, rtol=1e-15)
    # the network totals: every slice, message size 0 where there is no request (calc_message_sizes)
    want = ((90 + 30 + 1) * msg["robotic_surgery_case_1"] + 20 * msg["monitoring_case_1"] + 6 * msg["video_streaming_4k"]) / 1e6
    np.testing.assert_allclose(rep["total_network_throughput"], want, rtol=1e-15)
    prio = slice_type_report(log, scen, st, tabs, priority_only=True)
    assert prio["violations_per_slice_type"] == {"robotic_surgery_case_1": 10}
    assert prio["violations_slice_metric"] == {"robotic_surgery_case_1": {"throughput": 5, "reliability": 2, "latency": 5}}
    assert set(prio["served_mbit"]) == {"robotic_surgery_case_1"}


def test_slice_type_from_req_round_trips_the_ten_templates():
    from intent_radio_sched_multi_slice_amd.scenario import SLICE_TYPE_NAMES, slice_template_dict, slice_type_from_req
    req = {f"slice_{s}": slice_template_dict((s * 3) % 10) for s in range(10)}
    assert slice_type_from_req(req, 10).tolist() == [(s * 3) % 10 for s in range(10)]
    assert len(SLICE_TYPE_NAMES) == 10
    req["slice_3"] = {}
    req["slice_4"] = {"name": "something_else"}
    got = slice_type_from_req(req, 12)
    assert got[3] == -1 and got[4] == -1 and got[10] == -1 and got[11] == -1 and got[5] == 5
    assert slice_type_from_req(None, 2).tolist() == [-1, -1]


# ---- fixture ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["live_deque", "restarted_with_reset"])
def test_fixture_rows_aggregate_to_the_eval_metrics_fixture(tag):
    """slice_metrics.npz's per-TTI, per-slice drifts summed over the slices give eval_metrics.npz's ``violations`` and ``distance``
    columns of the same run (both come from the reference's functions on the same history files)."""
    fx, ev = load_golden("slice_metrics"), load_golden("eval_metrics")
    assert np.array_equal(fx["cfg"], ev["cfg"]) and np.array_equal(fx["scen_ids"], ev["scen_ids"])
    m = fx[f"{tag}_intent_slice_metric"]                     # [ep, t, S, 3]
    d = np.where(m == -2, 1.0, m)
    dmin = d.min(axis=3)
    viol = (dmin < 0).sum(axis=2)
    dist = np.minimum(dmin, 0.0).sum(axis=2)
    assert np.array_equal(viol, ev[tag][:, :, 0])
    np.testing.assert_allclose(dist, ev[tag][:, :, 2], rtol=0, atol=1e-12)
    assert viol.sum() > 0 and (m != -2).any(axis=(0, 1, 2)).all()
    # the throughputs: served <= capacity, requested == the traffic pool in packets x message size
    for name in ("total_network_throughput", "total_network_eff_throughput", "total_network_requested_throughput"):
        assert fx[f"{tag}_{name}"].shape == m.shape[:2] and (fx[f"{tag}_{name}"] >= 0).all()
    assert (fx[f"{tag}_total_network_eff_throughput"] <= fx[f"{tag}_total_network_throughput"] + 1e-9).all()


# ---- conditions on the inputs of the device's oracle test ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs():
    return {name: smr.run_of(name) for name in smr.CASES}


def test_case_shapes_are_the_ones_the_device_test_claims(runs):
    c = runs["ref-overfulfill-0.5"]["case"]
    assert (c["B"], c["steps"], c["S"], c["U"], c["Us"]) == (7, 26, 5, 25, 10)
    c = runs["range-intent"]["case"]
    assert (c["B"], c["steps"], c["S"], c["U"], c["Us"]) == (7, 26, 5, 25, 10) and c["range_intent"]
    assert (runs["s10-u100"]["case"]["S"], runs["s10-u100"]["case"]["U"]) == (10, 100)
    c = runs["s16-u256"]["case"]
    assert (c["S"], c["Us"], c["U"]) == (16, 16, 256)


def test_every_column_is_populated(runs):
    for name, run in runs.items():
        exp = smr.expected_sums(run)
        assert (np.abs(exp).sum(axis=(0, 1)) > 0).all(), (name, np.abs(exp).sum(axis=(0, 1)))


def test_each_metric_is_violated_alone_somewhere(runs):
    """Per metric: a TTI where it is violated while another DECLARED metric of the same active slice is not (so a kernel that
    counted 'the slice is in violation' into every declared metric would differ)."""
    alone = np.zeros(3, dtype=bool)
    for run in runs.values():
        tabs = run["tables"]
        for t in range(run["case"]["steps"]):
            for b, pe in enumerate(run["steps"][t][2]):
                sc = int(run["scen"][b])
                oa = np.asarray(pe[2]["obs_intra"], dtype=np.float64).reshape(tabs.n_slices, -1)
                for s in range(tabs.n_slices):
                    if not tabs.slice_active[sc, s]:
                        continue
                    dec = oa[s, 3:6] > 0
                    neg = dec & (oa[s, 0:3] < 0)
                    ok = dec & ~(oa[s, 0:3] < 0)
                    if ok.any():
                        alone |= neg
    assert alone.all(), alone


def test_tables_hold_the_awkward_slices(runs):
    inactive_with_drift = no_ues = False
    for run in runs.values():
        tabs = run["tables"]
        no_ues |= bool(np.any(tabs.slice_nues[run["scen"]] == 0))
        for t in range(run["case"]["steps"]):
            for b, pe in enumerate(run["steps"][t][2]):
                sc = int(run["scen"][b])
                oa = np.asarray(pe[2]["obs_intra"], dtype=np.float64).reshape(tabs.n_slices, -1)
                sel = (tabs.slice_active[sc] == 0) & (tabs.slice_nues[sc] > 0)
                inactive_with_drift |= bool(np.any(sel & (np.abs(oa[:, 0:3]).sum(axis=1) > 0) & (np.asarray(pe[2]["reward"])[1:] != 0)))
    assert inactive_with_drift and no_ues


def test_scenarios_place_different_types_at_one_index(runs):
    """Two scenario rows of one case that put slices of different kinds (request, parameters, buffer, message size, traffic) at one
    slice index: a log without the scenario row could not be read."""
    from intent_radio_sched_multi_slice_amd.scenario import _slice_signature
    for name, run in runs.items():
        tabs = run["tables"]
        rows = sorted(set(int(x) for x in run["scen"]))
        both = [(a, b, s) for a in rows for b in rows for s in range(tabs.n_slices)
                if a < b and tabs.slice_has_req[a, s] and tabs.slice_has_req[b, s] and _slice_signature(tabs, a, s) != _slice_signature(tabs, b, s)]
        assert len(both) >= 1, name


def test_slice_type_from_tables_matches_the_request_dicts():
    from intent_radio_sched_multi_slice_amd.scenario import slice_type_from_tables
    tabs, st = _two_scenarios()
    assert np.array_equal(slice_type_from_tables(tabs), st)
    ev = tables_from(load_golden("eval_metrics"))
    got = slice_type_from_tables(ev)
    assert ((got >= 0) == (ev.slice_has_req != 0)).all() and len(set(got[got >= 0].tolist())) >= 5


@pytest.mark.parametrize("slip", smr.SLIPS)
def test_each_planted_slip_moves_the_expected_sums(runs, slip):
    """On the cases the DEVICE runs: a kernel with that slip would miss the oracle's sums by at least one whole count."""
    worst = 0.0
    for name in smr.DEVICE_CASES:
        exp, bad = smr.expected_sums(runs[name]), smr.expected_sums(runs[name], slip)
        cols = [0, 1, 2, 3, 4, 6, 7, 8, 9]
        worst = max(worst, float(np.abs(exp[:, :, cols] - bad[:, :, cols]).max()))
    assert worst >= 1.0, (slip, worst)
