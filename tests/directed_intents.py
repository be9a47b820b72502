"""Directed intent inputs: scenario tables, traffic and channel tiles built by hand so that every branch of the intent
drift and of the reward is taken often -- which the ten slice templates (SLICE_TEMPLATES) never manage: they ask for
99.99 % reliability and more (a band 1e-4 wide at most), use `at_least` / `at_most` only and run under the default
scalars.  Shared by the census (tests/intent_census.py), the planted-variant test (tests/test_intent_branches_cpu.py)
and the device tests (tests/test_gpu_intent_branches.py).

Two kinds of slice:

* ``poisson``: Poisson traffic as the reference draws it, with requirement values placed where rate, capacity and
  queueing delay land under the case's load: reliability 80-99 % (band 0.01-0.2), latency a few TTIs either side of
  the delay, throughput around the offered rate.  These give the continuous spread: over-fulfilled, in the band,
  violated.
* ``burst``: every UE receives one burst of 2 x buffer_size packets every 10 TTIs and nothing in between, packets of
  2e6 bits, a power-of-two buffer.  Half of every burst is dropped, so the loss rate over a 10-deep window is exactly
  0.5 while the queue drains between bursts; the queue holds packets of one age, so the latency is a whole number of
  TTIs; the throughput is a whole multiple of 2.0.  These values are hit *exactly*, which is what separates `>=` from
  `>`, `<=` from `<`, and `==` from both.

The drift is continuous where an operator flips: at x == value both sides of `>=` against `>` (and of `<=` against `<`)
give 0.0, so a kernel that mixed them up would differ from the reference only where the wrongly taken side is 0 / 0.  Two
requirements put that there, both finite under the right operator: reliability `> 100` (never met, drift -x; `>= 100` is
met by a loss rate of 0, with a band 0 wide) and latency `< 0` (never met, drift -x / max_latency; `<= 0` is met by an
empty queue).  `==` against `>=` differs by whole units wherever x exceeds the value.

Every (metric order) x (1, 2, 3 parameters) appears, with the five operators rotating over them.  Around the slices with
a requirement, a scenario has slices with UEs and no requirement, inactive slices with UEs and a requirement, slices
without UEs, and priorities 0 and 1 mixed.  Everything is drawn from fixed seeds.
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np

from intent_radio_sched_multi_slice_amd.scenario import OP_UFUNC, ScenarioTables
from tests.synth import se_tile

BURST_PERIOD = 10
BURST_MSG = 2_000_000           # bits: throughput = sent * 2.0 exactly
OPS = (0, 1, 2, 3, 4)           # GE, LE, EQ, GT, LT
_METRIC = ("throughput", "reliability", "latency")

# every order of one, two and three distinct metrics: 3 + 6 + 6 = 15
METRIC_ORDERS: Tuple[Tuple[int, ...], ...] = tuple(
    itertools.chain.from_iterable(itertools.permutations(range(3), n) for n in (3, 2, 1)))

# requirement values of a poisson slice, by operator class.  "floor" operators (GE, GT) are fulfilled from the value
# upwards, "ceiling" operators (LE, LT) from the value downwards; EQ is met by exact hits only (burst slices).
_REL_VALUES = (80.0, 85.0, 90.0, 95.0, 99.0, 70.0)
_LAT_VALUES = (2.0, 3.0, 4.0, 6.0, 8.0)
_THR_FRACTIONS = (0.5, 0.7, 0.85, 1.0, 1.15)


def _poisson_slice(j: int, order, ops) -> dict:
    traffic = (5.0, 10.0, 20.0, 40.0)[j % 4]
    msg = (8192, 16000, 65536, 4096)[(j // 2) % 4]
    per_tti = traffic * 1e6 / msg
    params = []
    for p, m in enumerate(order):
        if m == 0:
            v = round(traffic * _THR_FRACTIONS[(j + p) % 5], 3)
        elif m == 1:
            v = _REL_VALUES[(j + p) % 6]
        else:
            v = _LAT_VALUES[(j + p) % 5]
        params.append((m, ops[p], v))
    return dict(kind="poisson", priority=(j // 3) % 2, params=params,
                ues=dict(buffer_size=max(4, int(per_tti * (2, 3, 5)[j % 3])), buffer_latency=(6, 10, 16, 24)[(j // 4) % 4],
                         message_size=msg, traffic=traffic))


def _burst_slice(j: int, order, ops) -> dict:
    bsize = (32, 64, 16)[j % 3]
    params = []
    for p, m in enumerate(order):
        if m == 0:
            v = 2.0 * (3, 5, 8, 12)[(j + p) % 4]          # a whole number of 2e6-bit packets per TTI
        elif m == 1:
            v = (50.0, 50.0, 100.0)[(j + p) % 3] if ops[p] == 3 else 50.0   # `> 100` is never met: 100 (1 - 0) == 100
        else:
            # `< 0` is never met and its drift -x / max_latency is finite; `<= 0` would be met by an empty queue, as 0 / 0
            v = 0.0 if (ops[p] == 4 and j % 2 == 0) else float((1, 2, 3, 4, 5)[(j + p) % 5])
        params.append((m, ops[p], v))
    return dict(kind="burst", priority=(j // 2) % 2, params=params,
                ues=dict(buffer_size=bsize, buffer_latency=(8, 12, 20)[(j // 3) % 3], message_size=BURST_MSG,
                         traffic=2 * bsize * BURST_MSG / 1e6 / BURST_PERIOD))


def catalogue() -> List[dict]:
    """60 slices with a requirement: 15 metric orders x {poisson, burst} x 2 operator rotations."""
    out = []
    j = 0
    for rot in (0, 2):
        for kind in (_poisson_slice, _burst_slice):
            for i, order in enumerate(METRIC_ORDERS):
                ops = tuple(OPS[(i + rot + 2 * p + m) % 5] for p, m in enumerate(order))
                out.append(kind(j, order, ops))
                j += 1
    return out


CATALOGUE = catalogue()


def _req(entry: dict, name: str) -> dict:
    return {
        "name": name, "priority": entry["priority"],
        "parameters": {f"par{p + 1}": {"name": _METRIC[m], "value": v, "unit": "", "operator": OP_UFUNC[op]}
                       for p, (m, op, v) in enumerate(entry["params"])},
        "ues": dict(entry["ues"], mobility=0),
    }


@dataclass
class Directed:
    tables: ScenarioTables
    kind: np.ndarray            # [NS, S] 0 = no traffic (no requirement), 1 = poisson, 2 = burst

    def traffic_rows(self, scen: int, rng: np.random.Generator, steps: int, load: float = 1.0) -> np.ndarray:
        """[steps, U] offered bits.  Poisson slices in MultSliceTraffic.step's draw order times ``load`` (floored);
        burst slices: 2 x buffer_size packets at the TTIs t with (t + ue) % 10 == 0.  Inactive slices with a
        requirement receive traffic too, as in the reference (traffics/mult_slice.py:24-32 asks for the request only)."""
        t_ = self.tables
        out = np.zeros((steps, t_.n_ues))
        for t in range(steps):
            for s in range(t_.n_slices):
                n = int(t_.slice_nues[scen, s])
                ues = t_.slice_ues[scen, s, :n]
                if self.kind[scen, s] == 1:
                    out[t, ues] = np.floor(rng.poisson(t_.slice_traffic[scen, s], n) * 1e6 * load)
                elif self.kind[scen, s] == 2:
                    hit = (t + ues) % BURST_PERIOD == 0
                    out[t, ues[hit]] = 2.0 * t_.slice_buffer_size[scen, s] * BURST_MSG
        return out


def build(n_scenarios: int, S: int, U: int, Us: int, seed: int = 0, first: int = 0, equal_sizes: bool = False,
          nothing_active=()) -> Directed:
    """``n_scenarios`` rows through ScenarioTables.set_from_reference.  Slice (i, s) takes catalogue entry
    ``first + i * S + s``; roughly one slice in eight has UEs and no requirement, one in eight is inactive with UEs and
    a requirement, one in twenty-four has no UE.  ``equal_sizes``: every slice the same number of UEs (with equal scores the
    RBGs then divide without remainder where S divides them).  ``nothing_active``: rows whose slices are all inactive
    (IBSched.action_format then leaves the allocation all-zero, agents/ib_sched.py:240-245)."""
    tabs = ScenarioTables.empty(n_scenarios, S, U, Us)
    kind = np.zeros((n_scenarios, S), dtype=np.int32)
    for i in range(n_scenarios):
        rng = np.random.default_rng(7000 + 131 * seed + i)
        perm = rng.permutation(U)
        bsa = np.ones((1, S)); sua = np.zeros((S, U)); req = {}
        left, at = U, 0
        for s in range(S):
            entry = CATALOGUE[(first + i * S + s) % len(CATALOGUE)]
            role = int(rng.integers(0, 24)) if S > 1 else 3
            cap = min(Us, left - (S - 1 - s)) if left >= S - s else min(Us, left)      # (one UE kept back for every slice still to come)
            if equal_sizes:
                n = min(Us, U // S)
            else:
                n = 0 if (role == 0 or cap < 1) else int(rng.integers(1, cap + 1))
            sua[s, perm[at:at + n]] = 1
            at += n; left -= n
            if role in (1, 2, 23):              # UEs, no requirement
                req[f"slice_{s}"] = {}
                continue
            if role in (4, 5, 6) and S > 2:     # inactive, with UEs and a requirement
                bsa[0, s] = 0
            req[f"slice_{s}"] = _req(entry, f"directed_{(first + i * S + s) % len(CATALOGUE)}")
            kind[i, s] = 1 if entry["kind"] == "poisson" else 2
        if i in nothing_active:
            bsa[:] = 0
        tabs.set_from_reference(i, bsa, sua, req, True)
    return Directed(tabs, kind)


def add_range_intents(tabs: ScenarioTables) -> int:
    """Replace the parameters of every slice that has a throughput requirement by a range intent: two
    parameters on ONE metric (throughput at least 0.4 x and at most 1.0 x the offered rate), written into the param_*
    arrays directly, since set_from_reference refuses such a request.  The oracle adds both terms, as the reference does
    (`observations[...] +=`, agents/common.py); the C ABI refuses the table (include/ranenv.h).  Returns how many slices changed."""
    changed = 0
    for i in range(tabs.n_scenarios):
        for s in range(tabs.n_slices):
            if not tabs.slice_has_req[i, s] or 0 not in tabs.param_metric[i, s, :tabs.slice_nparams[i, s]]:
                continue
            rate = float(tabs.slice_traffic[i, s])
            tabs.slice_nparams[i, s] = 2
            tabs.param_metric[i, s, :2] = 0
            tabs.param_op[i, s, :2] = (0, 1)
            tabs.param_value[i, s, :2] = (0.4 * rate, rate)
            changed += 1
    return changed


def se_tiles(seed: int, n: int, U: int, R: int, low_se: int = 0, scale: float = 1.0) -> np.ndarray:
    """[n, U, R] float32 tiles of tests/synth.se_tile, scaled (the SE level sets capacity against the offered load)."""
    return np.stack([(se_tile(seed, t, U, R, low_se_every=low_se) * np.float32(scale)).astype(np.float32) for t in range(n)])


# ----------------------------------------------------------------------------------------------------------------------
# the directed cases: shape, scalars, load, how the TTIs are driven.  `scalars` go to BatchedRanEnv and to make_cfg alike.
# ----------------------------------------------------------------------------------------------------------------------
# (the requirement values and `overfulfill` keep every observation below 256 in magnitude: from there on half a float32 ulp
# exceeds the 1e-5 bar of the device tests, which no float32 output could then meet; tests/test_intent_branches_cpu.py checks it)
DEFAULT_SCALARS = dict(overfulfill=0.2, norm_traffic=120.0, norm_ues=5.0, norm_se=40.0, bandwidth_hz=100e6)
ALL_SCALARS = dict(overfulfill=0.05, norm_traffic=75.0, norm_ues=8.0, norm_se=25.0, bandwidth_hz=60e6)


def _case(name, S, U, R, G, Us, B=7, steps=26, D=10, load=1.0, se_scale=1.0, low_se=0, policy=0, intra=255, n_scen=4,
          first=0, equal_sizes=False, range_intent=False, nothing_active=(), per_element=False, **scalars) -> dict:
    bad = set(scalars) - set(DEFAULT_SCALARS)
    assert not bad, bad
    return dict(name=name, S=S, U=U, R=R, G=G, Us=Us, B=B, steps=steps, D=D, load=load, se_scale=se_scale, low_se=low_se,
                policy=policy, intra=intra, n_scen=n_scen, first=first, equal_sizes=equal_sizes, range_intent=range_intent, nothing_active=tuple(nothing_active),
                per_element=per_element, scalars=dict(DEFAULT_SCALARS, **scalars))


# policy 0 = the caller's scores and per-slice intra choice, 1 = MARR, 2 = MAPF (device policies; intra 0 RR, 1 PF, 2 MT)
CASES: Tuple[dict, ...] = (
    # the reference size; every scalar at its default, then all changed, then one at a time
    _case("ref-default", 5, 25, 135, 5, 10, n_scen=12, B=12, steps=32, nothing_active=(11,)),
    _case("ref-all-scalars", 5, 25, 135, 5, 10, n_scen=12, B=12, first=60 // 2, steps=32, **ALL_SCALARS),
    _case("ref-overfulfill-0.5", 5, 25, 135, 5, 10, first=7, load=1.5, policy=2, intra=1, overfulfill=0.5),
    _case("ref-overfulfill-0.05", 5, 25, 135, 5, 10, first=19, policy=1, intra=0, overfulfill=0.05),
    _case("ref-norm-traffic", 5, 25, 135, 5, 10, first=23, policy=2, intra=2, norm_traffic=60.0),
    _case("ref-norm-ues", 5, 25, 135, 5, 10, first=31, policy=2, intra=0, norm_ues=3.0),
    _case("ref-norm-se", 5, 25, 135, 5, 10, first=37, load=0.6, policy=1, intra=1, norm_se=16.0),
    # (per_element: RANENV_F_SCALE_PER_ELEMENT, the other rounding of pkt_throughputs, on the handle and in the oracle)
    _case("ref-bandwidth", 5, 25, 135, 5, 10, first=43, policy=1, intra=2, bandwidth_hz=40e6, per_element=True),
    # two envs per wave where the build packs them (U <= 32, S and Us <= 8)
    _case("packable", 8, 32, 64, 2, 8, B=8, n_scen=8, first=3, load=1.3, low_se=3),
    # 64 < U <= 128: the mixed blocks; a partial last wave (U = 100 -> 64 + 36)
    _case("partial-wave", 12, 100, 120, 3, 12, n_scen=5, first=11, load=1.2, policy=2, intra=1, D=2, overfulfill=0.1),
    # the full 16 x 16 slot grid, four waves per env
    _case("grid-16x16", 16, 256, 96, 1, 16, B=5, n_scen=4, first=5, steps=24, load=2.0, se_scale=0.5,
          **dict(ALL_SCALARS, overfulfill=0.1)),
    # equal scores (MARR), equal slice sizes, 5 slices over 25 RBGs: round_int_equal_sum has nothing left to hand out
    _case("no-remainder", 5, 25, 125, 5, 5, first=13, policy=1, intra=0, equal_sizes=True, D=1, load=0.8),
    _case("one-slice", 1, 8, 40, 4, 8, B=4, n_scen=4, first=1, steps=22, load=3.0, se_scale=0.3, D=1, overfulfill=0.5),
)
CASE_BY_NAME: Dict[str, dict] = {c["name"]: c for c in CASES}
# oracle only: the device refuses these tables
RANGE_INTENT_CASE = _case("range-intent", 5, 25, 135, 5, 10, first=9, range_intent=True)


def materialise(case: dict):
    """(Directed, scenario [B], se_pool [B * steps, U, R] float32, traffic [B * steps, U] float64) of one case."""
    c = case
    d = build(c["n_scen"], c["S"], c["U"], c["Us"], seed=len(c["name"]) + c["first"], first=c["first"], equal_sizes=c["equal_sizes"],
              nothing_active=c["nothing_active"])
    if c["range_intent"]:
        assert add_range_intents(d.tables) > 0
    rng = np.random.default_rng(8000 + c["first"] + c["S"])
    scen = np.arange(c["B"]) % c["n_scen"]
    se_pool = se_tiles(400 + c["first"], c["B"] * c["steps"], c["U"], c["R"], low_se=c["low_se"], scale=c["se_scale"])
    trf = np.concatenate([d.traffic_rows(int(scen[b]), rng, c["steps"], c["load"]) for b in range(c["B"])])
    assert trf.max() < 2 ** 31
    return d, scen, se_pool, trf


def external_action(case: dict, t: int):
    """The caller's scores [B, S] and per-slice intra choice [B, S] at TTI ``t`` (policy 0): a fixed draw per (case, t);
    one score in seven is -1 (no RBs)."""
    rng = np.random.default_rng(9100 + 97 * case["first"] + t)
    B, S = case["B"], case["S"]
    sc = rng.uniform(-1, 1, (B, S))
    sc[rng.random((B, S)) < 0.15] = -1.0
    return sc, rng.integers(0, 3, (B, S)).astype(np.uint8)
