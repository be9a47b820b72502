"""The shape grid of the head / off-policy kernel family (tests/head_shapes_ref.py) without a GPU: the grid itself, the float32
restatement inside the float64 bounds on every new case, the conditions on the new inputs, and planted slips against the yardstick
(device error <= 8 x the float32 restatement's, floor 1e-6) -- those of sac_ref.SLIPS and four that depend on S, with the guard that
the old cases (S 5, S 10) could not see the ones that need the new shapes."""
from __future__ import annotations

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from intent_radio_sched_multi_slice_amd import adapters
from tests import head_policy_ref as hr
from tests import head_shapes_ref as hs
from tests import sac_ref as sr


@pytest.fixture(scope="module", params=list(hs.CASES))
def case(request):
    return hs.sac_case(request.param)


def _restate(c, slip=None, stochastic=True):
    return hs.restate(c["obs"], c["reward"], c["done"], *c["nets"], hs.GAMMA, hs.ENT_COEF, stochastic, hs.SEED, hs.DRAW, slip=slip)


# ---- the grid -----------------------------------------------------------------------------------------------------------------------
def test_the_grid_reaches_what_it_claims():
    net_ld = lambda x: x + (36 if x & 63 else 4)  # noqa: E731  (ranenv_net.hpp)
    S_of = sorted({c[0] for c in hs.CASES.values()})
    assert S_of == [1, 3, 6, 8, 16] and set(S_of) == set(hs.ENV_SHAPES) and len(hs.CASES) == 7
    assert {S: hs.pad32(11 * S) for S in S_of} == {1: 32, 3: 64, 6: 96, 8: 96, 16: 192}
    assert net_ld(96) == 96 + 36 and net_ld(64) == 64 + 4 and net_ld(192) == 192 + 4
    for S, kw in hs.ENV_SHAPES.items():
        assert kw["n_slices"] == S and kw["max_ues_slice"] <= 16 and kw["n_ues"] <= S * kw["max_ues_slice"]
    assert {S: -(-16 * S // 64) for S in (1, 3, 16)} == {1: 1, 3: 1, 16: 4}                  # the head kernel's waves
    assert [hs.ENV_SHAPES[S]["max_ues_slice"] for S in (1, 3, 16)] == [16, 16, 16]
    # pairs of a workgroup: none beyond 256 up to S 8, all 256 threads own a second one at S 16
    assert [max(0, hs.NET_ROWS * S - 256) for S in S_of] == [0, 0, 0, 0, 256]
    # the LDS row stride comes from the actor in one case and from the critics in another
    ldm = lambda S, widths, n_in, n_out: max(net_ld(hs.pad32(k)) for k in [n_in] + widths + [n_out])  # noqa: E731
    side = {name: (ldm(S, aw, 10 * S, 2 * S), ldm(S, qw, 11 * S, 1)) for name, (S, aw, _, qw, _) in hs.CASES.items()}
    assert any(a > q for a, q in side.values()) and any(q > a for a, q in side.values()), side
    widths = {w for _, aw, _, qw, _ in hs.CASES.values() for w in aw + qw}
    assert {1, 7, 33, 100, 255, 480, 511, 512} <= widths
    assert {len(aw) for _, aw, _, _, _ in hs.CASES.values()} | {len(qw) for _, _, _, qw, _ in hs.CASES.values()} == {1, 2, 3, 4}
    assert {a for _, _, a, _, _ in hs.CASES.values()} == {"tanh", "relu"} == {a for _, _, _, _, a in hs.CASES.values()}
    assert all(aw != qw or aa != qa for _, aw, aa, qw, qa in hs.CASES.values())
    for name in hs.TAIL_CASES:
        assert hs.CASES[name][0] in (1, 16)


def test_make_env_sizes_by_name_are_unchanged():
    assert hr.size_of("S5U25") is hr.SIZES["S5U25"] and hr.size_of("S10U100") is hr.SIZES["S10U100"]
    d = hs.ENV_SHAPES[16]
    assert hr.size_of(d) == d and hr.size_of(d) is not d


def test_the_existing_cases_nets_are_untouched():
    """sac_ref.sac_nets / head_policy_ref.head_nets: the first weights of the old fixtures, as they were before this module."""
    actor, q1, q2 = sr.sac_nets("64x64")
    plain = hr.mlp([50, 64, 64, 10], "tanh", 31, sr.OUT_SCALE)
    assert torch.equal(actor[0].weight, plain[0].weight) and torch.equal(actor[-1].weight, plain[-1].weight)
    assert torch.equal(actor[-1].bias[:5], plain[-1].bias[:5])
    shift = (actor[-1].bias[5:] - plain[-1].bias[5:]).tolist()
    assert shift == pytest.approx([-20.5, 2.6, -2.0, -2.0, -2.0], abs=1e-5)      # two biased positions, fixed: sac_ref.LOG_STD_BIAS


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_restate_without_a_slip_is_the_adapter_bit_for_bit(case):
    for st in (True, False):
        mine = _restate(case, None, st)
        assert all(torch.equal(mine[k], case["got"][st][k]) for k in mine), st


def test_torch_restatement_lies_inside_the_reference_bounds(case):
    for st in (True, False):
        sr.check_outputs(case["ref"][st], case["got"][st], f"{case['name']} stochastic={st}")
        d = case["done"] != 0
        assert np.array_equal(case["got"][st]["target"].numpy()[d], case["reward"][d])      # terminal rows: exactly float32(reward)
    mode = case["got"][False]
    assert np.all(mode["z"].numpy() == 0.0)
    assert np.array_equal(mode["next_action"].numpy(), np.tanh(mode["mu"].numpy()).astype(np.float32))


def test_conditions_on_the_test_inputs(case):
    """test_sac_cpu's conditions, unchanged; the share of rows with a tight target bound is printed, not asserted: it is 0.39 to 1.0
    here, which is why the yardstick exists."""
    ref = case["ref"][True]
    d = ref.done
    assert d.mean() >= 0.10 and (~d).mean() >= 0.10
    assert (ref.log_std_raw > 2.0).mean() >= 0.05 and (ref.log_std == 2.0).mean() >= 0.05
    assert (ref.log_std_raw < -20.0).sum() >= 1 and (ref.log_std == -20.0).sum() >= 1
    assert (np.abs(ref.next_action) > 0.999).mean() >= 0.05
    print(f"{case['name']}: target bound below 1e-3 (1 + |target|) on {(ref.target_bound < 1e-3 * (1.0 + np.abs(ref.target))).mean():.3g} of the rows")


def test_the_restatement_is_its_own_yardstick(case):
    """The correct restatement against itself: ratio <= 1 by construction, and the float64 reference is not zero anywhere it is used."""
    got = case["got"][True]
    ratios = hs.check_yardstick({k: got[k] for k in hs.SAC_OUTPUTS}, case["ref"][True], got, case["name"])
    assert max(ratios.values()) <= 1.0


# ---- planted slips ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slip", hs.SLIPS)
def test_planted_slips_fail_the_yardstick(case, slip):
    """Each slip, planted in the float32 restatement, puts some output's ratio above 8 against the correct restatement on every case it
    applies to -- by the restatement alone: no device, and no use of the rigorous bound."""
    if not hs.slip_applies(slip, case["S"]):
        assert slip in hs.SHAPE_SLIPS
        bad = _restate(case, slip)
        assert all(torch.equal(bad[k], case["got"][True][k]) for k in bad), "a slip that does not apply changed something"
        return
    bad = _restate(case, slip)
    ratios = hs.yardstick_ratios(bad, case["ref"][True], case["got"][True])
    print(f"{case['name']} {slip}: " + ", ".join(f"{k} {v[0]:.3g}" for k, v in ratios.items()))
    assert max(v[0] for v in ratios.values()) > hs.FACTOR
    with pytest.raises(AssertionError):
        hs.check_yardstick(bad, case["ref"][True], case["got"][True], slip)


def test_the_rigorous_bound_alone_misses_a_slip_at_wide_nets():
    """Why the yardstick: under [512, 512] nets at S 16 the sum of the critics in place of their minimum stays inside the target's
    rigorous bound on most live rows (test_sac_cpu asks for half of them OUTSIDE on its cases)."""
    c = hs.sac_case("S16_512x512")
    ref = c["ref"][True]
    bad = sr.SacRef(c["obs"], c["reward"], c["done"], *c["nets"], hs.GAMMA, hs.ENT_COEF, c["z"], slip="sum_not_min")
    inside = ~sr.outside(c["got"][True]["target"], bad.target, bad.target_bound)
    print(f"sum_not_min inside the bound on {int(inside[~ref.done].sum())} of {int((~ref.done).sum())} live rows")
    assert inside[~ref.done].mean() > 0.5


def test_every_shape_slip_applies_to_some_case():
    for slip in hs.SHAPE_SLIPS:
        assert any(hs.slip_applies(slip, c[0]) for c in hs.CASES.values()), slip
    assert [n for n, c in hs.CASES.items() if hs.slip_applies("second_pair_dropped", c[0])] == [n for n, c in hs.CASES.items() if c[0] == 16]


def _old_case(name):
    obs, reward, done = sr.sac_inputs(name)
    return dict(name=name, S=sr.CASES[name][0], obs=obs, reward=reward, done=done, nets=sr.sac_nets(name))


@pytest.mark.parametrize("slip,where", [("second_pair_dropped", "64x64"), ("second_pair_dropped", "odd"),
                                        ("terms_stride_16", "S16_512x512"), ("action_cols_pad32", "S16_512x512")])
def test_guard_the_shape_slips_are_invisible_where_the_shape_hides_them(slip, where):
    """The second pair does not exist at S 5 (160 pairs): the S 5 cases could not see it dropped.  Stride 16 and column pad32(10 S) are
    no slips at all at S 16 (16 = S, 160 = pad32(160)): they need the S that are not 16.  Bit for bit."""
    c = _old_case(where) if where in sr.CASES else hs.sac_case(where)
    good, bad = _restate(c), _restate(c, slip)
    assert all(torch.equal(bad[k], good[k]) for k in good) and not hs.slip_applies(slip, c["S"])


@pytest.mark.parametrize("slip", ["logp_short", "terms_stride_16", "action_cols_pad32"])
def test_guard_what_the_old_cases_did_see(slip):
    """The three other shape slips are NOT invisible at S 5: a missing position of log pi, a stride of 16 under S 5 and a critic that
    reads zeros at columns 50..54 (pad32(50) = 64) all leave sac_ref's rigorous bound there.  They stay in the planted set because the
    yardstick must see them at every S; what the old cases could not see is the second pair (above) and everything that is only
    wrong at S 16 or only at widths off the 64 grid."""
    c = _old_case("64x64")
    z = sr.noise(sr.N_ROWS, c["S"], hs.SEED, hs.DRAW)
    ref = sr.SacRef(c["obs"], c["reward"], c["done"], *c["nets"], hs.GAMMA, hs.ENT_COEF, z)
    sr.check_outputs(ref, _restate(c), "64x64")
    with pytest.raises(AssertionError):
        sr.check_outputs(ref, _restate(c, slip), "64x64 " + slip)


# ---- the head policies' nets and the directed scenario tables ---------------------------------------------------------------------------
@pytest.mark.parametrize("dist", ["gauss_clip", "gauss_tanh"])
def test_head_restatement_lies_inside_the_bound(case, dist):
    name, S, B = case["name"], case["S"], 70
    actor, log_std, critic = hs.head_nets(name, dist)
    obs = hr.injected_head_obs(np.random.default_rng(17), B, S)
    ids, zero = np.arange(B), np.zeros(B, dtype=np.int64)
    for st in (False, True):
        z = hr.noise(ids, ids, zero, S, 5) if st else None
        ref = hr.HeadRef(obs, actor, dist, log_std, z)
        want, _ = adapters.head_policy_actions(obs, actor, dist, log_std, st, 5, env_ids=ids, episode=ids, step=zero)
        hr.check_scores(ref, want.numpy(), name)
        assert (np.abs(ref.action) > 1.0).any() and (np.abs(ref.action) < 1.0).any()
        assert hs.rel_error(want.numpy(), ref.scores) < 1e-5
    y, bound = hr.value_ref(obs, critic)
    assert y.shape == (B,) and np.all(bound > 0)


@pytest.mark.parametrize("S", [1, 3, 16])
def test_directed_tables_hold_the_member_counts(S):
    kw = hs.ENV_SHAPES[S]
    t, scen = hs.directed_tables(S, kw["n_ues"])
    nues = np.asarray(t.slice_nues)
    assert nues.tolist() == scen
    want = set(hs.MEMBER_COUNTS) - ({0} if S == 1 else set())
    assert set(nues.reshape(-1).tolist()) == want
    assert np.array_equal(np.asarray(t.slice_active), (nues > 0).astype(np.int32))
    assert np.array_equal(np.asarray(t.sorted_slices), np.broadcast_to(np.arange(S), nues.shape))
