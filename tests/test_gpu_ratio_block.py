"""-m gpu: the ratio test and the multiplier test that end a working-set recalculation (Lane::iterate, Lane::multipliers_ok: the two
Z faces of a foot as one step-length candidate, multiplier candidates with only their high word selected, `neg` on the selected
value, the directions as the negated step operand; tests/test_ratio_block_cpu.py restates them without a GPU).  The code is shared
by every lane width and form, so each body runs once at its smallest shapes: the racing 4-lane kernel at n = 1, 4 (one racing
wave), 5 (a second wave with one robot), 4 096 (the last racing size) and 4 097 (the first size past the race), cold and warm; the
one- and two-lane bodies at n = 1, 64, 65; the general and the dense form at n = 4.  Forces and status against the C oracle at
tests/test_gpu_parity.py's bar.  Handles with fzmax lowered and with fzmin raised put robots on the upper and on the lower Z face
(asserted on the returned working-set words), on all three widths.  Non-SPD and non-finite inputs still come back QC_NOT_PD with
zero forces.
"""
import numpy as np
import pytest

from tests.gpu_arrays import q  # noqa: F401
from tests.test_gpu_parity import RTOL

pytestmark = pytest.mark.gpu

SIZES = (1, 4, 5, 4096, 4097)
QC_NOT_PD = 3

_cache = {}


def _batch(q, cfg, n, **params):
    key = (cfg, n, tuple(sorted(params.items())))
    if key not in _cache:
        from oracle import c_oracle as O
        from quadruped_control_amd import workloads as W

        P = dict(q.cheetah_params(0.6), **params)
        b = (W.config2 if cfg == 2 else W.config3)(n, seed=0x7A710000 + 16 * cfg + n)
        ref, st, _ = O.control_batch(P, b, threads=8)
        _cache[key] = (P, b, ref, st)
    return _cache[key]


def _relerr(a, ref):
    scale = np.maximum(1.0, np.abs(ref).max(axis=1, keepdims=True))
    return float(np.max(np.abs(a - ref) / scale)) if a.size else 0.0


def _check(o, b, ref, ref_st, what):
    ok = ref_st == 0
    assert np.array_equal(o["status"], ref_st), (what, o["status"], ref_st)
    assert _relerr(o["grf_body"][ok], ref[ok]) < RTOL, what
    assert np.all(o["grf_body"][~ok] == 0.0), what
    assert np.all(o["grf_body"][np.repeat(b["stance"] == 0, 3, axis=1)] == 0.0), what


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cfg", (2, 3))
def test_cold_batches_match_the_oracle_across_the_race_boundary(q, cfg, n):
    P, b, ref, ref_st = _batch(q, cfg, n)
    ctl = q.BalanceController.from_params(P)
    info = ctl.query_launch(n)
    assert (info["strategies"] > 1) == (n <= 4096), (cfg, n, info)
    if n <= 4096:
        assert info["lanes_per_robot"] == 4, (cfg, n, info)
    _check(ctl.control_batch_host(b), b, ref, ref_st, (cfg, n))


@pytest.mark.parametrize("cfg", (2, 3))
def test_one_warm_started_racing_wave_matches_the_oracle(q, cfg):
    n = 4
    P, b, ref, ref_st = _batch(q, cfg, n)
    prev = dict(b)
    prev["xdot_d"] = b["xdot_d"] * 0.9
    prev["x"] = b["x"] + 1e-3
    words = q.BalanceController.from_params(P).control_batch_host(prev, want_active_set=True)["active_set"]
    for race in (None, 4):  # the planner's own choice for a warm batch, and the 4-strategy racing kernel
        ctl = q.BalanceController.from_params(P)
        if race is not None:
            ctl = ctl.set_tuning(race=race)
            assert ctl.query_launch(n, warm=True)["strategies"] == 4
        assert ctl.query_launch(n, warm=True)["lanes_per_robot"] == 4
        _check(ctl.control_batch_host(b, warm=words), b, ref, ref_st, (cfg, race))


@pytest.mark.parametrize("n", (1, 64, 65))
@pytest.mark.parametrize("group", (1, 2))
def test_one_and_two_lane_bodies_match_the_oracle(q, group, n):
    P, b, ref, ref_st = _batch(q, 3, n)
    ctl = q.BalanceController.from_params(P).set_tuning(group=group)
    assert ctl.query_launch(n)["lanes_per_robot"] == group
    _check(ctl.control_batch_host(b), b, ref, ref_st, (group, n))


@pytest.mark.parametrize("form", ("force_general", "force_dense"))
def test_general_and_dense_forms_match_the_oracle(q, form):
    n = 4
    P, b, ref, ref_st = _batch(q, 3, n)
    ctl = q.BalanceController.from_params(P).set_tuning(**{form: 1})
    _check(ctl.control_batch_host(b), b, ref, ref_st, form)


def _z_fields(words):
    """the Z fields of the working-set words (two bits per axis, six per foot: 1 = upper face, 3 = lower face)"""
    w = np.asarray(words).astype(np.uint32)
    return np.stack([(w >> np.uint32(6 * k + 4)) & np.uint32(3) for k in range(4)], axis=1)


@pytest.mark.parametrize("group", (1, 2, 4))
def test_both_z_faces_are_taken_on_every_width(q, group):
    n = 64
    seen = set()
    for params in (dict(fzmax=30.0), dict(fzmin=45.0)):
        P, b, ref, ref_st = _batch(q, 3, n, **params)
        ctl = q.BalanceController.from_params(P).set_tuning(group=group)
        assert ctl.query_launch(n)["lanes_per_robot"] == group
        o = ctl.control_batch_host(b, want_active_set=True)
        _check(o, b, ref, ref_st, (group, params))
        z = _z_fields(o["active_set"])[b["stance"] != 0]
        seen |= set(np.unique(z).tolist())
        if "fzmax" in params:
            assert (z == 1).any(), (group, params)  # the upper Z face (odd code)
        else:
            assert (z == 3).any(), (group, params)  # the lower Z face
    assert {1, 3} <= seen, (group, seen)


def test_non_spd_and_non_finite_inputs_are_not_pd_with_zero_forces(q):
    from oracle import c_oracle as O
    from quadruped_control_amd import workloads as W

    P = q.cheetah_params(0.6)
    ctl = q.BalanceController.from_params(P)
    rng = np.random.default_rng(5)
    n = 4
    b = W.config3(n)
    cases = {}
    cases["scaled"] = dict(b, Rwb=np.ascontiguousarray(b["Rwb"] * rng.uniform(0.5, 1.5, (n, 1))))
    cases["random"] = dict(b, Rwb=np.ascontiguousarray(rng.normal(size=(n, 9))), Rwb_d=np.ascontiguousarray(rng.normal(size=(n, 9))))
    cases["at_com"] = dict(b, feet=np.zeros_like(b["feet"]))
    f = b["feet"].copy().reshape(n, 4, 3); f[:, 1:] = f[:, :1]
    cases["coincident"] = dict(b, feet=np.ascontiguousarray(f.reshape(n, 12)))
    cases["km_legs"] = dict(b, feet=np.ascontiguousarray(b["feet"] * 1e3))
    cases["denormal"] = dict(b, x=np.ascontiguousarray(b["x"] + 1e-310))
    x = b["x"].copy(); x[0, 0] = np.inf; x[3, 2] = np.nan
    cases["nonfinite"] = dict(b, x=x)
    assert ctl.query_launch(n)["lanes_per_robot"] == 4 and ctl.query_launch(n)["strategies"] == 4
    for name, c in cases.items():
        o = ctl.control_batch_host(c)
        ref, st, _ = O.control_batch(P, c, threads=4)
        assert np.array_equal(o["status"], st), (name, o["status"], st)
        assert np.isfinite(o["grf_body"]).all(), name
        ok = st == 0
        tol = 1e-4 if name == "km_legs" else 1e-6  # (tests/test_gpu_properties.py::test_unphysical_inputs_match_the_oracle's bars)
        if ok.any():
            assert _relerr(o["grf_body"][ok], ref[ok]) < tol, name
        assert np.all(o["grf_body"][~ok] == 0.0), name
    o = ctl.control_batch_host(cases["nonfinite"])
    assert (o["status"][[0, 3]] == QC_NOT_PD).all() and np.all(o["grf_body"][[0, 3]] == 0.0)
