"""CPU: the legged plant step's host logic (the sanitized stand-alone program) and the closed-form cases of its restatement
(tests/leg_plant_restatement.py).  No GPU.

Pool design (shared with tests/test_gpu_leg_plant.py): stance legs are bent - knee cosine |d| <= 0.9 - and |det J| lies four
orders of magnitude above the closed-form band's lower end, before and after the step, so the 50-digit step needs no case
excluded: the exclusion cap is zero, and test_pool_margins asserts both margins."""
import os
import subprocess

import numpy as np
import pytest

from tests import leg_plant_restatement as LR
from tests import plant_restatement as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = LR.EPS
DT = 1.0 / 300.0
INERTIA = (0.02, 0.02, 0.02)


@pytest.fixture(scope="module")
def P():
    from oracle import numpy_restatement as R

    return R.cheetah_params()


def test_host_program_passes():
    """check_leg_plant_args and leg_plant_constants with every message, under the address and undefined-behaviour sanitizers"""
    import __graft_entry__ as g

    exe = g.build_host_test("leg_plant_host_test")
    assert exe is not None
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "leg plant host logic ok" in r.stdout


def _pool(n=24, seed=3):
    return LR.make_pool(n, seed)


def test_all_swing_zero_torque_is_ballistic(P):
    """No stance leg, no torque: the body falls freely (xdot' = xdot - dt g e_z, x' = x + dt xdot', w' = w for the diagonal Ib
    only up to the gyroscopic term - so w = 0 here: Rwb' = Rwb bit for bit) and the joints coast: qdot' = qdot, q' = q + dt qdot."""
    s = _pool()
    n = s["x"].shape[0]
    s["w"][:] = 0.0
    tau = np.zeros((n, 12))
    o = LR.leg_plant_step_np(P["mass"], P["Ib"], s["Rwb"], s["x"], s["xdot"], s["w"], s["joint_q"], s["joint_qdot"], tau, np.zeros((n, 4), bool), INERTIA, DT)
    v1 = s["xdot"] + DT * np.array([0.0, 0.0, -PR.G])
    assert np.array_equal(o["xdot"], v1) and np.array_equal(o["x"], s["x"] + DT * v1)
    assert np.array_equal(o["Rwb"], s["Rwb"]) and np.array_equal(o["w"], s["w"])
    assert np.array_equal(o["joint_qdot"], s["joint_qdot"]) and np.array_equal(o["joint_q"], s["joint_q"] + DT * s["joint_qdot"])
    assert (o["flags"] == 0).all()


def test_all_stance_equals_the_rigid_body_plant(P):
    """All legs stance with tau = J^T g: the recovered force is g to a few ulps of its condition (|J^-T| |J^T| |g|), and the
    body's next state equals plant_restatement's given grf_body = g and foot_world = x + Rwb FK(q) - exactly when handed the
    recovered forces, and within the propagated force error when handed g itself."""
    s = _pool()
    n = s["x"].shape[0]
    rng = np.random.default_rng(11)
    g = rng.uniform(-1, 1, (n, 4, 3)) * np.array([10.0, 10.0, 25.0]) - np.array([0.0, 0.0, 25.0])
    q = s["joint_q"].reshape(n, 4, 3)
    tau = np.array([[LR.jacobian(l, q[i, l]).T @ g[i, l] for l in range(4)] for i in range(n)])
    assert np.abs(tau).max() < 20.0
    o = LR.leg_plant_step_np(P["mass"], P["Ib"], s["Rwb"], s["x"], s["xdot"], s["w"], s["joint_q"], s["joint_qdot"], tau.reshape(n, 12), np.ones((n, 4), bool), INERTIA, DT)
    R = s["Rwb"].reshape(n, 3, 3)
    pw = np.array([[s["x"][i] + R[i] @ LR.fk(l, q[i, l]) for l in range(4)] for i in range(n)]).reshape(n, 12)
    assert np.array_equal(o["foot_world"], pw)
    same = PR.plant_step_np(P["mass"], P["Ib"], s["Rwb"], s["x"], s["xdot"], s["w"], o["g"], pw, DT)
    for k in ("Rwb", "x", "xdot", "w"):
        assert np.array_equal(o[k], same[k]), k
    # J^-T J^T g = g: each of the two 3x3 products loses at most cond(J) ulps of |g|; cond(J) <= 40 on this pool (asserted)
    cond = max(np.linalg.cond(LR.jacobian(l, q[i, l])) for i in range(n) for l in range(4))
    assert cond <= 40.0, cond
    dg = np.abs(o["g"] - g.reshape(n, 12)).max()
    assert dg <= 16 * cond * EPS * np.abs(g).max(), (dg, cond)
    ref = PR.plant_step_np(P["mass"], P["Ib"], s["Rwb"], s["x"], s["xdot"], s["w"], g.reshape(n, 12), pw, DT)
    assert np.abs(o["xdot"] - ref["xdot"]).max() <= DT * 4 * dg / P["mass"] + 4 * EPS
    assert np.abs(o["w"] - ref["w"]).max() <= DT / np.min(np.diagonal(np.asarray(P["Ib"]).reshape(3, 3))) * 4 * 0.5 * np.sqrt(3.0) * dg + 64 * EPS
    assert (o["flags"] == 0).all()


def test_pinned_feet_return_to_their_contact_points(P):
    """x' + Rwb' FK(q') = c_i for every stance leg.  The bar: IK then FK is the identity up to the conditioning of IK, which the
    50-digit step bounds here - FK moves by at most |J| |dq| for the measured stance-IK bar dq (leg_plant_restatement), |J| <= 0.52
    (the leg's length), plus the few ulps of the 0.5 m sums themselves."""
    s = _pool()
    n = s["x"].shape[0]
    mask = LR.contact_mask(n, gait_phase=s["gait_phase"])
    assert mask.any() and not mask.all()
    o = LR.leg_plant_step_np(P["mass"], P["Ib"], s["Rwb"], s["x"], s["xdot"], s["w"], s["joint_q"], s["joint_qdot"], s["joint_tau"], mask, INERTIA, DT)
    ref = [LR.leg_plant_step_mp(P["mass"], P["Ib"], *(s[k][i] for k in LR.STATE), s["joint_tau"][i], mask[i], INERTIA, DT) for i in range(n)]
    bars = LR.stance_ik_bars(o, {k: np.stack([r[k][0] for r in ref]) for k in ("joint_q", "joint_qdot")}, mask)
    bar = 0.52 * np.sqrt(3.0) * bars["joint_q"] + 16 * EPS
    R1, q1 = o["Rwb"].reshape(n, 3, 3), o["joint_q"].reshape(n, 4, 3)
    worst = 0.0
    for i in range(n):
        for l in range(4):
            if mask[i, l]:
                back = o["x"][i] + R1[i] @ LR.fk(l, q1[i, l])
                worst = max(worst, float(np.abs(back - o["foot_world"][i, 3 * l:3 * l + 3]).max()))
    print(f"pinned feet: worst |x' + Rwb' FK(q') - c| = {worst:.3e} (bar {bar:.3e})")
    assert worst <= bar
    assert (o["flags"] == 0).all()


def test_contact_rule_agrees_with_the_tick_restatement():
    """The phase rule against oracle/tick_restatement.py's GaitScheduler.phase on a sweep of phases, the ends of the stance
    interval with +-1e-12 and their neighbours included; stance bytes and the commander's gait_running override it."""
    from oracle import tick_restatement as TR

    for duty in (0.8 / 0.98, 0.5, 0.3):
        gs = TR.GaitScheduler(1.0 - duty, duty, [0.0] * 4)  # t_swing + t_stance = 1: stance_phase = duty up to a rounding
        duty_used = gs.stance_phase
        edge = [0.0, -0.0, 1e-13, -1e-13, 1e-12, -1e-12, 2e-12, -2e-12, np.nextafter(1e-12, 0), -np.nextafter(1e-12, 0), 0.999999, 1.0]
        edge += [duty_used + d for d in (0.0, 1e-13, -1e-13, 1e-12, -1e-12, 2e-12, -2e-12, 0.9e-12, 1.1e-12)]
        ph = np.array(edge + list(np.linspace(-0.1, 1.1, 241)))
        ph = np.resize(ph, (-(-ph.size // 4), 4))
        n = ph.shape[0]
        got = LR.contact_mask(n, gait_phase=ph, gait_duty=np.full(n, duty_used))
        want = np.array([[gs.phase(p) == 1 for p in row] for row in ph])
        assert np.array_equal(got, want), duty
        assert np.array_equal(LR.contact_mask(n, gait_phase=ph, default_duty=duty_used), want)
        assert got.any() and not got.all()
        # the commander's flag: all stance until the gait runs, the phase rule afterwards
        run = np.arange(n) % 2
        both = LR.contact_mask(n, gait_phase=ph, gait_duty=np.full(n, duty_used), gait_running=run)
        assert both[run == 0].all() and np.array_equal(both[run == 1], want[run == 1])
        # stance bytes win over phases
        st = (np.arange(4 * n).reshape(n, 4) % 3 == 0).astype(np.uint8) * 7
        assert np.array_equal(LR.contact_mask(n, stance=st, gait_phase=ph), st != 0)
    assert LR.contact_mask(5).all()


def test_pool_margins(P):
    """Both margins of the pool hold before and after the step: stance legs' knee cosine |d| <= 0.9 and |det J| >= 1e4 lo."""
    s = _pool(64)
    n = s["x"].shape[0]
    for mask in (np.ones((n, 4), bool), LR.contact_mask(n, gait_phase=s["gait_phase"])):
        dmax, detmin = LR.pool_margins(s["joint_q"], mask)
        assert dmax <= 0.9 and detmin >= 1e4, (dmax, detmin)
        o = LR.leg_plant_step_np(P["mass"], P["Ib"], s["Rwb"], s["x"], s["xdot"], s["w"], s["joint_q"], s["joint_qdot"], s["joint_tau"], mask, INERTIA, DT)
        dmax, detmin = LR.pool_margins(o["joint_q"], mask)
        assert dmax <= 0.9 and detmin >= 1e4, (dmax, detmin)
        assert (o["flags"] == 0).all()


def test_numpy_step_inside_the_50_digit_bars(P):
    """A plain double evaluation stays inside the derived bars (the entries that have one).  foot_world's bars are a few ulps of
    0.5 m (<= 32 EPS).  The body's bars are wide: Er charges the cofactor form of J^-T tau with the condition sums of the
    cofactors over |det J| ~ 0.01, twice (numerator and determinant), which comes to 1e6 ... 1e8 EPS for w (up to 2e-8 rad/s) and dt times
    that for Rwb, where a double evaluation is a few EPS off - a valid first-order bound, far from tight."""
    s = _pool()
    n = s["x"].shape[0]
    mask = LR.contact_mask(n, gait_phase=s["gait_phase"])
    o = LR.leg_plant_step_np(P["mass"], P["Ib"], s["Rwb"], s["x"], s["xdot"], s["w"], s["joint_q"], s["joint_qdot"], s["joint_tau"], mask, INERTIA, DT)
    worst = {}
    for i in range(n):
        ref = LR.leg_plant_step_mp(P["mass"], P["Ib"], *(s[k][i] for k in LR.STATE), s["joint_tau"][i], mask[i], INERTIA, DT)
        for k in LR.STATE + ("foot_world",):
            val, bar = ref[k]
            has = ~np.isnan(bar)
            worst[k] = max(worst.get(k, 0.0), PR.worst_over_bar(o[k][i][has], (val[has], bar[has])))
        assert ref["foot_world"][1].max() <= 32 * EPS and ref["w"][1].max() <= 1e-7
        assert np.abs(ref["knee"][mask[i]]).max() <= 0.9
    print(f"numpy step / bar: {worst}")
    assert max(worst.values()) <= 1.0, worst


def test_numpy_step_inside_the_50_digit_bars_at_the_odd_model(P):
    """The same comparison at ODD_KIN with its anisotropic leg inertia: the pool rebuilt under the model (torques through the model's
    Jacobians, inside its limits), no robot flagged by the float64 step, both margins before and after the step against each leg's
    own band, and the float64 step inside the derived bars of the 50-digit step."""
    from tests.device_math_reference import ODD_KIN as K

    s = LR.make_pool(24, 3, K)
    n = s["x"].shape[0]
    assert K.tau_min < s["joint_tau"].min() and s["joint_tau"].max() < K.tau_max and len(set(K.leg_inertia)) == 3
    for mask in (np.ones((n, 4), bool), LR.contact_mask(n, gait_phase=s["gait_phase"])):
        o = LR.leg_plant_step_np(P["mass"], P["Ib"], *(s[k] for k in LR.STATE), s["joint_tau"], mask, K.leg_inertia, DT, kin=K)
        assert (o["flags"] == 0).all()
        for jq in (s["joint_q"], o["joint_q"]):
            dmax, detmin = LR.pool_margins(jq, mask, K)
            assert dmax <= 0.9 and detmin >= 1e4, (dmax, detmin)
    assert mask.any() and not mask.all()
    worst = {}
    for i in range(n):
        ref = LR.leg_plant_step_mp(P["mass"], P["Ib"], *(s[k][i] for k in LR.STATE), s["joint_tau"][i], mask[i], K.leg_inertia, DT, kin=K)
        for k in LR.STATE + ("foot_world",):
            val, bar = ref[k]
            has = ~np.isnan(bar)
            worst[k] = max(worst.get(k, 0.0), PR.worst_over_bar(o[k][i][has], (val[has], bar[has])))
        assert np.abs(ref["knee"][mask[i]]).max(initial=0.0) <= 0.9
    print(f"numpy step / bar at the odd model: {worst}")
    assert max(worst.values()) <= 1.0, worst
