"""CPU tests of the swing references and their reverse pass (qc_swing_reference_batch, qc_swing_reference_adjoint_batch): the
restatement against the oracle's planner and trajectory, its reverse pass against central differences and against 50 digits, the host
logic of the two entry points, the exported symbols.  No GPU."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import tick_restatement as TR
from tests import swing_reference_restatement as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tr_robot(t_swing, t_stance, phases):
    return TR.GaitScheduler(t_swing, t_stance, phases), TR.FootPlanner(), TR.FootTrajectoryManager(0.08, t_swing, t_stance)


def _tr_step(gait, planner, trajs, t_stance, R, x, xdot, w, xdot_d, q, dt):
    """the front half of tick_restatement.Commander.tick: (swing_pos [12], swing_vel [12], leg_state, has_traj)"""
    gait.update(dt)
    feet = {leg: TR.forward_kinematics(leg, q[3 * i:3 * i + 3]) for i, leg in enumerate(TR.LEGS)}
    gm = gait.schedule()
    new, final = planner.positions(t_stance, R, x, xdot, w, xdot_d, feet, gm)
    if new:
        trajs.reference_states_planned(gm, {leg: (R @ feet[leg] + x, pf) for leg, pf in final.items()})
    pos, vel = np.zeros(12), np.zeros(12)
    for i, leg in enumerate(TR.LEGS):
        if gm[leg][0] == 0:
            pos[3 * i:3 * i + 3], vel[3 * i:3 * i + 3] = trajs.reference_state(leg, gm[leg][1])
    return pos, vel, [gm[leg][0] for leg in TR.LEGS], [1 if leg in trajs.traj_map else 0 for leg in TR.LEGS]


def _run_against_oracle(M, inputs, x_of_tick, dts, phase0):
    """ticks x robots: the restated forward against the oracle's classes, threaded through the record"""
    n = phase0.shape[0]
    robots = [_tr_robot(M.t_swing, M.t_stance, phase0[i]) for i in range(n)]
    state = np.zeros(n, SR.STATE_DTYPE)
    state["leg_state"] = -1
    phases = phase0.copy()
    worst, edges = 0.0, 0
    for x, dt in zip(x_of_tick, dts):
        b = dict(inputs, x=x, gait_phase=phases)
        val, state, phases, planned = SR.reference_np(M, b, state, gait_dt=dt)
        edges += int(np.unpackbits(planned[:, None], axis=1).sum())
        for i in range(n):
            pos, vel, ls, ht = _tr_step(*robots[i], M.t_stance, inputs["Rwb"][i].reshape(3, 3), x[i], inputs["xdot"][i], inputs["w"][i], inputs["xdot_d"][i],
                                        inputs["joint_q"][i], dt[i])
            assert np.array_equal(robots[i][0].phases, phases[i]) and ls == list(state["leg_state"][i]) and ht == list(state["has_traj"][i])
            fin = np.isfinite(pos) & np.isfinite(vel)
            assert np.array_equal(fin, np.isfinite(val["swing_pos"][i]) & np.isfinite(val["swing_vel"][i]))
            worst = max(worst, float(np.abs(val["swing_pos"][i] - pos)[fin].max(initial=0.0)), float(np.abs(val["swing_vel"][i] - vel)[fin].max(initial=0.0)))
    return worst, edges


def test_forward_equals_the_oracle_on_the_tick_golden_vectors():
    """tests/golden/tick_golden.json: two gaits, 10 robots, 30 jittered ticks each.  The oracle solves the 7x7 sextic system per
    trajectory where the restatement uses its inverse's columns: the two agree to the rounding of that solve, 1e-10 on positions of
    ~0.3 m and velocities of a few m/s (condition ~1e4 x EPS)."""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "tick_golden.json")))
    for c in gold["cases"]:
        M = SR.Model("golden", SR.DEFAULT_KIN, SR.DEFAULT_MODEL.planner_hip, TR.PLANNER_K, 0.08, c["t_swing"], c["t_stance"])
        inputs = {k: np.array(c["inputs"][k], float) for k in ("Rwb", "xdot", "w", "xdot_d", "joint_q")}
        worst, edges = _run_against_oracle(M, inputs, [np.array(t["x"]) for t in c["ticks"]], [np.array(t["dt"]) for t in c["ticks"]], np.array(c["phase0"]))
        print(f"gait {c['t_swing']}/{c['t_stance']}: worst |restatement - oracle| {worst:.2e}, {edges} replans")
        assert edges > 0 and worst < 1e-10


def test_forward_equals_the_oracle_on_random_states():
    rng = np.random.default_rng(7)
    n, ticks = 12, 25
    M = SR.DEFAULT_MODEL
    b, _, _ = SR.pool(M, n, seed=3)
    inputs = {k: b[k] for k in ("Rwb", "xdot", "w", "xdot_d", "joint_q")}
    phase0 = np.fmod(np.array([0.0, 0.5, 0.5, 0.0])[None] + rng.uniform(0, 1, (n, 1)), 1.0)
    xs = [b["x"] + 0.004 * t * b["xdot"] for t in range(ticks)]
    worst, edges = _run_against_oracle(M, inputs, xs, [0.02 * rng.uniform(0.5, 1.5, n) for _ in range(ticks)], phase0)
    print(f"random states: worst |restatement - oracle| {worst:.2e}, {edges} replans")
    assert edges > 0 and worst < 1e-10


@pytest.mark.parametrize("model", ["default", "odd"])
def test_reverse_pass_against_central_differences(model):
    """<bars, d outputs> along a committed direction by central differences of the restated forward (h = 1e-6: the forward is smooth
    away from the decisions, which the pool keeps 5 % of an interval away) against <reverse pass, direction>, per robot; every kind of
    the pool - first call, one and two edges, carried, cleared, all stance - is there.  Bar: 1e-7 of the scale sum |terms|: the
    truncation h^2 |f'''| ~ 1e-12 and the rounding EPS / h ~ 2e-10 are both far below."""
    M = SR.MODELS[model]
    n = 24
    b, state, dt = SR.pool(M, n)
    bars = SR.cotangents(n)
    names = ("Rwb", "x", "xdot", "w", "xdot_d", "joint_q")
    rng = np.random.default_rng(99)
    v = {k: rng.normal(0.0, 1.0, b[k].shape) for k in names}
    vs = {k: rng.normal(0.0, 1.0, (n, 12)) for k in ("p_start", "p_final")}
    _, after, phases, planned = SR.reference_np(M, b, state, gait_dt=dt)
    val, flags = SR.reference_adjoint_np(M, dict(b, gait_phase=phases), state, bars)
    assert not flags.any()
    assert planned.any() and (planned == 0).any()

    def loss(s):
        moved = dict(b, **{k: b[k] + s * v[k] for k in names})
        st = state.copy()
        st["p_start"] = state["p_start"] + s * vs["p_start"]
        st["p_final"] = state["p_final"] + s * vs["p_final"]
        out, aft, _, _ = SR.reference_np(M, moved, st, gait_dt=dt)
        # the record after the call holds p_start / p_final of every leg, replanned or passed through
        return sum((bars[k] * (out[k] if k.startswith("swing") else aft[k])).sum(axis=1) for k in SR.COTANGENTS)

    h = 1e-6
    fd = (loss(h) - loss(-h)) / (2 * h)
    an = sum((val[k + "_bar"] * v[k].reshape(n, -1)).sum(axis=1) for k in names) + sum((val[k + "_bar"] * vs[k]).sum(axis=1) for k in vs)
    scale = sum(np.abs(val[k + "_bar"] * v[k].reshape(n, -1)).sum(axis=1) for k in names) + sum(np.abs(val[k + "_bar"] * vs[k]).sum(axis=1) for k in vs) + 1.0
    err = np.abs(fd - an) / scale
    print(f"{model}: worst |fd - reverse pass| / scale {err.max():.2e}")
    assert err.max() < 1e-7
    # xdot_d enters through the planner alone: its cotangent is non-zero exactly on the replanned robots
    assert np.array_equal(np.abs(val["xdot_d_bar"]).sum(axis=1) > 0.0, planned != 0)


def test_float64_against_50_digits():
    """The float64 restatement within its own condition-sum bound of the 50-digit one on the odd model's pool - forward and reverse,
    with every accumulator -, per output; the observed worst ratios are printed and held below C_FWD / C_REF, the yardsticks of the
    device's bars (tests/test_gpu_swing_reference.py: 4 x)."""
    M = SR.ODD_MODEL
    n = 257
    b, state, dt = SR.pool(M, n)
    f_np, after, phases, planned = SR.reference_np(M, b, state, gait_dt=dt)
    f_mp, f_cond, after_mp, phases_mp, planned_mp = SR.reference_mp(M, b, state, gait_dt=dt)
    assert np.array_equal(planned, planned_mp) and np.array_equal(phases, phases_mp)
    assert np.array_equal(after["leg_state"], after_mp["leg_state"]) and np.array_equal(after["has_traj"], after_mp["has_traj"])
    for k, c in SR.C_FWD.items():
        r = SR.worst_ratio(f_np[k], f_mp[k], f_cond[k])
        print(f"forward {k}: worst ratio {r:.3f} (C_FWD {c})")
        assert r <= c
    bars, ins = SR.cotangents(n), SR.accumulators(n)
    bb = dict(b, gait_phase=phases)
    a_np, fl = SR.reference_adjoint_np(M, bb, state, bars, **ins)
    a_mp, a_cond, fl_mp = SR.reference_adjoint_mp(M, bb, state, bars, **ins)
    assert not fl.any() and not fl_mp.any()
    for k, c in SR.C_REF.items():
        r = SR.worst_ratio(a_np[k], a_mp[k], a_cond[k])
        print(f"reverse {k}: worst ratio {r:.3f} (C_REF {c})")
        assert r <= c


def test_handle_basis_is_the_sextic_basis():
    """SR.handle_basis (the elimination qc_create makes, in double) against the exact inverse.  Bar: EPS x the system's condition
    (~1e4) x the largest entry (192) = 4e-10, rounded to 1e-9; observed 4.3e-12, twelve of the 21 entries off their integers."""
    from tests import device_math_reference as DMR

    exact = DMR.sextic_basis_mp()[1].reshape(7, 3)
    got = SR.handle_basis()
    print("worst |handle basis - exact|", float(np.abs(got - exact).max()), "entries off:", int((got != exact).sum()))
    assert np.abs(got - exact).max() < 1e-9


def test_flagged_robots():
    M = SR.ODD_MODEL
    b, state, dt = SR.pool(M, 12)
    _, _, phases, planned = SR.reference_np(M, b, state, gait_dt=dt)
    bad = np.array([0.0, -0.1, np.nan, np.inf] * 3)
    b["x"][:, 2] = bad
    val, flags = SR.reference_adjoint_np(M, dict(b, gait_phase=phases), state, SR.cotangents(12))
    assert np.array_equal(flags, planned.astype(np.int32))  # every replanned leg, and no other
    for k in SR.OUTPUTS:
        assert np.isnan(val[k][planned != 0]).all() and np.isfinite(val[k][planned == 0]).all()


def test_host_logic_binary():
    """tests/cpp/swing_reference_host_test.cpp: every refusal of check_swing_reference_args and check_swing_reference_adjoint_args,
    sanitized, stand-alone."""
    import __graft_entry__ as g

    exe = g.build_host_test("swing_reference_host_test")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "swing reference host logic ok" in r.stdout


def test_exported_symbols():
    from quadruped_control_amd import _lib

    for name in ("qc_default_swing_reference", "qc_swing_reference_batch", "qc_default_swing_reference_adjoint", "qc_swing_reference_adjoint_batch"):
        assert name in _lib.EXPORTS
    if os.path.exists(_lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
        for name in ("qc_swing_reference_batch", "qc_swing_reference_adjoint_batch"):
            assert f" T {name}\n" in out
    assert ctypes.sizeof(_lib.QcSwingReferenceIo) == 4 * 8 and ctypes.sizeof(_lib.QcSwingReferenceAdjointIo) == 20 * 8
