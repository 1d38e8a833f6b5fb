"""The forward mode of the commander step (qc_commander_step_tangent_batch, include/qc_tangent.h) restated on the CPU
(tests/test_commander_tangent_cpu.py, tests/test_gpu_commander_tangent.py), written from the model's equations and not from the kernel,
on top of tests/commander_adjoint_restatement.py: its pool and KINDS, its `decide`, its forward step and its 50-digit Exp.

One robot's derivative is written ONCE over an arithmetic (tests/leg_plant_adjoint_restatement.py: `_Float`, Python floats and libm;
`_Mp`, 50-digit values with condition sums) and evaluated twice: tangent_np in float64, tangent_mp at 50 digits on the exact double
inputs with, per output entry, the condition sum.  It is the derivative of the ANALYTIC function (Rb = Exp(d) down to d = 0), as the
adjoint's restatement is its transpose.  HELD, decided in double: fresh, the stand latch, running, pending, applied, the gimbal-lock
flag.  In the adjoint's symbols, delta = Rwb_rot_tan, dvb = fresh ? twist_tan : Vb_tan = (dv, dom):
  always       Vb_next_tan = dvb
  not applied  the four outputs are the four `_prev_` tangents
  applied      beta = Jl(d) cmd_dt dom,  dt = beta x t + cmd_dt Rb dv,
               dpsi = (cy (delta_2 R00 - delta_0 R20) - sy (delta_1 R20 - delta_2 R10)) / h
               Rwb_d_rot_tan = dpsi e_z + Y beta,  x_d_tan = (dx_0 + g_0, dx_1 + g_1, 0),  g = dpsi e_z x (Y t) + Y dt
               xdot_d_tan = Rwb^T (du - delta x u),  du = dv - dx x om - x x dom,   w_d_tan = Rwb^T (dom - delta x om)"""
from __future__ import annotations

import mpmath as mp
import numpy as np

from tests import commander_adjoint_restatement as CA
from tests.device_math_reference import DPS, EPS  # noqa: F401
from tests.leg_plant_adjoint_restatement import _cr, _Float, _Mp, _mtv, _mv
from tests.swing_reference_restatement import _out
from tests.swing_tangent_restatement import exp_rotation, skew_times

TANGENTS = {"twist_tan": 6, "Vb_tan": 6, "Rwb_rot_tan": 3, "x_tan": 3, "Rwb_d_rot_prev_tan": 3, "x_d_prev_tan": 3, "xdot_d_prev_tan": 3, "w_d_prev_tan": 3}
OUTPUTS = {"Rwb_d_rot_tan": 3, "x_d_tan": 3, "xdot_d_tan": 3, "w_d_tan": 3, "Vb_next_tan": 6}
PREV_OF = {"Rwb_d_rot_tan": "Rwb_d_rot_prev_tan", "x_d_tan": "x_d_prev_tan", "xdot_d_tan": "xdot_d_prev_tan", "w_d_tan": "w_d_prev_tan"}
# C_CT: the worst |tangent_np - tangent_mp| / (EPS x condition sum) per output over CA.pool(257), three directions, as
# tests/test_commander_tangent_cpu.py measures it on the CPU against 50 digits (printed there: 5.036, 0.982, 1.193, 1.260, and 0 for
# Vb_next_tan, a copy; the first is a yaw within 1e-4 of pi, where the y entry of Y beta is a chain of six roundings on one term), rounded up to one decimal with a little headroom; that test asserts the measurement stays below,
# tests/test_gpu_commander_tangent.py derives the device's bar (4 C_CT) from it.  Never measured on the device.
C_CT = {"Rwb_d_rot_tan": 5.1, "x_d_tan": 1.0, "xdot_d_tan": 1.2, "w_d_tan": 1.3, "Vb_next_tan": 0.0}
# C_CDOT: the worst gap of the pairing <cotangents, tangent_np's outputs> = <adjoint_np's outputs, tangents>, in EPS x the sum of the
# magnitudes of all terms on both sides, over the same pool the same way.  Measured: 0.912 (on smooth_Rwb_d, below).
C_CDOT = 1.0


def random_tangents(n, K, seed=83):
    rng = np.random.default_rng(seed)
    scale = {"twist_tan": 0.3, "Vb_tan": 0.3, "Rwb_rot_tan": 0.1, "x_tan": 0.01, "Rwb_d_rot_prev_tan": 0.1, "x_d_prev_tan": 0.01, "xdot_d_prev_tan": 0.1,
             "w_d_prev_tan": 0.1}
    return {k: rng.normal(0.0, scale[k], (K, n, m)) for k, m in TANGENTS.items()}


def _tangent_one(A, R, x, vb, applied, fresh, dt, t):
    c = A.const
    vec = lambda a: [c(v) for v in np.asarray(a, float).reshape(-1)]
    dvb = vec(t["twist_tan"] if fresh else t["Vb_tan"])
    out = {k: vec(t[p]) for k, p in PREV_OF.items()}
    out["Vb_next_tan"] = dvb
    if not applied:
        return out
    R, x, vb, dtc = vec(R), vec(x), vec(vb), c(dt)
    dl, dx = vec(t["Rwb_rot_tan"]), vec(t["x_tan"])
    v, om, dv, dom = vb[0:3], vb[3:6], dvb[0:3], dvb[3:6]
    d = [o * dtc for o in om]
    dd = [o * dtc for o in dom]
    Rb, Bj, Cj = CA._exp_mp(d) if A is _Mp else CA._exp_float(d)
    k1 = _cr(d, dd)
    k2 = _cr(d, k1)
    beta = [dd[k] + (Bj * k1[k] + Cj * k2[k]) for k in range(3)]
    tt = [e * dtc for e in _mv(Rb, v)]
    bt, rdv = _cr(beta, tt), _mv(Rb, dv)
    dtt = [bt[k] + dtc * rdv[k] for k in range(3)]
    h = A.sqrt(R[0] * R[0] + R[3] * R[3])
    cy, sy = R[0] / h, R[3] / h
    dpsi = (cy * (dl[2] * R[0] - dl[0] * R[6]) - sy * (dl[1] * R[6] - dl[2] * R[3])) / h
    yt = [cy * tt[0] - sy * tt[1], sy * tt[0] + cy * tt[1]]
    out["Rwb_d_rot_tan"] = [cy * beta[0] - sy * beta[1], sy * beta[0] + cy * beta[1], dpsi + beta[2]]
    out["x_d_tan"] = [dx[0] + ((cy * dtt[0] - sy * dtt[1]) - dpsi * yt[1]), dx[1] + ((sy * dtt[0] + cy * dtt[1]) + dpsi * yt[0]), c(0.0)]
    xo, dxo, xdo = _cr(x, om), _cr(dx, om), _cr(x, dom)
    u = [v[k] - xo[k] for k in range(3)]
    du = [dv[k] - dxo[k] - xdo[k] for k in range(3)]
    cu, co = _cr(dl, u), _cr(dl, om)
    out["xdot_d_tan"] = _mtv(R, [du[k] - cu[k] for k in range(3)])
    out["w_d_tan"] = _mtv(R, [dom[k] - co[k] for k in range(3)])
    return out


def _tangent(A, state_before, Rwb, x, twist, fresh, tans, stand_height, stand_tol, cmd_dt):
    n = state_before.shape[0]
    K = next(np.asarray(t).shape[0] for t in tans.values() if t is not None)
    t = {k: (np.zeros((K, n, m)) if tans.get(k) is None else np.asarray(tans[k], np.float64).reshape(K, n, m)) for k, m in TANGENTS.items()}
    Rwb, x = np.asarray(Rwb, float).reshape(n, 9), np.asarray(x, float).reshape(n, 3)
    val = {k: np.zeros((K, n, m)) for k, m in OUTPUTS.items()}
    cond = {k: np.zeros((K, n, m)) for k, m in OUTPUTS.items()} if A is _Mp else None
    flags = np.zeros(n, np.int32)
    for i in range(n):
        f = fresh is not None and bool(fresh[i])
        _, _, applied = CA.decide(state_before[i], x[i, 2], f, stand_height, stand_tol)
        vb = np.asarray(twist, float).reshape(n, 6)[i] if f else state_before[i]["Vb"]
        if applied and not CA.yaw_ok(Rwb[i]):
            flags[i] = 1
            for k in OUTPUTS:
                val[k][:, i] = np.nan
            continue
        for kd in range(K):
            out = _tangent_one(A, Rwb[i], x[i], vb, applied, f, cmd_dt, {name: t[name][kd, i] for name in TANGENTS})
            for name in OUTPUTS:
                v, cs = _out(A, out[name])
                val[name][kd, i] = v
                if cond is not None:
                    # (a value passed through or a constant: no rounding behind it)
                    passed = name == "Vb_next_tan" or not applied
                    cond[name][kd, i] = 0.0 if passed else cs
    if cond is not None:
        cond["x_d_tan"][:, :, 2] = 0.0  # the height's tangent is the constant 0, or the record's own
    return val, cond, flags


def tangent_np(state_before, Rwb, x, twist, fresh, tans, stand_height=CA.SCALARS["stand_height"], stand_tol=CA.SCALARS["stand_tol"], cmd_dt=CA.SCALARS["cmd_dt"]):
    """float64: (dict over OUTPUTS of [K, n, m], flags [n] int32)"""
    val, _, flags = _tangent(_Float, state_before, Rwb, x, twist, fresh, tans, stand_height, stand_tol, cmd_dt)
    return val, flags


def tangent_mp(state_before, Rwb, x, twist, fresh, tans, stand_height=CA.SCALARS["stand_height"], stand_tol=CA.SCALARS["stand_tol"], cmd_dt=CA.SCALARS["cmd_dt"]):
    """50 digits: (values rounded to double, condition sums, flags)"""
    with mp.workdps(DPS):
        return _tangent(_Mp, state_before, Rwb, x, twist, fresh, tans, stand_height, stand_tol, cmd_dt)


def pairing(bars, outs, tans, adj, Rwb, Rwb_d, Rwb_d_prev):
    """The two sides of <G, [Rwb_d_rot_tan]x Rwb_d> + <a, x_d_tan> + <b, xdot_d_tan> + <c, w_d_tan> + <Vb_next_bar, Vb_next_tan> =
    <twist_bar, twist_tan> + <Vb_bar, Vb_tan> + <Rwb_bar, [delta]x Rwb> + <x_bar, dx> + the four `_prev_` pairings per (direction,
    robot), and the sum of the magnitudes of all terms.  bars: dict over CA.COTANGENTS of [n, m]; outs: dict over OUTPUTS of [K, n, m];
    adj: the adjoint's [n, ...] outputs; Rwb_d: the forward call's output, Rwb_d_prev: the record's before it.  -> (lhs, rhs, terms) [K, n]."""
    K, n = outs["x_d_tan"].shape[:2]
    g = lambda a, m: np.broadcast_to(np.asarray(a, np.float64).reshape(1, n, m), (K, n, m))
    rot = lambda d, R: skew_times(np.asarray(d, np.float64).reshape(K, n, 3), g(R, 9))
    left = [(g(bars["Rwb_d"], 9), rot(outs["Rwb_d_rot_tan"], Rwb_d)), (g(bars["x_d"], 3), outs["x_d_tan"]), (g(bars["xdot_d"], 3), outs["xdot_d_tan"]),
            (g(bars["w_d"], 3), outs["w_d_tan"]), (g(bars["Vb"], 6), outs["Vb_next_tan"])]
    right = [(g(adj["twist_bar"], 6), tans["twist_tan"]), (g(adj["Vb_bar"], 6), tans["Vb_tan"]), (g(adj["Rwb_bar"], 9), rot(tans["Rwb_rot_tan"], Rwb)),
             (g(adj["x_bar"], 3), tans["x_tan"]), (g(adj["Rwb_d_prev_bar"], 9), rot(tans["Rwb_d_rot_prev_tan"], Rwb_d_prev)),
             (g(adj["x_d_prev_bar"], 3), tans["x_d_prev_tan"]), (g(adj["xdot_d_prev_bar"], 3), tans["xdot_d_prev_tan"]),
             (g(adj["w_d_prev_bar"], 3), tans["w_d_prev_tan"])]

    def side(pairs):
        tot, mag = np.zeros((K, n)), np.zeros((K, n))
        for a, t in pairs:
            t = np.asarray(t, np.float64).reshape(a.shape)
            tot += (a * t).sum(axis=2)
            mag += (np.abs(a) * np.abs(t)).sum(axis=2)
        return tot, mag

    (lhs, ml), (rhs, mr) = side(left), side(right)
    return lhs, rhs, ml + mr


def smooth_Rwb_d(Rwb_d, state_before, x, twist, fresh, stand_height=CA.SCALARS["stand_height"], stand_tol=CA.SCALARS["stand_tol"], cmd_dt=CA.SCALARS["cmd_dt"]):
    """The Rwb_d of the function that is differentiated.  Below |d| = 1e-12 the forward pass takes Rb = I, so its Rwb_d is Y and not
    Y Exp(d): off by |d|, thousands of EPS.  The tangent and the adjoint are those of the smooth function, so the pairing's
    [Rwb_d_rot_tan]x Rwb_d is taken on Y Exp(d) = Rwb_d Exp(d) for those robots; every other robot's row is the forward call's own."""
    out = np.asarray(Rwb_d, np.float64).reshape(-1, 9).copy()
    for i in range(out.shape[0]):
        f = fresh is not None and bool(fresh[i])
        _, _, applied = CA.decide(state_before[i], np.asarray(x).reshape(-1, 3)[i, 2], f, stand_height, stand_tol)
        d = cmd_dt * (np.asarray(twist, float).reshape(-1, 6)[i] if f else state_before[i]["Vb"])[3:6]
        if applied and float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])) < 1.0e-12:
            out[i] = (out[i].reshape(3, 3) @ exp_rotation(d)).reshape(9)
    return out


def moved(state, Rwb, x, twist, tans, k, h):
    """the records, the pose and the command moved by h along direction k of `tans` (the rotations along their left tangents)"""
    n = state.shape[0]
    st = state.copy()
    rotate = lambda R, d: np.stack([exp_rotation(h * d[i]) @ R[i].reshape(3, 3) for i in range(n)]).reshape(n, 9)
    st["Vb"] = state["Vb"] + h * tans["Vb_tan"][k]
    st["Rwb_d"] = rotate(state["Rwb_d"], tans["Rwb_d_rot_prev_tan"][k])
    for name in ("x_d", "xdot_d", "w_d"):
        st[name] = state[name] + h * tans[name + "_prev_tan"][k]
    return st, rotate(np.asarray(Rwb), tans["Rwb_rot_tan"][k]), np.asarray(x) + h * tans["x_tan"][k], np.asarray(twist) + h * tans["twist_tan"][k]
