"""The commander step (qc_commander_step_batch) and its reverse pass (qc_commander_step_adjoint_batch) restated on the CPU
(tests/test_commander_adjoint_cpu.py, tests/test_gpu_commander_adjoint.py), written from the model's equations - include/qc_balance.h,
tests/commander_restatement.py - and not from the kernels.

FORWARD  step_np: the state machine per robot (fresh command, stand latch, gait start, pending command applied) around
         commander_restatement's integrate_twist_yaw and adjoint_twist - float64, the tick's values.
REVERSE  one robot's reverse pass is written ONCE over an arithmetic (tests/leg_plant_adjoint_restatement.py: `_Float`, Python floats and
         libm; `_Mp`, 50-digit values with condition sums - a + b -> c_a + c_b, a * b -> c_a c_b, a / b -> c_a c_b / b^2, a function value
         enters with its own magnitude) and evaluated twice: adjoint_np in float64, adjoint_mp at 50 digits on the exact double inputs
         with, per output entry, the condition sum.  It is the reverse pass of the ANALYTIC function
           Rwb_d = Y Exp(d),  x_d = (x0 + (Y t)0, x1 + (Y t)1, stand_height),  xdot_d = Rwb^T (v - x x om),  w_d = Rwb^T om,
           d = cmd_dt om,  t = cmd_dt Exp(d) v,  Y = Rz(yaw of Rwb)
         with Exp by its series near zero at 50 digits - so below the forward pass's |d| < 1e-12 branch (Rb = I) the derivative is that of
         the smooth function, and at d = 0 its limit delta Rb = [delta d]x.
What is DECIDED is decided in double in both arithmetics: fresh, the stand latch, running, pending, applied, the gimbal-lock flag."""
from __future__ import annotations

import math

import mpmath as mp
import numpy as np

from tests import commander_restatement as CR
from tests.device_math_reference import DPS, EPS, mpf
from tests.leg_plant_adjoint_restatement import Cs, _Float, _Mp, _cr, _mtv, _mv
from tests.swing_reference_restatement import _out, worst_ratio  # noqa: F401 - worst_ratio is the tests' yardstick

OUTPUTS = ("twist_bar", "Vb_bar", "Rwb_bar", "x_bar", "Rwb_d_prev_bar", "x_d_prev_bar", "xdot_d_prev_bar", "w_d_prev_bar")
SIZES = {"twist_bar": 6, "Vb_bar": 6, "Rwb_bar": 9, "x_bar": 3, "Rwb_d_prev_bar": 9, "x_d_prev_bar": 3, "xdot_d_prev_bar": 3, "w_d_prev_bar": 3}
INS = ("Rwb_bar_in", "x_bar_in")
COTANGENTS = {"Rwb_d": 9, "x_d": 3, "xdot_d": 3, "w_d": 3, "Vb": 6}
# C_REF: the worst |adjoint_np - adjoint_mp| / (EPS x condition sum) per output over pool(257), as tests/test_commander_adjoint_cpu.py
# measures it (printed there: 0.907, 0.941, 1.296, 0.981 and four times 0), rounded up to one decimal with a little headroom; that test
# asserts the measurement stays below, tests/test_gpu_commander_adjoint.py derives the device's bar (4 C_REF) from it.  The four
# `_prev_bar` outputs are copies or zeros - no rounding - so their bar is 0: equality.  Never measured on the device.
C_REF = {"twist_bar": 1.0, "Vb_bar": 1.0, "Rwb_bar": 1.4, "x_bar": 1.0, "Rwb_d_prev_bar": 0.0, "x_d_prev_bar": 0.0, "xdot_d_prev_bar": 0.0, "w_d_prev_bar": 0.0}

STATE_DTYPE = np.dtype([("standing", np.int32), ("gait_running", np.int32), ("cmd_pending", np.int32), ("reserved", np.int32),
                        ("Vb", np.float64, 6), ("Rwb_d", np.float64, 9), ("x_d", np.float64, 3), ("xdot_d", np.float64, 3),
                        ("w_d", np.float64, 3)])  # == qc_commander_state
SCALARS = dict(stand_height=CR.X_STAND[2], stand_tol=CR.STAND_TOL, cmd_dt=CR.CMD_DT)


# ------------------------------------------------------------------ what is decided, in double
def decide(rec, x2, fresh, stand_height, stand_tol):
    """(standing after, run, applied) of one robot from its record before the call"""
    standing = bool(rec["standing"]) or abs(float(x2) - stand_height) < stand_tol
    running = bool(rec["gait_running"])
    pending = bool(rec["cmd_pending"]) or bool(fresh)
    return standing, standing and running, standing and running and pending


def yaw_ok(R):
    h = math.sqrt(R[0] * R[0] + R[3] * R[3])
    return h > 0.0 and h < 1e300


# ------------------------------------------------------------------ forward, float64
def step_np(state, Rwb, x, twist=None, fresh=None, stand_height=SCALARS["stand_height"], stand_tol=SCALARS["stand_tol"], cmd_dt=SCALARS["cmd_dt"]):
    """One commander step of n robots on a COPY of `state`: returns (state', out) with out = Rwb_d [n,9], x_d, xdot_d, w_d [n,3] - the
    desired state fed to the QP this tick - and run, applied uint8 [n]."""
    n = state.shape[0]
    new = state.copy()
    Rwb, x = np.asarray(Rwb, float).reshape(n, 9), np.asarray(x, float).reshape(n, 3)
    run, applied = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for i in range(n):
        f = fresh is not None and bool(fresh[i])
        standing, r, a = decide(state[i], x[i, 2], f, stand_height, stand_tol)
        rec = new[i]
        if f:
            rec["Vb"] = np.asarray(twist, float).reshape(n, 6)[i]
            rec["cmd_pending"] = 1
        rec["standing"] = int(standing)
        if standing and not state[i]["gait_running"]:
            rec["gait_running"] = 1
        if a:
            Rd, xd = CR.integrate_twist_yaw(Rwb[i], x[i], rec["Vb"], cmd_dt)
            xd[0, 2] = stand_height
            v, w = CR.adjoint_twist(Rwb[i], x[i], rec["Vb"])
            rec["Rwb_d"], rec["x_d"], rec["xdot_d"], rec["w_d"] = Rd.reshape(9), xd[0], v[0], w[0]
            rec["cmd_pending"] = 0
        run[i], applied[i] = r, a
    out = {k: new[k].copy() for k in ("Rwb_d", "x_d", "xdot_d", "w_d")}
    out.update(run=run, applied=applied)
    return new, out


# ------------------------------------------------------------------ Exp and the left Jacobian's coefficients
def _exp_float(d):
    """(Rb, A, B): Exp(d) by Rodrigues with 1 - cos from the half angle, A = (1 - cos th) / th^2, B = (th - sin th) / th^3 (series below 1e-4)"""
    th = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    Rb = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    if th == 0.0:
        return Rb, 0.5, 1.0 / 6.0
    s, co, sh = math.sin(th), math.cos(th), math.sin(0.5 * th)
    ax = [v / th for v in d]
    oc = 2.0 * sh * sh
    Rb = [oc * ax[r] * ax[j] + (co if r == j else 0.0) for r in range(3) for j in range(3)]
    Rb[1] -= s * ax[2]; Rb[3] += s * ax[2]
    Rb[2] += s * ax[1]; Rb[6] -= s * ax[1]
    Rb[5] -= s * ax[0]; Rb[7] += s * ax[0]
    q = sh / (0.5 * th)
    B = (1.0 - th * th / 20.0) / 6.0 if th < 1e-4 else (th - s) / (th * th * th)
    return Rb, 0.5 * q * q, B


def _exp_mp(d):
    """the same at 50 digits: the three coefficient functions by their series near zero, every value entering with its own magnitude"""
    dv = [a.v for a in d]
    t2 = dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]
    if t2 < mpf(10) ** -10:  # sin t / t, (1 - cos t) / t^2, (t - sin t) / t^3: 8 terms of the series leave t^16 / 16!
        a = sum((-t2) ** k / mp.factorial(2 * k + 1) for k in range(8))
        bq = sum((-t2) ** k / mp.factorial(2 * k + 2) for k in range(8))
        cq = sum((-t2) ** k / mp.factorial(2 * k + 3) for k in range(8))
    else:
        t = mp.sqrt(t2)
        a, bq, cq = mp.sin(t) / t, (1 - mp.cos(t)) / t2, (t - mp.sin(t)) / (t2 * t)
    K = [0, -dv[2], dv[1], dv[2], 0, -dv[0], -dv[1], dv[0], 0]
    Rb = [(1 if r == j else 0) + a * K[3 * r + j] + bq * (dv[r] * dv[j] - (t2 if r == j else 0)) for r in range(3) for j in range(3)]
    return [Cs(mpf(v)) for v in Rb], Cs(bq), Cs(cq)


# ------------------------------------------------------------------ one robot, reverse
def _adjoint_one(A, R, x, vb, applied, fresh, dt, bars, ins):
    c = A.const
    vec = lambda a: [c(v) for v in np.asarray(a, float).reshape(-1)]
    bar = lambda k: vec(np.zeros(COTANGENTS[k]) if bars.get(k) is None else bars[k])
    G, xa, b, cc, nb = bar("Rwb_d"), bar("x_d"), bar("xdot_d"), bar("w_d"), bar("Vb")
    Rbar = vec(np.zeros(9) if ins.get("Rwb_bar_in") is None else ins["Rwb_bar_in"])
    xb = vec(np.zeros(3) if ins.get("x_bar_in") is None else ins["x_bar_in"])
    zero = c(0.0)
    if applied:
        R, x, vb, dtc = vec(R), vec(x), vec(vb), c(dt)
        v, om = vb[0:3], vb[3:6]
        d = [o * dtc for o in om]
        Rb, Ac, Bc = _exp_mp(d) if A is _Mp else _exp_float(d)
        t = [e * dtc for e in _mv(Rb, v)]
        h = A.sqrt(R[0] * R[0] + R[3] * R[3])
        cy, sy = R[0] / h, R[3] / h
        xo = _cr(x, om)
        u = [v[k] - xo[k] for k in range(3)]
        ub, rc = _mv(R, b), _mv(R, cc)
        uxo, xxu = _cr(ub, om), _cr(x, ub)
        for r in range(3):
            for k in range(3):
                Rbar[3 * r + k] = Rbar[3 * r + k] + (u[r] * b[k] + om[r] * cc[k])
        tb = [cy * xa[0] + sy * xa[1], cy * xa[1] - sy * xa[0], zero]
        cyb = xa[0] * t[0] + xa[1] * t[1]
        syb = xa[1] * t[0] - xa[0] * t[1]
        M = [zero] * 9
        for j in range(3):
            M[j] = cy * G[j] + sy * G[3 + j] + dtc * tb[0] * v[j]
            M[3 + j] = cy * G[3 + j] - sy * G[j] + dtc * tb[1] * v[j]
            M[6 + j] = G[6 + j]
            cyb = cyb + (G[j] * Rb[j] + G[3 + j] * Rb[3 + j])
            syb = syb + (G[3 + j] * Rb[j] - G[j] * Rb[3 + j])
        q = cyb * sy - syb * cy
        Rbar[0] = Rbar[0] + sy * q / h
        Rbar[3] = Rbar[3] - cy * q / h
        N = [M[3 * r] * Rb[3 * k] + M[3 * r + 1] * Rb[3 * k + 1] + M[3 * r + 2] * Rb[3 * k + 2] for r in range(3) for k in range(3)]
        wv = [N[7] - N[5], N[2] - N[6], N[3] - N[1]]
        dw = _cr(d, wv)
        ddw = _cr(d, dw)
        rt = _mtv(Rb, tb)
        for k in range(3):
            db = wv[k] - Ac * dw[k] + Bc * ddw[k]
            nb[k] = nb[k] + (ub[k] + dtc * rt[k])
            nb[3 + k] = nb[3 + k] + (rc[k] + xxu[k] + dtc * db)
            xb[k] = xb[k] + (uxo[k] + xa[k] if k < 2 else uxo[k])
        G, xa, b, cc = [zero] * 9, [zero] * 3, [zero] * 3, [zero] * 3
    z6 = [zero] * 6
    return {"twist_bar": nb if fresh else z6, "Vb_bar": z6 if fresh else nb, "Rwb_bar": Rbar, "x_bar": xb, "Rwb_d_prev_bar": G, "x_d_prev_bar": xa,
            "xdot_d_prev_bar": b, "w_d_prev_bar": cc}


def _adjoint(A, state_before, Rwb, x, twist, fresh, bars, ins, stand_height, stand_tol, cmd_dt):
    n = state_before.shape[0]
    Rwb, x = np.asarray(Rwb, float).reshape(n, 9), np.asarray(x, float).reshape(n, 3)
    val = {k: np.zeros((n, SIZES[k])) for k in OUTPUTS}
    cond = {k: np.zeros((n, SIZES[k])) for k in OUTPUTS} if A is _Mp else None
    flags = np.zeros(n, np.int32)
    row = lambda dct, i: {k: (None if v is None else np.asarray(v, float).reshape(n, -1)[i]) for k, v in dct.items()}
    for i in range(n):
        f = fresh is not None and bool(fresh[i])
        _, _, applied = decide(state_before[i], x[i, 2], f, stand_height, stand_tol)
        vb = np.asarray(twist, float).reshape(n, 6)[i] if f else state_before[i]["Vb"]
        if applied and not yaw_ok(Rwb[i]):
            flags[i] = 1
            for k in OUTPUTS:
                val[k][i] = np.nan
            continue
        acc = _adjoint_one(A, Rwb[i], x[i], vb, applied, f, cmd_dt, row(bars, i), row(ins, i))
        for k in OUTPUTS:
            v, cs = _out(A, acc[k])
            val[k][i] = v
            if cond is not None:
                cond[k][i] = cs
    return val, cond, flags


def adjoint_np(state_before, Rwb, x, twist, fresh, bars, stand_height=SCALARS["stand_height"], stand_tol=SCALARS["stand_tol"], cmd_dt=SCALARS["cmd_dt"], **ins):
    """bars: dict over COTANGENTS of [n,k] arrays or None; ins: Rwb_bar_in, x_bar_in.  Returns (values, flags)."""
    val, _, flags = _adjoint(_Float, state_before, Rwb, x, twist, fresh, bars, ins, stand_height, stand_tol, cmd_dt)
    return val, flags


def adjoint_mp(state_before, Rwb, x, twist, fresh, bars, stand_height=SCALARS["stand_height"], stand_tol=SCALARS["stand_tol"], cmd_dt=SCALARS["cmd_dt"], **ins):
    """Returns (values, condition sums, flags) at 50 digits."""
    with mp.workdps(DPS):
        return _adjoint(_Mp, state_before, Rwb, x, twist, fresh, bars, ins, stand_height, stand_tol, cmd_dt)


# ------------------------------------------------------------------ the pool, committed seeds
KINDS = ("fresh", "held", "idle", "not_standing", "latching", "starting", "om0", "below", "above", "yaw_pi", "latch_applied")


def _rotation(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    Rz = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cr, -sr], [0.0, sr, cr]])
    return (Rz @ Ry @ Rx).reshape(9)


def pool(n=257, seed=53):
    """n robots cycling through KINDS: returns (state_before, Rwb, x, twist, fresh, kinds).
    fresh / held: running, a command applied from the twist / from the held Vb;  idle: running, nothing pending;  not_standing: the
    height is off, nothing happens;  latching: the height is reached, the gait starts;  starting: standing, a fresh command waits;
    om0: a fresh command with om = 0 EXACTLY;  below / above: |cmd_dt om| = 0.5e-12 / 2e-12, either side of the forward pass's branch;
    yaw_pi: yaw within 1e-3 ... 1e-9 of +-pi;  latch_applied: the stand latch closes in the call that applies a held command."""
    rng = np.random.default_rng(seed)
    st = np.zeros(n, STATE_DTYPE)
    Rwb, x = np.zeros((n, 9)), np.zeros((n, 3))
    twist, fresh = rng.uniform(-0.8, 0.8, (n, 6)), np.zeros(n, np.uint8)
    kinds = [KINDS[i % len(KINDS)] for i in range(n)]
    for i, kind in enumerate(kinds):
        yaw = rng.uniform(-math.pi, math.pi)
        if kind == "yaw_pi":
            yaw = rng.choice([-1.0, 1.0]) * (math.pi - 10.0 ** rng.uniform(-9, -3))
        Rwb[i] = _rotation(yaw, rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4))
        x[i] = (rng.uniform(-2, 2), rng.uniform(-2, 2), SCALARS["stand_height"] + rng.uniform(-0.004, 0.004))
        st[i]["Vb"] = rng.uniform(-0.8, 0.8, 6)
        st[i]["Rwb_d"] = _rotation(rng.uniform(-3, 3), 0.0, 0.0)
        st[i]["x_d"], st[i]["xdot_d"], st[i]["w_d"] = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
        st[i]["standing"], st[i]["gait_running"] = 1, 1
        if kind in ("fresh", "om0", "below", "above", "yaw_pi"):
            fresh[i] = 1
            st[i]["cmd_pending"] = int(rng.integers(0, 2))
        elif kind == "held":
            st[i]["cmd_pending"] = 1
        elif kind == "not_standing":
            st[i]["standing"], st[i]["gait_running"] = 0, 0
            x[i, 2] = SCALARS["stand_height"] + rng.choice([-1.0, 1.0]) * rng.uniform(0.006, 0.1)
            fresh[i] = i % 2
        elif kind == "latching":
            st[i]["standing"], st[i]["gait_running"] = 0, 0
        elif kind == "starting":
            st[i]["gait_running"] = 0
            fresh[i] = 1
        elif kind == "latch_applied":
            st[i]["standing"], st[i]["cmd_pending"] = 0, 1
        if kind == "om0":
            twist[i, 3:6] = 0.0
        elif kind in ("below", "above"):
            a = rng.normal(size=3)
            twist[i, 3:6] = a / np.linalg.norm(a) * ((0.5e-12 if kind == "below" else 2e-12) / SCALARS["cmd_dt"])
    return st, Rwb, x, twist, fresh, kinds


def cotangents(n, seed=59):
    rng = np.random.default_rng(seed)
    return {k: rng.uniform(-1.0, 1.0, (n, m)) for k, m in COTANGENTS.items()}


def accumulators(n, seed=61):
    rng = np.random.default_rng(seed)
    return {"Rwb_bar_in": rng.uniform(-1.0, 1.0, (n, 9)), "x_bar_in": rng.uniform(-1.0, 1.0, (n, 3))}
