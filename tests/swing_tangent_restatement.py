"""The forward mode of the swing legs' PD torques (qc_swing_torque_tangent_batch, include/qc_tangent.h) restated on the CPU
(tests/test_swing_tangent_cpu.py, tests/test_gpu_swing_tangent.py), written from the model's equations and not from the kernel.

One swing leg's forward chain and its derivative are written ONCE over an arithmetic (tests/leg_plant_adjoint_restatement.py: `_Float`,
Python floats and libm; `_Mp`, 50-digit values with condition sums) and evaluated twice:
  swing_tangent_np   plain float64, the IK end by the identity the kernel uses, dq_ref = J(q_ref)^-1 dp_b
  swing_tangent_mp   50 digits on the exact double inputs, the IK end by the forward derivative of legInverseKinematics AS WRITTEN -
                     the atan2 / sqrt chain of leg_plant_adjoint_restatement._ik, differentiated operation by operation -; the
                     CONDITION SUM per entry (a + b -> c_a + c_b, a * b -> c_a c_b, a / b -> c_a c_b / b^2, a function value enters
                     with its own magnitude) is the one of the J^-1 pass, the expression a double evaluation computes
(ik="chain" / ik="jacobian" selects the IK end in either arithmetic.)

Per direction and swing leg, delta the world-frame left tangent of Rwb (Rwb <- exp([delta]x) Rwb), p_b = Rwb^T pos - x (sic), v_b =
Rwb^T vel, q_ref = IK(p_b), qd = J(q_ref)^-1 v_b, H_r = d^2 FK_r / dq^2 at q_ref:
  dp_b = Rwb^T (dpos - delta x pos) - dx,  dv_b = Rwb^T (dvel - delta x vel),  dq_ref = (dIK / dp) dp_b,
  dqd = J^-1 (dv_b - B),  B_r = dq_ref^T H_r qd,  dtau = m o (kp o (dq_ref - dq) + kd o (dqd - dqdot)) + joint_tau_tan_in
m_c = not (tau_raw_c < tau_min) and not (tau_raw_c > tau_max).  A stance leg's row is joint_tau_tan_in.  FLAGS: the adjoint's
(sensitivity_swing_restatement) - bit l; the leg's row is NaN in every direction, the other legs are untouched."""
from __future__ import annotations

import math

import mpmath as mp
import numpy as np

from tests import sensitivity_swing_restatement as SW
from tests.device_math_reference import DEFAULT_KIN, DPS, EPS  # noqa: F401
from tests.leg_plant_adjoint_restatement import _cr, _Float, _ik, _in_band, _Leg, _Mp, _mtv

TANGENTS = {"Rwb_rot_tan": 3, "x_tan": 3, "swing_pos_tan": 12, "swing_vel_tan": 12, "joint_q_tan": 12, "joint_qdot_tan": 12, "joint_tau_tan_in": 12}
PER_LEG_TANGENTS = tuple(k for k, m in TANGENTS.items() if m == 12)
# the adjoint's cotangent that pairs with each tangent (joint_tau_tan_in has none: it passes through)
BAR_OF = {"swing_pos_tan": "swing_pos_bar", "swing_vel_tan": "swing_vel_bar", "joint_q_tan": "joint_q_bar", "joint_qdot_tan": "joint_qdot_bar", "x_tan": "x_bar"}
# C_ST: the worst |swing_tangent_np - swing_tangent_mp| / (EPS x condition sum) over the first 65 robots of the pool of each kinematic
# model, three directions, as tests/test_swing_tangent_cpu.py measures it, rounded up to one decimal; that test asserts the
# measurement stays below, tests/test_gpu_swing_tangent.py holds the device to 4 x it.  Never measured on the device.
# Measured: 0.4174 (default), 0.4996 (odd).
C_ST = {"default": 0.5, "odd": 0.5}
# C_SDOT: the worst gap of the pairing <joint_tau_bar, dtau - joint_tau_tan_in> = <cotangents of swing_adjoint_np, tangents>, in EPS x
# the sum of the magnitudes of all terms on both sides, the same way.  Measured: 0.6255 (default), 0.6150 (odd).
C_SDOT = {"default": 0.7, "odd": 0.7}


def random_tangents(n, K, seed=47):
    """{name: [K, n, m]}: 0.1 rad, 1 cm, 1 cm, 0.1 m/s, 0.1 rad, 1 rad/s and 1 N m normal draws"""
    rng = np.random.default_rng(seed)
    scale = {"Rwb_rot_tan": 0.1, "x_tan": 0.01, "swing_pos_tan": 0.01, "swing_vel_tan": 0.1, "joint_q_tan": 0.1, "joint_qdot_tan": 1.0, "joint_tau_tan_in": 1.0}
    return {k: rng.normal(0.0, scale[k], (K, n, m)) for k, m in TANGENTS.items()}


def _ik_forward(A, tape, dp):
    """(dIK / dp) dp by differentiating _ik's operations one by one: atan2(v, u) -> (u dv - v du) / (u^2 + v^2), sqrt -> d / (2 sqrt)"""
    x, y, z, ya, right, rt, l1, l2, l3, d, u, s3, c3, V, U, two = tape
    dx, dy, dz = dp
    dd = (two * x * dx + two * y * dy + two * z * dz) / (two * l2 * l3)
    drt = (two * y * dy + two * z * dz) / (two * rt)
    dya = dy if right else -dy
    # q1 = +-(atan2(z, +-y) + atan2(rt, -l1))
    dq1 = (ya * dz - z * dya) / (z * z + ya * ya) + (-(l1 * drt)) / (rt * rt + l1 * l1)
    if not right:
        dq1 = -dq1
    # q3 = atan2(u, d), u = -sqrt(1 - d^2): du / dd = -d / u
    du = -(d / u) * dd
    dq3 = (d * du - u * dd) / (u * u + d * d)
    # q2 = -atan2(x, rt) - atan2(V, U), V = l3 sin q3, U = l2 + l3 cos q3
    dV, dU = l3 * c3 * dq3, -(l3 * s3 * dq3)
    dq2 = -((rt * dx - x * drt) / (x * x + rt * rt)) - (U * dV - V * dU) / (V * V + U * U)
    return [dq1, dq2, dq3]


class _Forward:
    """One swing leg's forward chain in arithmetic A, from the equations of sensitivity_swing_restatement._swing_leg: what every
    direction shares.  flagged: outside the smooth domain (the adjoint's rules)."""

    def __init__(self, A, leg, R, x, pos, vel, q, qdot, kin):
        self.flagged, self.raw = True, None
        if not all(math.isfinite(v) for v in list(R) + list(x) + list(pos) + list(vel)):
            return
        c = A.const
        self.A, self.R, self.pos, self.vel = A, [c(v) for v in R], [c(v) for v in pos], [c(v) for v in vel]
        rp, vb = _mtv(self.R, self.pos), _mtv(self.R, self.vel)
        pb = [rp[k] - c(x[k]) for k in range(3)]
        qr, dv, tape = _ik(A, leg, pb, kin)
        if qr is None or not dv < 1.0:
            return
        y, z, l1 = tape[1], tape[2], tape[6]
        if A.val(y * y + z * z - l1 * l1) < 0.0:
            return
        self.L = L = _Leg(A, leg, qr, kin)
        if not _in_band(A.val(L.det), L.det_lo):
            return
        self.tape, self.qd = tape, L.solve(vb)
        self.kp, self.kd = [c(v) for v in kin.jc_kp], [c(v) for v in kin.jc_kd]
        e = []
        for k in range(3):
            turns = SW._wrap_turns(A.val(qr[k]), q[k])
            e.append(qr[k] - c(q[k]) + SW._two_pi(A, turns) if turns else qr[k] - c(q[k]))
        self.raw = [A.val(self.kp[k] * e[k] + self.kd[k] * (self.qd[k] - c(qdot[k])) + c(kin.jc_kff[k])) for k in range(3)]
        self.passes = [not self.raw[k] < kin.tau_min and not self.raw[k] > kin.tau_max for k in range(3)]
        self.flagged = False

    def tangent(self, delta, dx, dpos, dvel, dq, dqdot, ik):
        """kp o (dq_ref - dq) + kd o (dqd - dqdot), unmasked, for one direction (flat float inputs)"""
        A, c, L = self.A, self.A.const, self.L
        dl, dxA = [c(v) for v in delta], [c(v) for v in dx]
        w1, w2 = _cr(dl, self.pos), _cr(dl, self.vel)
        rp = _mtv(self.R, [c(dpos[k]) - w1[k] for k in range(3)])
        dpb = [rp[k] - dxA[k] for k in range(3)]
        dvb = _mtv(self.R, [c(dvel[k]) - w2[k] for k in range(3)])
        dqr = _ik_forward(A, self.tape, dpb) if ik == "chain" else L.solve(dpb)
        unit = lambda r: [c(1.0 if k == r else 0.0) for k in range(3)]
        B = []
        for r in range(3):
            h = L.hessian_apply(unit(r), self.qd)
            B.append(dqr[0] * h[0] + dqr[1] * h[1] + dqr[2] * h[2])
        dqd = L.solve([dvb[k] - B[k] for k in range(3)])
        return [self.kp[k] * (dqr[k] - c(dq[k])) + self.kd[k] * (dqd[k] - c(dqdot[k])) for k in range(3)]


def _swing_tangent(A, b, swing, tans, ik, kin=DEFAULT_KIN):
    """The batch in arithmetic A.  b: dict of float arrays (Rwb [n,9], x [n,3], joint_q, joint_qdot, swing_pos, swing_vel [n,12]); swing:
    [n,4] bool; tans: dict of [K, n, m] arrays (a missing one is zero).  Returns (joint_tau_tan [K,n,4,3], condition sums or None,
    flags [n], tau_raw [n,4,3])."""
    n = b["x"].shape[0]
    K = next(np.asarray(t).shape[0] for t in tans.values() if t is not None)
    arr = lambda k, m: np.asarray(b[k], np.float64).reshape(n, *m)
    R, x = arr("Rwb", (9,)), arr("x", (3,))
    q, qdot, pos, vel = (arr(k, (4, 3)) for k in ("joint_q", "joint_qdot", "swing_pos", "swing_vel"))
    t = {k: (np.zeros((K, n) + ((4, 3) if m == 12 else (3,))) if tans.get(k) is None else np.asarray(tans[k], np.float64).reshape((K, n) + ((4, 3) if m == 12 else (3,))))
         for k, m in TANGENTS.items()}
    val = t["joint_tau_tan_in"].copy()  # stance rows and masked entries: the input, exactly
    cond = np.zeros((K, n, 4, 3)) if A is _Mp else None
    flags = np.zeros(n, np.int32)
    raw = np.full((n, 4, 3), np.nan)
    for i in range(n):
        for leg in range(4):
            if not swing[i, leg]:
                continue
            F = _Forward(A, leg, R[i], x[i], pos[i, leg], vel[i, leg], q[i, leg], qdot[i, leg], kin)
            if F.flagged:
                flags[i] |= 1 << leg
                val[:, i, leg] = np.nan
                continue
            raw[i, leg] = F.raw
            for k in range(K):
                d = F.tangent(t["Rwb_rot_tan"][k, i], t["x_tan"][k, i], t["swing_pos_tan"][k, i, leg], t["swing_vel_tan"][k, i, leg],
                              t["joint_q_tan"][k, i, leg], t["joint_qdot_tan"][k, i, leg], ik)
                for c in range(3):
                    if F.passes[c]:
                        o = d[c] + A.const(val[k, i, leg, c])
                        val[k, i, leg, c] = A.val(o)
                        if cond is not None:
                            cond[k, i, leg, c] = o.c
    return val, cond, flags, raw


def swing_tangent_np(b, swing, tans, ik="jacobian", kin=DEFAULT_KIN):
    """float64: (joint_tau_tan [K,n,4,3], flags [n] int32, tau_raw [n,4,3] - NaN for stance and flagged legs)"""
    val, _, flags, raw = _swing_tangent(_Float, b, np.asarray(swing, bool), tans, ik, kin)
    return val, flags, raw


def swing_tangent_mp(b, swing, tans, ik="chain", kin=DEFAULT_KIN):
    """50 digits: (joint_tau_tan rounded to double with the IK end `ik`, the condition sums of the J^-1 pass, flags, tau_raw)"""
    with mp.workdps(DPS):
        val, cond, flags, raw = _swing_tangent(_Mp, b, np.asarray(swing, bool), tans, ik, kin)
        if ik != "jacobian":
            cond = _swing_tangent(_Mp, b, np.asarray(swing, bool), tans, "jacobian", kin)[1]
        return val, cond, flags, raw


def skew_times(delta, Rwb):
    """[delta]x Rwb, entrywise [..., 9]: what the adjoint's entrywise Rwb_bar pairs with"""
    d = np.asarray(delta, np.float64)
    R = np.asarray(Rwb, np.float64).reshape(d.shape[:-1] + (3, 3))
    S = np.zeros(d.shape[:-1] + (3, 3))
    S[..., 0, 1], S[..., 0, 2], S[..., 1, 0], S[..., 1, 2], S[..., 2, 0], S[..., 2, 1] = -d[..., 2], d[..., 1], d[..., 2], -d[..., 0], -d[..., 1], d[..., 0]
    return (S @ R).reshape(d.shape[:-1] + (9,))


def pairing(tau_bar, dtau, tans, bars, Rwb):
    """The two sides of <joint_tau_bar, dtau - joint_tau_tan_in> = <swing_pos_bar, dpos> + <swing_vel_bar, dvel> + <joint_q_bar, dq> +
    <joint_qdot_bar, dqdot> + <x_bar, dx> + <Rwb_bar, [delta]x Rwb> per (direction, robot) and the sum of the magnitudes of all terms
    on both sides.  tans: [K, n, m] arrays, bars: the adjoint's [n, ...] outputs.  Returns (lhs, rhs, terms), each [K, n]."""
    K, n = dtau.shape[:2]
    tb = np.asarray(tau_bar, np.float64).reshape(1, n, 12)
    zero = lambda m: np.zeros((K, n, m))
    diff = np.asarray(dtau, np.float64).reshape(K, n, 12) - (zero(12) if tans.get("joint_tau_tan_in") is None else np.asarray(tans["joint_tau_tan_in"]).reshape(K, n, 12))
    lhs, terms = (tb * diff).sum(axis=2), (np.abs(tb) * np.abs(diff)).sum(axis=2)
    rhs = np.zeros((K, n))
    for name, bar in BAR_OF.items():
        if tans.get(name) is None:
            continue
        m = TANGENTS[name]
        g, t = np.asarray(bars[bar], np.float64).reshape(1, n, m), np.asarray(tans[name], np.float64).reshape(K, n, m)
        rhs += (g * t).sum(axis=2)
        terms += (np.abs(g) * np.abs(t)).sum(axis=2)
    if tans.get("Rwb_rot_tan") is not None:
        g, t = np.asarray(bars["Rwb_bar"], np.float64).reshape(1, n, 9), skew_times(np.asarray(tans["Rwb_rot_tan"]).reshape(K, n, 3), np.broadcast_to(np.asarray(Rwb).reshape(1, n, 9), (K, n, 9)))
        rhs += (g * t).sum(axis=2)
        terms += (np.abs(g) * np.abs(t)).sum(axis=2)
    return lhs, rhs, terms


def exp_rotation(delta):
    """exp([delta]x), [3,3] (Rodrigues)"""
    d = np.asarray(delta, np.float64)
    th = float(np.linalg.norm(d))
    Kx = np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])
    if th == 0.0:
        return np.eye(3)
    return np.eye(3) + (math.sin(th) / th) * Kx + ((1.0 - math.cos(th)) / th ** 2) * (Kx @ Kx)


def moved(b, tans, k, h):
    """the batch moved by h along direction k of `tans` (the rotation along its left tangent); joint_tau_tan_in moves nothing"""
    n = b["x"].shape[0]
    out = dict(b)
    for name, key in (("x", "x_tan"), ("swing_pos", "swing_pos_tan"), ("swing_vel", "swing_vel_tan"), ("joint_q", "joint_q_tan"), ("joint_qdot", "joint_qdot_tan")):
        if tans.get(key) is not None:
            out[name] = np.ascontiguousarray(np.asarray(b[name]) + h * np.asarray(tans[key])[k].reshape(np.asarray(b[name]).shape))
    if tans.get("Rwb_rot_tan") is not None:
        R = np.asarray(b["Rwb"]).reshape(n, 3, 3)
        out["Rwb"] = np.ascontiguousarray(np.stack([exp_rotation(h * np.asarray(tans["Rwb_rot_tan"])[k, i]) @ R[i] for i in range(n)]).reshape(n, 9))
    return out
