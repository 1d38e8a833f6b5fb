"""High-precision references for the hand-written device math of quadruped_control_amd/csrc/qc_device.hpp
(tests/test_gpu_device_math.py).  Each one is written from the reference project's formula that the header's comments cite -
Eigen's matrix -> quaternion -> angle-axis, kinematics.cpp, numerics.cpp, trajectory.cpp - not from the device code: mpmath at
50 digits for the edge sets, np.longdouble (64-bit mantissa) for the large random sweeps."""
from __future__ import annotations

import math

import mpmath as mp
import numpy as np

EPS = 2.0 ** -52
DPS = 50
PI = 3.14159265358979323846  # numerics.cpp's PI (the double nearest pi)

# kinematics.cpp:20-47 (the geometry the CPU notebook test uses: oracle_default_kinematics / qc_default_kinematics)
XBH, YBH, ZBH, L1, L2, L3 = 0.196, 0.050, 0.0, 0.077, 0.211, 0.230
HIP = np.array([[-XBH, YBH, ZBH], [XBH, YBH, ZBH], [-XBH, -YBH, ZBH], [XBH, -YBH, ZBH]])  # RL FL RR FR
LINKS = np.array([[L1, -L2, -L3], [L1, -L2, -L3], [-L1, -L2, -L3], [-L1, -L2, -L3]])
LEG_NAMES = ("RL", "FL", "RR", "FR")
JC_KFF, JC_KP, JC_KD = (0.0, 0.0, 0.0), (40.0, 40.0, 50.0), (1.0, 1.0, 1.0)  # mit_cheetah_config.yaml:50-53


class Kin:
    """One kinematic model as the restatements take it (their optional `kin` argument): hip, links [4, 3], the joint controller's
    gains, the torque limits and the leg inertia the plant tests use with it.  No module keeps a "current" model."""

    def __init__(self, name, hip, links, jc_kp, jc_kd, jc_kff, tau_min, tau_max, leg_inertia):
        self.name = name
        self.hip, self.links = np.array(hip, np.float64).reshape(4, 3), np.array(links, np.float64).reshape(4, 3)
        self.jc_kp, self.jc_kd, self.jc_kff = tuple(map(float, jc_kp)), tuple(map(float, jc_kd)), tuple(map(float, jc_kff))
        self.tau_min, self.tau_max = float(tau_min), float(tau_max)
        self.leg_inertia = tuple(map(float, leg_inertia))
        self.hip.setflags(write=False)
        self.links.setflags(write=False)

    def det_lo(self, leg):
        """the lower end of the closed-form band of det J for this leg, from the leg's own links (swing_pd's `lo`)"""
        return max(EPS, 64.0 * EPS * float(np.abs(self.links[leg]).sum()) ** 3)

    def handle_arguments(self):
        """the keywords of BalanceController.set_kinematics for this model"""
        return dict(hip=self.hip.reshape(12), links=self.links.reshape(12), tau_min=self.tau_min, tau_max=self.tau_max, jc_kp=self.jc_kp,
                    jc_kd=self.jc_kd, jc_kff=self.jc_kff)


# the library's default model (qc_default_kinematics).  It is a degenerate point of the model space: hip z = 0, kff = 0, kd = 1, the
# same |links| on all four legs, hips that differ in sign only, tau_min = -tau_max - a kernel that reads the wrong leg's or the wrong
# joint's constant is bit-identical there.
DEFAULT_KIN = Kin("default", HIP, LINKS, JC_KP, JC_KD, JC_KFF, -20.0, 20.0, (0.02, 0.03, 0.025))
# ODD_KIN: the second model of the tests, committed as literal numbers.  Links: the defaults times the twelve factors 0.85 1.10 0.95 /
# 1.20 0.90 1.05 / 0.97 1.18 0.82 / 1.08 0.83 1.22 (signs kept; no two legs share a length, |l2| != |l3| on every leg).  Hip x, y: the
# defaults times 0.90 1.20 / 1.15 0.88 / 1.05 1.10 / 0.84 0.93; hip z non-zero, of both signs, |z| <= 0.04.  Nine distinct gains, no kd
# equal to 1, kff non-zero with mixed signs and small against the limits; asymmetric limits; an anisotropic leg inertia.
ODD_KIN = Kin("odd",
              hip=[[-0.1764, 0.060, 0.031], [0.2254, 0.044, -0.017], [-0.2058, -0.055, -0.038], [0.16464, -0.0465, 0.012]],
              links=[[0.06545, -0.2321, -0.2185], [0.0924, -0.1899, -0.2415], [-0.07469, -0.24898, -0.1886], [-0.08316, -0.17513, -0.2806]],
              jc_kp=(33.0, 47.0, 58.0), jc_kd=(0.7, 1.3, 1.9), jc_kff=(0.4, -0.25, 0.15), tau_min=-13.0, tau_max=17.0,
              leg_inertia=(0.018, 0.031, 0.024))
KINS = {"default": DEFAULT_KIN, "odd": ODD_KIN}


def mpf(x):
    return mp.mpf(float(x))


# ------------------------------------------------------------------ sin / cos
def sincos_mp(x):
    """(sin x, cos x) of the exact double x, rounded to double from 50 digits"""
    with mp.workdps(DPS):
        v = mpf(x)
        return float(mp.sin(v)), float(mp.cos(v))


def sincos_ld(x):
    v = np.asarray(x, np.longdouble)
    return np.sin(v), np.cos(v)


# ------------------------------------------------------------------ rsqrt / rcp
def rsqrt_rcp_ld(x):
    v = np.asarray(x, np.longdouble)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.longdouble(1) / np.sqrt(v), np.longdouble(1) / v


# --------------------------------------------------------- rotation log (Eigen)
def eigen_case(m):
    """The branch Eigen's quaternionbase_assign_impl takes: the trace as Eigen forms it (a double, summed in order), then
    i = 0, i = 1 if m11 > m00, i = 2 if m22 > m(i, i) -> -1 for the trace branch, else i"""
    m = np.asarray(m, float).reshape(3, 3)
    t = float(m[0, 0]) + float(m[1, 1])
    t = t + float(m[2, 2])
    if t > 0.0:
        return -1
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    return i


def angle_axis_total_mp(m):
    """Rotation3d::angleAxisTotal (rigid3d.cpp:177-179, 198-203): Eigen's Quaternion(matrix) then AngleAxis(quaternion),
    angle * axis, evaluated on the exact double entries at 50 digits.  Returns (rotvec as floats, angle as float, case)."""
    case = eigen_case(m)
    with mp.workdps(DPS):
        M = [[mpf(v) for v in row] for row in np.asarray(m, float).reshape(3, 3)]
        q = [mp.mpf(0)] * 4  # x y z w
        if case < 0:
            t = mp.sqrt(M[0][0] + M[1][1] + M[2][2] + 1)
            q[3] = t / 2
            t = mp.mpf(1) / (2 * t)
            q[0] = (M[2][1] - M[1][2]) * t
            q[1] = (M[0][2] - M[2][0]) * t
            q[2] = (M[1][0] - M[0][1]) * t
        else:
            i = case
            j, k = (i + 1) % 3, (i + 2) % 3
            t = mp.sqrt(M[i][i] - M[j][j] - M[k][k] + 1)
            q[i] = t / 2
            t = mp.mpf(1) / (2 * t)
            q[3] = (M[k][j] - M[j][k]) * t
            q[j] = (M[j][i] + M[i][j]) * t
            q[k] = (M[k][i] + M[i][k]) * t
        n = mp.sqrt(q[0] ** 2 + q[1] ** 2 + q[2] ** 2)
        if n == 0:
            return np.zeros(3), 0.0, case
        angle = 2 * mp.atan2(n, abs(q[3]))
        s = (-angle if q[3] < 0 else angle) / n
        return np.array([float(q[k] * s) for k in range(3)]), float(angle), case


def rotation_mp(axis, angle):
    """Rodrigues' rotation matrix of a unit axis and an angle, rounded entry-wise to double"""
    with mp.workdps(DPS):
        a = [mpf(v) for v in axis]
        n = mp.sqrt(sum(v * v for v in a))
        a = [v / n for v in a]
        th = mp.mpf(angle) if not isinstance(angle, float) else mpf(angle)
        c, s = mp.cos(th), mp.sin(th)
        K = [[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]
        R = [[(1 if r == cc else 0) * c + (1 - c) * a[r] * a[cc] + s * K[r][cc] for cc in range(3)] for r in range(3)]
        return np.array([[float(R[r][cc]) for cc in range(3)] for r in range(3)])


# ------------------------------------------------------------------ angle wraps
def normalize_angle_2PI_unfused(angle):
    """numerics.cpp:23-35 in float64, every operation rounded on its own (the reference's x86-64 build does not fuse)"""
    a = np.asarray(angle, np.float64)
    with np.errstate(invalid="ignore"):
        q = np.floor(a / (2.0 * PI))
        r = a - (q * 2.0) * PI
        return np.where(r < 0.0, r + 2.0 * PI, r)


def normalize_angle_PI_unfused(rad):
    """numerics.cpp:37-50, unfused float64"""
    a = np.asarray(rad, np.float64)
    with np.errstate(invalid="ignore"):
        q = np.floor((a + PI) / (2.0 * PI))
        r = (a + PI) - (q * 2.0) * PI
        r = np.where(r < 0.0, r + 2.0 * PI, r)
        return r - PI


# ------------------------------------------------------------------ leg kinematics
def leg_fk_ld(leg, q, kin=DEFAULT_KIN):
    """forwardKinematics (kinematics.cpp:81-103) in long double; q [n, 3]"""
    l1, l2, l3 = (np.longdouble(v) for v in kin.links[leg])
    q = np.asarray(q, np.longdouble)
    t1, t2, t3 = q[:, 0], q[:, 1], q[:, 2]
    h = kin.hip[leg].astype(np.longdouble)
    s1, c1, s2, c2, s23, c23 = np.sin(t1), np.cos(t1), np.sin(t2), np.cos(t2), np.sin(t2 + t3), np.cos(t2 + t3)
    return np.stack([l2 * s2 + l3 * s23 + h[0], l1 * c1 - l2 * s1 * c2 - l3 * s1 * c23 + h[1], l1 * s1 + l2 * c1 * c2 + l3 * c1 * c23 + h[2]], 1)


def leg_jacobian_ld(leg, q, kin=DEFAULT_KIN):
    """legJacobian (kinematics.cpp:162-188) in long double; q [n, 3] -> [n, 3, 3]"""
    l1, l2, l3 = (np.longdouble(v) for v in kin.links[leg])
    q = np.asarray(q, np.longdouble)
    t1, t2, t3 = q[:, 0], q[:, 1], q[:, 2]
    s1, c1, s2, c2, s23, c23 = np.sin(t1), np.cos(t1), np.sin(t2), np.cos(t2), np.sin(t2 + t3), np.cos(t2 + t3)
    z = np.zeros_like(t1)
    return np.stack([np.stack([z, l2 * c2 + l3 * c23, l3 * c23], 1),
                     np.stack([-l1 * s1 - l2 * c1 * c2 - l3 * c1 * c23, (l2 * s2 + l3 * s23) * s1, l3 * s1 * s23], 1),
                     np.stack([l1 * c1 - l2 * s1 * c2 - l3 * s1 * c23, -(l2 * s2 + l3 * s23) * c1, -l3 * s23 * c1], 1)], 1)


def _jacobian_mp(leg, q, kin=DEFAULT_KIN):
    l1, l2, l3 = (mpf(v) for v in kin.links[leg])
    t1, t2, t3 = q
    s1, c1, s2, c2, s23, c23 = mp.sin(t1), mp.cos(t1), mp.sin(t2), mp.cos(t2), mp.sin(t2 + t3), mp.cos(t2 + t3)
    return mp.matrix([[0, l2 * c2 + l3 * c23, l3 * c23],
                      [-l1 * s1 - l2 * c1 * c2 - l3 * c1 * c23, (l2 * s2 + l3 * s23) * s1, l3 * s1 * s23],
                      [l1 * c1 - l2 * s1 * c2 - l3 * s1 * c23, -(l2 * s2 + l3 * s23) * c1, -l3 * s23 * c1]])


def knee_cosine_double(leg, p, kin=DEFAULT_KIN):
    """d of legInverseKinematics as the reference's build computes it: float64, every operation rounded on its own"""
    l1, l2, l3 = (abs(float(v)) for v in kin.links[leg])
    x, y, z = (float(p[k]) - float(kin.hip[leg][k]) for k in range(3))
    num = x * x + y * y + z * z - l1 * l1 - l2 * l2 - l3 * l3
    return num / (2.0 * l2 * l3)


def leg_inverse_kinematics_mp(leg, p, d=None, kin=DEFAULT_KIN):
    """legInverseKinematics (kinematics.cpp:117-160) at 50 digits on the exact double target p (body frame); returns mp values.
    `d`: the knee cosine to use instead of the exact one (near full stretch every ulp of d is a different knee angle)."""
    l1, l2, l3 = (abs(mpf(v)) for v in kin.links[leg])
    x, y, z = (mpf(p[k]) - mpf(kin.hip[leg][k]) for k in range(3))
    if d is None:
        d = (x * x + y * y + z * z - l1 * l1 - l2 * l2 - l3 * l3) / (2 * l2 * l3)
    else:
        d = mpf(d)
    if d > 1:
        d = mp.mpf(1)
    sc = y * y + z * z - l1 * l1
    if sc < 0:
        sc = mp.mpf(0)
    if LEG_NAMES[leg] in ("FR", "RR"):
        q1 = mp.atan2(z, y) + mp.atan2(mp.sqrt(sc), -l1)
    else:
        q1 = -(mp.atan2(z, -y) + mp.atan2(mp.sqrt(sc), -l1))
    q3 = mp.atan2(-mp.sqrt(1 - d * d), d)
    q2 = -mp.atan2(x, mp.sqrt(sc)) - mp.atan2(l3 * mp.sin(q3), l2 + l3 * mp.cos(q3))
    return [q1, q2, q3], d


def _wrap_PI_mp(v):
    two_pi = 2 * mp.pi
    r = v - mp.floor((v + mp.pi) / two_pi) * two_pi
    return r


def swing_torque_mp(leg, pb, vb, q, qdot, kff=None, kp=None, kd=None, d=None, kin=DEFAULT_KIN):
    """The swing-leg torque: legInverseKinematics -> legJacobianInverse -> JointController::control (joint_controller.cpp:21-39:
    kff + kp wrap(q_ref - q) + kd (J^-1 v - qdot)).  The inverse is the exact one where J is regular; where IK makes J singular
    (the knee stretched, d clamped to 1, or folded, d = -1: sin q3 = 0 exactly) it is the pseudo-inverse of rank 2, the rank
    the device's elimination keeps there.  The error is wrapped into [-pi, pi) exactly as
    normalize_angle_PI(normalize_angle_2PI(a) - normalize_angle_2PI(b)) is mathematically.
    Returns (tau as floats, cond = sigma_1 / sigma_rank, the knee cosine d, max |J^+ vb|)."""
    kff, kp, kd = (kin.jc_kff if kff is None else kff), (kin.jc_kp if kp is None else kp), (kin.jc_kd if kd is None else kd)
    with mp.workdps(DPS):
        qr, d = leg_inverse_kinematics_mp(leg, pb, d, kin)
        J = _jacobian_mp(leg, qr, kin)
        U, S, V = mp.svd_r(J)
        order = sorted(range(3), key=lambda k: -S[k])
        rank = 3 if S[order[2]] > mp.mpf(10) ** -30 * S[order[0]] else 2
        v = [mpf(x) for x in vb]
        qd = [sum(V[k, r] * sum(U[c, k] * v[c] for c in range(3)) / S[k] for k in order[:rank]) for r in range(3)]
        cond = float(S[order[0]] / S[order[rank - 1]])
        tau = []
        for c in range(3):
            e = _wrap_PI_mp(qr[c] - mpf(q[c]))
            tau.append(float(mpf(kff[c]) + mpf(kp[c]) * e + mpf(kd[c]) * (qd[c] - mpf(qdot[c]))))
        return np.array(tau), cond, float(d), float(max(abs(x) for x in qd))


def pinv_mp(J, rank):
    """Moore-Penrose pseudo-inverse of the exact double 3x3 J, truncated to `rank` singular values, at 50 digits"""
    with mp.workdps(DPS):
        A = mp.matrix([[mpf(v) for v in row] for row in np.asarray(J, float).reshape(3, 3)])
        U, S, V = mp.svd_r(A)
        P = mp.zeros(3, 3)
        order = sorted(range(3), key=lambda k: -S[k])
        for k in order[:rank]:
            for r in range(3):
                for c in range(3):
                    P[r, c] += V[k, r] * U[c, k] / S[k]
        return P


# ------------------------------------------------------------------ sextic swing trajectory
def sextic_basis_mp():
    """Column k of A^-1 (k = start, final, centre) of the sextic system of trajectory.cpp:256-277, solved at 50 digits:
    s(0) = p0, s(1) = pf, s(1/2) = pc, zero velocity and acceleration at both ends -> (basis as a [7, 3] mp matrix,
    rounded [21] doubles in the device's [power j][k] layout)"""
    with mp.workdps(DPS):
        h = mp.mpf(1) / 2
        A = mp.matrix([[1, 0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1], [1, h, h ** 2, h ** 3, h ** 4, h ** 5, h ** 6],
                       [0, 1, 0, 0, 0, 0, 0], [0, 1, 2, 3, 4, 5, 6], [0, 0, 2, 0, 0, 0, 0], [0, 0, 2, 6, 12, 20, 30]])
        Ai = mp.inverse(A)
        B = mp.matrix(7, 3)
        for j in range(7):
            for k in range(3):
                B[j, k] = Ai[j, k]
        return B, np.array([float(B[j, k]) for j in range(7) for k in range(3)])


def track_swing_mp(basis, phase, p0, pf, swing_height, t_swing, t_stance):
    """FootTrajectoryManager::referenceState + FootTrajectory::trackTrajectory (trajectory.cpp:234-254, 360-388) at 50 digits:
    t = clamp(slope phase + y_int, 0, 1) with the manager's double-precision slope / intercept, then s(t), s'(t) of the sextic
    through (p0, pc, pf), pc = ((p0 + pf) / 2 in x, y; swing_height in z), its coefficients from the exact basis"""
    duty = t_stance / (t_swing + t_stance)
    slope = 1.0 / (1.0 - duty)
    yint = 1.0 - slope
    u = slope * phase + yint
    t = min(max(u, 0.0), 1.0)  # std::clamp (a NaN phase is handled by the caller)
    with mp.workdps(DPS):
        tt = mpf(t)
        pc = [(mpf(p0[0]) + mpf(pf[0])) / 2, (mpf(p0[1]) + mpf(pf[1])) / 2, mpf(swing_height)]
        pos, vel = [], []
        for r in range(3):
            P = [mpf(p0[r]), mpf(pf[r]), pc[r]]
            coef = [sum(basis[j, k] * P[k] for k in range(3)) for j in range(7)]
            pos.append(float(sum(coef[j] * tt ** j for j in range(7))))
            vel.append(float(sum(j * coef[j] * tt ** (j - 1) for j in range(1, 7))))
        return np.array(pos), np.array(vel), t


# ------------------------------------------------------------------ packed SPD solves
def pack_lower(M):
    N = M.shape[0]
    return np.array([M[r, c] for r in range(N) for c in range(r + 1)])


def solve_mp(M, b):
    with mp.workdps(DPS):
        A = mp.matrix([[mpf(v) for v in row] for row in M])
        x = mp.lu_solve(A, mp.matrix([mpf(v) for v in b]))
        return np.array([float(v) for v in x])


def residual_ld(M, x, b):
    """|M x - b| in long double (the backward-error check of the device solves)"""
    return np.abs(np.asarray(M, np.longdouble) @ np.asarray(x, np.longdouble) - np.asarray(b, np.longdouble))


def exact_sum(v):
    return math.fsum(float(x) for x in v)


# ------------------------------------------------------------------ tracked arithmetic (value, condition sum, rounding count)
class Tr:
    """A high-precision value `v` (an mp number or an np.longdouble array - the same code serves the 50-digit edge sets and the
    long-double sweeps) with what a double evaluation of the same expression can lose:
      c = the condition sum: sum of |terms| of the expression that produced v (|v| for an exact input),
      k = the number of roundings on the longest chain that produced v (0 for an exact input).
    To first order a double evaluation that rounds every operation once, in any order of association and with or without
    FMA contraction (contraction only removes roundings), is within k EPS c of v:
      a + b: c = c_a + c_b, k = max(k_a, k_b) + 1     (each term carries (1 + d)^k, the sum one more rounding)
      a * b: c = c_a c_b,   k = k_a + k_b + 1         (relative errors add)
      a / b: c = c_a / |b|, k = k_a + k_b + 1         (b a sum of positive terms: a norm)
      sqrt:  c = sqrt(c),   k = ceil(k / 2) + 1       (half the relative error of the argument, one rounding)"""
    __slots__ = ("v", "c", "k")

    def __init__(self, v, c=None, k=0):
        self.v, self.c, self.k = v, (abs(v) if c is None else c), k

    def __add__(a, b):
        return Tr(a.v + b.v, a.c + b.c, np.maximum(a.k, b.k) + 1)

    def __sub__(a, b):
        return Tr(a.v - b.v, a.c + b.c, np.maximum(a.k, b.k) + 1)

    def __mul__(a, b):
        return Tr(a.v * b.v, a.c * b.c, a.k + b.k + 1)

    def __truediv__(a, b):
        return Tr(a.v / b.v, a.c / abs(b.v), a.k + b.k + 1)

    def __neg__(a):
        return Tr(-a.v, a.c, a.k)


def _is_arr(v):
    return isinstance(v, np.ndarray)


def tr_sqrt(a):
    r = np.sqrt(a.v) if _is_arr(a.v) else mp.sqrt(a.v)
    rc = np.sqrt(a.c) if _is_arr(a.c) else mp.sqrt(a.c)
    return Tr(r, rc, (a.k + 1) // 2 + 1)


def tr_select(mask, a, b):
    """a where mask else b (a python bool for mp scalars, a bool array for long-double sweeps)"""
    if isinstance(mask, (bool, np.bool_)):
        return a if mask else b
    return Tr(np.where(mask, a.v, b.v), np.where(mask, a.c, b.c), np.where(mask, a.k, b.k))


def _const(like, x):
    """the exact constant x in the arithmetic of `like`"""
    if _is_arr(like):
        return Tr(np.full(like.shape, x, np.longdouble), None, 0)
    return Tr(mp.mpf(x), None, 0)


def _sincos_tr(th):
    """sin / cos of a tracked angle as sincos_joint delivers them: 2 EPS absolute (test_sincos_joint's pinned bar) plus the
    argument's own k_th roundings through |d sin| <= |d th|: condition 1 + |th|, count max(2, k_th)."""
    s, c = (np.sin(th.v), np.cos(th.v)) if _is_arr(th.v) else (mp.sin(th.v), mp.cos(th.v))
    one = _const(th.v, 1.0).v
    k = np.maximum(2, th.k)
    return Tr(s, one + abs(th.v), k), Tr(c, one + abs(th.v), k)


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _unpack(vals, shape):
    """list of Tr -> (float64 values, float64 condition sums, rounding counts), each reshaped to [..., *shape]"""
    arr = _is_arr(vals[0].v)
    if arr:
        n = vals[0].v.shape[0]
        v = np.stack([np.asarray(np.broadcast_to(t.v, (n,)), np.longdouble) for t in vals], 1)
        c = np.stack([np.asarray(np.broadcast_to(t.c, (n,)), np.float64) for t in vals], 1)
        k = np.stack([np.broadcast_to(np.asarray(t.k), (n,)) for t in vals], 1)
        return v.reshape((n,) + shape), c.reshape((n,) + shape), k.reshape((n,) + shape)
    v = np.array([float(t.v) for t in vals]).reshape(shape)
    c = np.array([float(t.c) for t in vals]).reshape(shape)
    k = np.array([int(t.k) for t in vals]).reshape(shape)
    return v, c, k


# ------------------------------------------------------------------ commander: twist integration + adjoint
def commander_decisions(Rwb, Vb, dt):
    """The two decisions of the step that are made in double, on the double values (arrays [n, ...]):
    small = almost_equal(|u(3:5) dt|, 0) = |angle - 0| < 1e-12 (numerics.cpp:18-21, trajectory.cpp:32-41), the norm formed in
    double from the rounded products - the reference's own decision.
    yaw_ok is NOT the reference's: what Drake's RollPitchYaw does at gimbal lock is not known here, and the rule below is the one the
    LIBRARY documents (commander section) - on that branch this reference restates the documented behaviour and is no
    independent witness; away from it (every pose with a yaw) the formulas are the reference's.  yaw_ok = the measured pose has a yaw to extract: h = sqrt(R00^2 + R10^2) > 0 and finite
    (below 1e300) in double - where it is not (pitch = +-pi/2 exactly, |R00|, |R10| < 1.5e-162 whose squares underflow to 0, a
    non-finite entry) the library documents yaw = 0."""
    Rwb = np.asarray(Rwb, np.float64).reshape(-1, 9)
    Vb = np.asarray(Vb, np.float64).reshape(-1, 6)
    with np.errstate(all="ignore"):
        d = Vb[:, 3:6] * dt
        angle = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        small = np.abs(angle - 0.0) < 1e-12
        h = np.sqrt(Rwb[:, 0] * Rwb[:, 0] + Rwb[:, 3] * Rwb[:, 3])
        yaw_ok = (h > 0.0) & (h < 1e300)
    return small, yaw_ok


def _commander_core(R, x, V, dt, stand_height, small, yaw_ok):
    """R[9], x[3], V[6]: lists of exact Tr; dt, stand_height: exact Tr; small, yaw_ok: the double decisions.
    trajectory.cpp:29-69: delta = u(3:5) dt, angle = |delta|; almost zero: Rbb' = I, tbb' = u(0:2) dt; else axis = delta / angle,
    Rbb' = the rotation by angle about axis (Quaternion(angle, axis).matrix(): cos I + sin [a]x + (1 - cos) a a^T),
    tbb' = Rbb' u(0:2) dt; Twb' = (Rz(yaw(Rwb)), x) (Rbb', tbb'): Rwb_d = Rz Rbb', x_d = x + Rz tbb', then x_d(2) = the stand height
    (commander_node.cpp:409).  rigid3d.cpp:259-271: Ad = [[R^T, -R^T [x]x], [0, R^T]] applied to u: xdot_d = R^T (v - x x w),
    w_d = R^T w."""
    one, zero = _const(dt.v, 1.0), _const(dt.v, 0.0)
    v, w = V[0:3], V[3:6]
    d = [w[k] * dt for k in range(3)]
    th = tr_sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    th_safe = tr_select(small, one, th)  # (the rotated branch is evaluated and discarded where the angle is almost zero)
    a = [d[k] / th_safe for k in range(3)]
    s, c = _sincos_tr(th_safe)
    oc = one - c
    K = [[None, -a[2], a[1]], [a[2], None, -a[0]], [-a[1], a[0], None]]
    Rb = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            big = oc * a[i] * a[j] + c if i == j else oc * a[i] * a[j] + s * K[i][j]
            Rb[i][j] = tr_select(small, one if i == j else zero, big)
    t = [tr_select(small, v[i] * dt, (Rb[i][0] * v[0] + Rb[i][1] * v[1] + Rb[i][2] * v[2]) * dt) for i in range(3)]
    h = tr_sqrt(R[0] * R[0] + R[3] * R[3])
    h_safe = tr_select(yaw_ok, h, one)
    cy = tr_select(yaw_ok, R[0] / h_safe, one)
    sy = tr_select(yaw_ok, R[3] / h_safe, zero)
    Rd = [cy * Rb[0][j] - sy * Rb[1][j] for j in range(3)] + [sy * Rb[0][j] + cy * Rb[1][j] for j in range(3)] + [Rb[2][j] for j in range(3)]
    xd = [x[0] + (cy * t[0] - sy * t[1]), x[1] + (sy * t[0] + cy * t[1]), stand_height]
    u = [a_ - b_ for a_, b_ in zip(v, _cross(x, w))]
    xdotd = [R[k] * u[0] + R[3 + k] * u[1] + R[6 + k] * u[2] for k in range(3)]
    wd = [R[k] * w[0] + R[3 + k] * w[1] + R[6 + k] * w[2] for k in range(3)]
    return Rd, xd, xdotd, wd


def commander_apply_mp(Rwb, x, Vb, dt, stand_height):
    """What the commander makes of a held command on the tick it applies it (trajectory.cpp:29-69, rigid3d.cpp:259-271,
    commander_node.cpp:397-428), at DPS digits on the exact double inputs, the two double decisions of commander_decisions()
    made on the doubles.  Returns dict(field -> (values, condition sums, rounding counts)) for Rwb_d [9], x_d [3], xdot_d [3],
    w_d [3], plus "small" and "yaw_ok".  A double evaluation is within count * EPS * condition sum of the value, entry by entry."""
    small, yaw_ok = commander_decisions(Rwb, Vb, dt)
    small, yaw_ok = bool(small[0]), bool(yaw_ok[0])
    with mp.workdps(DPS):
        lift = lambda arr: [Tr(mpf(v)) for v in np.asarray(arr, np.float64).reshape(-1)]
        # (a pose without a yaw may hold non-finite or underflowing entries in R00 / R10: they are not used then)
        Rl = np.asarray(Rwb, np.float64).reshape(9).copy()
        if not yaw_ok:
            Rl[0] = Rl[3] = 0.0
        Rd, xd, xdotd, wd = _commander_core(lift(Rl), lift(x), lift(Vb), Tr(mpf(dt)), Tr(mpf(stand_height)), small, yaw_ok)
        out = dict(Rwb_d=_unpack(Rd, (9,)), x_d=_unpack(xd, (3,)), xdot_d=_unpack(xdotd, (3,)), w_d=_unpack(wd, (3,)))
    out["small"], out["yaw_ok"] = small, yaw_ok
    return out


def commander_apply_ld(Rwb, x, Vb, dt, stand_height):
    """commander_apply_mp for n robots in long double (64-bit mantissa: the reference's own error is 2^-11 of the bars)."""
    small, yaw_ok = commander_decisions(Rwb, Vb, dt)
    Rl = np.asarray(Rwb, np.float64).reshape(-1, 9).copy()
    Rl[~yaw_ok, 0] = 0.0
    Rl[~yaw_ok, 3] = 0.0
    n = Rl.shape[0]
    cols = lambda arr, m: [Tr(np.asarray(arr, np.float64).reshape(n, m)[:, k].astype(np.longdouble)) for k in range(m)]
    L = lambda s: Tr(np.full(n, s, np.longdouble))
    with np.errstate(all="ignore"):
        Rd, xd, xdotd, wd = _commander_core(cols(Rl, 9), cols(x, 3), cols(Vb, 6), L(dt), L(stand_height), small, yaw_ok)
        out = dict(Rwb_d=_unpack(Rd, (9,)), x_d=_unpack(xd, (3,)), xdot_d=_unpack(xdotd, (3,)), w_d=_unpack(wd, (3,)))
    out["small"], out["yaw_ok"] = small, yaw_ok
    return out


# rounding counts of the commander step, per field and branch, as Tr counts them (test_commander_cpu pins them):
#   delta = w dt 1; |delta|^2 3 + 2 sums = 5; angle = sqrt: 4; axis = delta / angle: 6; sin, cos: max(2, 4) = 4; 1 - cos: 5;
#   (1 - cos) a_i a_j: 5 + 6 + 6 + 2 = 19; + cos or sin a_k (4 + 6 + 1 = 11): Rbb' 20;  h^2: 1 + 1 = 2, h: 2, R00 / h: 3;
#   Rwb_d = cy Rbb' - sy Rbb': 3 + 20 + 1 + 1 = 25 (rows 0, 1; row 2 = Rbb': 20);  tbb' = (Rbb' v) dt: 20 + 1 + 2 + 1 = 24;
#   x_d = x + (cy t - sy t): 24 + 3 + 1 + 1 + 1 = 30.  Almost-zero angle: Rwb_d = cy 1 - sy 0: 3 + 1 + 1 = 5; tbb' = v dt: 1; x_d: 1 + 3 + 1 + 1 + 1 = 7.
#   Without a yaw cy = 1, sy = 0 are exact: 3 fewer each.  xdot_d = R^T (v - x x w): 1 + 1 + 1 + 1 + 2 = 6; w_d = R^T w: 3.
COMMANDER_COUNTS = {"Rwb_d": 25, "x_d": 30, "xdot_d": 6, "w_d": 3}
COMMANDER_COUNTS_SMALL = {"Rwb_d": 5, "x_d": 7, "xdot_d": 6, "w_d": 3}


# ------------------------------------------------------------------ wrench target b, lever arms r, foothold
def angle_axis_total_ld(M):
    """angle_axis_total_mp for n matrices [n, 9] in long double: Eigen's branch from the double entries (eigen_case), its
    quaternion and angle-axis formulas in long double.  Returns (rotvec [n, 3] long double, angle [n])."""
    M = np.asarray(M, np.float64).reshape(-1, 3, 3)
    return _angle_axis_ld_entries(M.astype(np.longdouble), M)


def _rotation_error_tr(Rd, R, log_fn):
    """e = log(Rwb_d Rwb^T) (BC.cpp:133-136) as tracked values.  The product Re is formed in double on the device: <= 3
    roundings on each entry's sum of |terms| s_ij (two with the contraction the library is built with); the log map carries that
    to e as sum_ij |de_k / dRe_ij| 3 EPS s_ij, measured by perturbing Re entry by entry in the reference's own precision; the log
    map itself is pinned at 8 EPS max(1, angle) (test_angle_axis_total, angles up to pi - 1e-3).  With k = 8:
    c = max(1, angle) + (3 / 8) sum_ij |de_k / dRe_ij| s_ij."""
    Re = [[_dot(Rd[3 * i:3 * i + 3], R[3 * j:3 * j + 3]) for j in range(3)] for i in range(3)]
    e0, angle = log_fn([[Re[i][j].v for j in range(3)] for i in range(3)], None)
    sens = [0 * e0[0], 0 * e0[1], 0 * e0[2]]
    h = 2.0 ** -26  # a step far above the reference's own rounding and far below the map's curvature scale (pi - angle >= 1e-3)
    for i in range(3):
        for j in range(3):
            ep, _ = log_fn([[Re[a][b].v for b in range(3)] for a in range(3)], (i, j, h))
            for k in range(3):
                sens[k] = sens[k] + abs(ep[k] - e0[k]) / h * Re[i][j].c
    one = _const(angle, 1.0).v
    big = np.maximum(one, angle) if _is_arr(angle) else max(one, angle)
    return [Tr(e0[k], big + sens[k] * 3 / 8, 8) for k in range(3)], angle


def _log_mp(Re, bump):
    # (the entries are mp numbers: Eigen's branch is taken from their double roundings, as the device sees them)
    M = mp.matrix(Re)
    if bump is not None:
        M[bump[0], bump[1]] += bump[2]
    Md = np.array([[float(M[i, j]) for j in range(3)] for i in range(3)])
    case = eigen_case(Md)
    q = [mp.mpf(0)] * 4
    if case < 0:
        t = mp.sqrt(M[0, 0] + M[1, 1] + M[2, 2] + 1)
        q[3] = t / 2
        t = 1 / (2 * t)
        q[0], q[1], q[2] = (M[2, 1] - M[1, 2]) * t, (M[0, 2] - M[2, 0]) * t, (M[1, 0] - M[0, 1]) * t
    else:
        i = case
        j, k = (i + 1) % 3, (i + 2) % 3
        t = mp.sqrt(M[i, i] - M[j, j] - M[k, k] + 1)
        q[i] = t / 2
        t = 1 / (2 * t)
        q[3], q[j], q[k] = (M[k, j] - M[j, k]) * t, (M[j, i] + M[i, j]) * t, (M[k, i] + M[i, k]) * t
    n = mp.sqrt(q[0] ** 2 + q[1] ** 2 + q[2] ** 2)
    if n == 0:
        return [mp.mpf(0)] * 3, mp.mpf(0)
    angle = 2 * mp.atan2(n, abs(q[3]))
    s = (-angle if q[3] < 0 else angle) / n
    return [q[k] * s for k in range(3)], angle


def _log_ld(Re, bump):
    M = np.stack([np.stack(row, 1) for row in Re], 1).astype(np.longdouble)  # [n, 3, 3]
    if bump is not None:
        M[:, bump[0], bump[1]] += bump[2]
    # (angle_axis_total_ld takes its branch from doubles; keep the long-double entries for the formulas)
    Md = M.astype(np.float64)
    e, angle = _angle_axis_ld_entries(M, Md)
    return [e[:, k] for k in range(3)], angle


def _angle_axis_ld_entries(L, Md):
    n = L.shape[0]
    t = (Md[:, 0, 0] + Md[:, 1, 1]) + Md[:, 2, 2]
    i = np.where(Md[:, 1, 1] > Md[:, 0, 0], 1, 0)
    i = np.where(Md[:, 2, 2] > Md[np.arange(n), i, i], 2, i)
    case = np.where(t > 0.0, -1, i)
    q = np.zeros((n, 4), np.longdouble)
    with np.errstate(all="ignore"):
        m = case < 0
        tt = np.sqrt(L[:, 0, 0] + L[:, 1, 1] + L[:, 2, 2] + 1)
        inv = 1 / (2 * tt)
        q[m, 3] = (tt / 2)[m]
        q[m, 0] = ((L[:, 2, 1] - L[:, 1, 2]) * inv)[m]
        q[m, 1] = ((L[:, 0, 2] - L[:, 2, 0]) * inv)[m]
        q[m, 2] = ((L[:, 1, 0] - L[:, 0, 1]) * inv)[m]
        for c in range(3):
            m = case == c
            if not m.any():
                continue
            j, k = (c + 1) % 3, (c + 2) % 3
            tt = np.sqrt(L[:, c, c] - L[:, j, j] - L[:, k, k] + 1)
            inv = 1 / (2 * tt)
            q[m, c] = (tt / 2)[m]
            q[m, 3] = ((L[:, k, j] - L[:, j, k]) * inv)[m]
            q[m, j] = ((L[:, j, c] + L[:, c, j]) * inv)[m]
            q[m, k] = ((L[:, k, c] + L[:, c, k]) * inv)[m]
        nv = np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2 + q[:, 2] ** 2)
        angle = 2 * np.arctan2(nv, np.abs(q[:, 3]))
        s = np.where(q[:, 3] < 0, -angle, angle) / np.where(nv == 0, 1, nv)
        e = q[:, :3] * s[:, None]
        e[nv == 0] = 0
    return e, angle


def _wrench_core(P, S, feet, log_fn, lift, sic=True):
    """P: dict of lists of exact Tr (mass, kff[6], kp_p, kd_p, kp_w, kd_w [3], Ib[9]); S: dict of lists (Rwb[9], Rwb_d[9], x, x_d,
    xdot, xdot_d, w, w_d [3]); feet: 4 x [3] tracked body-frame foot positions.
    BC.cpp:126-129: xddot_d = kp_p (x_d - x) + kd_p (xdot_d - xdot), (0) += kff0 xdot_d0, (1) += kff1 xdot_d1, (2) += kff2 m 9.81;
    :133-139: wdot_d = kp_w log(Rwb_d Rwb^T) + kd_w (w_d - w), (0) += kff3 w_d0, (1) += kff4 w_d1, (1) += kff5 w_d2 (sic);
    :244-248: r_i = Rwb p_i; :251: Iw = Rwb Ib Rwb^T; :264-269: b = [m (xddot_d + g); Iw wdot_d + w_d x (Iw w_d)], g = (0, 0, -9.81).
    `sic` = False evaluates the index the line looks like it meant ((2) += kff5 w_d2): only for showing that a test tells the two apart."""
    R, Rd = S["Rwb"], S["Rwb_d"]
    g = lift(9.81)
    m = P["mass"]
    a = [P["kp_p"][k] * (S["x_d"][k] - S["x"][k]) + P["kd_p"][k] * (S["xdot_d"][k] - S["xdot"][k]) for k in range(3)]
    a[0] = a[0] + P["kff"][0] * S["xdot_d"][0]
    a[1] = a[1] + P["kff"][1] * S["xdot_d"][1]
    a[2] = a[2] + P["kff"][2] * m * g
    e, angle = _rotation_error_tr(Rd, R, log_fn)
    wd = S["w_d"]
    al = [P["kp_w"][k] * e[k] + P["kd_w"][k] * (wd[k] - S["w"][k]) for k in range(3)]
    al[0] = al[0] + P["kff"][3] * wd[0]
    al[1] = al[1] + P["kff"][4] * wd[1]
    if sic:
        al[1] = al[1] + P["kff"][5] * wd[2]
    else:
        al[2] = al[2] + P["kff"][5] * wd[2]
    b = [m * a[0], m * a[1], m * (a[2] - g)]
    Rm = [R[0:3], R[3:6], R[6:9]]
    Ib = [P["Ib"][0:3], P["Ib"][3:6], P["Ib"][6:9]]
    Iw_of = lambda vec: [_dot(Rm[k], [_dot(Ib[r], [_dot([Rm[0][c], Rm[1][c], Rm[2][c]], vec) for c in range(3)]) for r in range(3)]) for k in range(3)]
    Ia, Iwd = Iw_of(al), Iw_of(wd)
    cr = _cross(wd, Iwd)
    b += [Ia[k] + cr[k] for k in range(3)]
    r = [_dot(Rm[k], feet[i]) for i in range(4) for k in range(3)]
    return b, r, angle


def _fk_tr(leg, q, hip, links):
    """forwardKinematics (kinematics.cpp:81-103) of tracked joint angles; sin / cos as leg_trig delivers them (2 EPS absolute per
    factor; s23, c23 by the addition theorem: sum of two products)"""
    l1, l2, l3 = links[3 * leg:3 * leg + 3]
    sc = [_sincos_tr(q[k]) for k in range(3)]
    (s1, c1), (s2, c2), (s3, c3) = sc
    s23, c23 = s2 * c3 + c2 * s3, c2 * c3 - s2 * s3
    h = hip[3 * leg:3 * leg + 3]
    return [l2 * s2 + l3 * s23 + h[0], l1 * c1 - l2 * s1 * c2 - l3 * s1 * c23 + h[1], l1 * s1 + l2 * c1 * c2 + l3 * c1 * c23 + h[2]]


WRENCH_P_KEYS = (("mass", 1), ("kff", 6), ("kp_p", 3), ("kd_p", 3), ("kp_w", 3), ("kd_w", 3), ("Ib", 9))
WRENCH_S_KEYS = (("Rwb", 9), ("Rwb_d", 9), ("x", 3), ("x_d", 3), ("xdot", 3), ("xdot_d", 3), ("w", 3), ("w_d", 3))


def wrench_mp(P, state, feet_or_q, kin=None, sic=True):
    """b [6] and r [4, 3] of the balance controller's dynamics (BC.cpp:126-139, 244-269) for ONE robot at DPS digits on the exact
    doubles.  `feet_or_q` [12]: body-frame foot positions, or - with `kin` = (hip [12], links [12]) - joint angles that go through
    forwardKinematics first.  Returns dict(b=(values, condition sums, counts), r=(...), angle)."""
    with mp.workdps(DPS):
        lift = lambda v: Tr(mpf(v))
        Pl = {k: [lift(v) for v in np.asarray(P[k], np.float64).reshape(-1)] for k, _ in WRENCH_P_KEYS}
        Pl["mass"] = Pl["mass"][0]
        Sl = {k: [lift(v) for v in np.asarray(state[k], np.float64).reshape(-1)] for k, _ in WRENCH_S_KEYS}
        f = [lift(v) for v in np.asarray(feet_or_q, np.float64).reshape(-1)]
        if kin is not None:
            hip, links = ([lift(v) for v in np.asarray(a, np.float64).reshape(-1)] for a in kin)
            feet = [_fk_tr(i, f[3 * i:3 * i + 3], hip, links) for i in range(4)]
        else:
            feet = [f[3 * i:3 * i + 3] for i in range(4)]
        b, r, angle = _wrench_core(Pl, Sl, feet, _log_mp, lift, sic)
        return dict(b=_unpack(b, (6,)), r=_unpack(r, (4, 3)), angle=float(angle))


def wrench_ld(P, state, feet_or_q, kin=None, sic=True):
    """wrench_mp for n robots in long double (state arrays [n, ...], P shared)."""
    n = np.asarray(state["x"]).reshape(-1, 3).shape[0]
    L = lambda v: Tr(np.full(n, v, np.longdouble))
    cols = lambda arr, m: [Tr(np.asarray(arr, np.float64).reshape(n, m)[:, k].astype(np.longdouble)) for k in range(m)]
    with np.errstate(all="ignore"):
        Pl = {k: [L(v) for v in np.asarray(P[k], np.float64).reshape(-1)] for k, _ in WRENCH_P_KEYS}
        Pl["mass"] = Pl["mass"][0]
        Sl = {k: cols(state[k], m) for k, m in WRENCH_S_KEYS}
        f = cols(feet_or_q, 12)
        if kin is not None:
            hip, links = ([L(v) for v in np.asarray(a, np.float64).reshape(-1)] for a in kin)
            feet = [_fk_tr(i, f[3 * i:3 * i + 3], hip, links) for i in range(4)]
        else:
            feet = [f[3 * i:3 * i + 3] for i in range(4)]
        b, r, angle = _wrench_core(Pl, Sl, feet, _log_ld, L, sic)
        return dict(b=_unpack(b, (6,)), r=_unpack(r, (4, 3)), angle=np.asarray(angle, np.float64))


def _wrench_params(rng):
    """Test parameters for wrench_mp / wrench_ld with every quirk visible: kff[3..5] all different and non-zero, a full symmetric
    positive definite Ib, non-uniform gains"""
    import quadruped_control_amd as q

    P = q.cheetah_params(0.6)
    A = rng.normal(size=(3, 3))
    P["Ib"] = np.diag([0.011253, 0.036203, 0.042673]) + 0.004 * (A @ A.T) + 0.001 * (A + A.T) * np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0]])
    P["kff"] = np.array([0.3, -0.2, 0.15, 0.7, -1.1, 1.9])
    P["kp_p"], P["kd_p"] = np.array([100.0, 80.0, 130.0]), np.array([50.0, 35.0, 61.0])
    P["kp_w"], P["kd_w"] = np.array([5000.0, 4200.0, 3100.0]), np.array([500.0, 410.0, 290.0])
    return P


def _wrench_states(rng, n, max_angle=2.5):
    """n random test states for them: any Rwb, Rwb_d up to max_angle away from it"""
    from scipy.spatial.transform import Rotation

    Rw = Rotation.random(n, random_state=int(rng.integers(1 << 30)))
    ax = rng.normal(size=(n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    Rd = Rotation.from_rotvec(ax * rng.uniform(0, max_angle, (n, 1))) * Rw
    v = lambda s: rng.normal(size=(n, 3)) * s
    return dict(Rwb=Rw.as_matrix().reshape(n, 9), Rwb_d=Rd.as_matrix().reshape(n, 9), x=v(1.0), x_d=v(1.0), xdot=v(1.0), xdot_d=v(1.0), w=v(2.0),
                w_d=v(2.0), feet=rng.uniform(-0.4, 0.4, (n, 12)))


def _foothold_core(hipv, k_, t_stance, R, x, xdot, w, xdot_d, foot, half, g, foot_is_lever=False):
    """foot_planner.cpp:76-104: p_thigh = Rwb hip + x; tang = w x (Rwb foot); foothold = p_thigh + (t_stance / 2) xdot +
    k (xdot - xdot_d) + (t_stance / 2) tang + 0.5 sqrt(x(2) / g) xdot, g = 9.81; foothold(2) = 0.
    `foot_is_lever`: `foot` is Rwb foot already (the lever arm the wrench assembly computed), taken as exact."""
    Rm = [R[0:3], R[3:6], R[6:9]]
    pt = [_dot(Rm[r], hipv) + x[r] for r in range(3)]
    pc = foot if foot_is_lever else [_dot(Rm[r], foot) for r in range(3)]
    tv = _cross(w, pc)
    hs = half * t_stance
    lip = half * tr_sqrt(x[2] / g)
    return [pt[r] + (hs * xdot[r] + k_ * (xdot[r] - xdot_d[r])) + hs * tv[r] + lip * xdot[r] for r in range(2)]


def foothold_mp(planner_hip, planner_k, t_stance, Rwb, x, xdot, w, xdot_d, foot, foot_is_lever=False):
    """FootPlanner::singleFoot for one leg at DPS digits (x(2) > 0: a negative height is NaN in x and y, like std::sqrt's).
    Returns (values [3], condition sums [3], counts [3]); entry 2 is exactly 0."""
    with mp.workdps(DPS):
        l = lambda arr: [Tr(mpf(v)) for v in np.asarray(arr, np.float64).reshape(-1)]
        fh = _foothold_core(l(planner_hip), Tr(mpf(planner_k)), Tr(mpf(t_stance)), l(Rwb), l(x), l(xdot), l(w), l(xdot_d), l(foot),
                            Tr(mp.mpf(0.5)), Tr(mpf(9.81)), foot_is_lever)
        v, c, k = _unpack(fh, (2,))
        return np.append(v, 0.0), np.append(c, 0.0), np.append(k, 0)


def foothold_ld(planner_hip, planner_k, t_stance, Rwb, x, xdot, w, xdot_d, foot, foot_is_lever=False):
    """foothold_mp for n robots and one hip vector per robot ([n, 3]) in long double."""
    n = np.asarray(x).reshape(-1, 3).shape[0]
    L = lambda v: Tr(np.full(n, v, np.longdouble))
    cols = lambda arr, m: [Tr(np.asarray(arr, np.float64).reshape(n, m)[:, k].astype(np.longdouble)) for k in range(m)]
    with np.errstate(all="ignore"):
        fh = _foothold_core(cols(planner_hip, 3), L(planner_k), L(t_stance), cols(Rwb, 9), cols(x, 3), cols(xdot, 3), cols(w, 3),
                            cols(xdot_d, 3), cols(foot, 3), L(0.5), L(9.81), foot_is_lever)
        v, c, k = _unpack(fh, (2,))
    z = np.zeros((n, 1))
    return np.concatenate([v, z], 1), np.concatenate([c, z], 1), np.concatenate([k, z.astype(int)], 1)
