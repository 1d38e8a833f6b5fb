"""The legged plant step of qc_leg_plant_step_batch restated on the CPU (tests/test_leg_plant_cpu.py, tests/test_gpu_leg_plant.py),
written from the model's equations - include/qc_balance.h - and not from the kernel.  Per robot:

  contact mask: `stance` bytes, else the phase rule (gait.cpp:125-134, 1e-12 slack) on the phases as they are, else all stance;
                a commander state with gait_running == 0 is all stance
  stance leg i: p_i = FK(q_i), J_i = legJacobian(q_i), g_i = J_i^-T tau_i (cofactors over det inside the band, the pseudo-inverse
                of J_i^T and flag bit i outside), f_i = -Rwb g_i at r_i = Rwb p_i, pinned at c_i = x + r_i
  swing leg:    qdot' = qdot + dt (tau / I),  q' = q + dt qdot'
  body:         the step of tests/plant_restatement.py with grf_body = g (0 for swing legs) and foot_world = c
  stance leg:   p_i' = Rwb'^T (c_i - x'),  q_i' = legInverseKinematics(p_i'),  qdot_i' = wrapPI(q_i' - q_i) / dt,
                flag bit 4 + i when d > 1 (clamped) or not d >= -1
  foot_world:   c_i = x + Rwb FK(q_i) for all four legs (the state the step read)

leg_plant_step_np is plain float64 numpy / math over a batch.  leg_plant_step_mp evaluates one robot at 50 digits on the exact
double inputs in plant_restatement's tracked arithmetic (Er), so that Rwb, x, xdot, w, foot_world and the swing legs' joint_q /
joint_qdot come with the bar a double evaluation of the same chain of operations meets: sines and cosines of the joint angles
enter with sincos_joint's pinned 2 EPS (tests/test_gpu_device_math.py::test_sincos_joint), everything else follows the Er rules.

What has NO derivable bar here: joint_q and joint_qdot of a STANCE leg.  They come out of five atan2 of lengths that are
themselves rounded, behind the whole body step, and qdot' divides an IK difference by dt.  Their bar is MEASURED ON THE CPU and
never on the device: the largest deviation of leg_plant_step_np from the 50-digit values over the test pool, times
IK_BAR_MARGIN (stance_ik_bars).  IK_BAR_MARGIN = 8: the pool maximum is a sample of one legitimate double evaluation (libm's
atan2 / sin / cos at <= 1 ulp, no contraction); the device is another (its library's atan2 at <= 2 ulp, sincos_joint at 2 EPS,
FMA contraction in y^2 + z^2 - l1^2 and in 1 - d^2), so each of the ~4 rounded inputs of an atan2 may be off by twice as much
(x 2 ... 4), and a maximum over a finite pool underestimates the supremum (x 2)."""
from __future__ import annotations

import math

import mpmath as mp
import numpy as np

from tests import plant_restatement as PR
from tests.device_math_reference import DEFAULT_KIN, DPS, EPS, LINKS, _cross, mpf
from tests.plant_restatement import Er, er_sinc_cos, er_sqrt

G = PR.G
PI = math.pi
IK_BAR_MARGIN = 8.0
SINCOS_EPS = 2.0  # sincos_joint's pinned absolute bar, in EPS
DET_LO = max(EPS, 64.0 * EPS * float(np.abs(LINKS[0]).sum()) ** 3)  # the lower end of the closed-form band (swing_pd's `lo`) at the default model:
# all four legs share it there; at another model it is per leg, from that leg's own links (Kin.det_lo)
DET_HI = 2.0 ** 52
STATE = ("Rwb", "x", "xdot", "w", "joint_q", "joint_qdot")


# ------------------------------------------------------------------ the contact rule
def contact_mask(n, stance=None, gait_phase=None, gait_duty=None, default_duty=0.8 / 0.98, gait_running=None):
    """[n, 4] bool.  gait_running: [n] ints of the commander states, or None."""
    if stance is not None:
        m = np.asarray(stance).reshape(n, 4) != 0
    elif gait_phase is not None:
        ph = np.asarray(gait_phase, np.float64).reshape(n, 4)
        duty = np.full(n, default_duty) if gait_duty is None else np.asarray(gait_duty, np.float64).reshape(n)
        ge0 = (ph > 0.0) | (np.abs(ph) < 1.0e-12)
        le = (ph < duty[:, None]) | (np.abs(ph - duty[:, None]) < 1.0e-12)
        m = ge0 & le
    else:
        m = np.ones((n, 4), bool)
    if gait_running is not None:
        m = m | (np.asarray(gait_running).reshape(n, 1) == 0)
    return m


# ------------------------------------------------------------------ leg kinematics, double
def fk(leg, q, kin=DEFAULT_KIN):
    l1, l2, l3 = kin.links[leg]
    t1, t2, t3 = q
    return np.array([l2 * math.sin(t2) + l3 * math.sin(t2 + t3), l1 * math.cos(t1) - l2 * math.sin(t1) * math.cos(t2) - l3 * math.sin(t1) * math.cos(t2 + t3),
                     l1 * math.sin(t1) + l2 * math.cos(t1) * math.cos(t2) + l3 * math.cos(t1) * math.cos(t2 + t3)]) + kin.hip[leg]


def jacobian(leg, q, kin=DEFAULT_KIN):
    l1, l2, l3 = kin.links[leg]
    t1, t2, t3 = q
    s1, c1, s2, c2, s23, c23 = math.sin(t1), math.cos(t1), math.sin(t2), math.cos(t2), math.sin(t2 + t3), math.cos(t2 + t3)
    a, b = l2 * c2 + l3 * c23, l2 * s2 + l3 * s23
    return np.array([[0.0, a, l3 * c23], [-l1 * s1 - a * c1, b * s1, l3 * s1 * s23], [l1 * c1 - a * s1, -b * c1, -l3 * s23 * c1]])


def det3(J):
    return float(J[0, 0] * (J[1, 1] * J[2, 2] - J[1, 2] * J[2, 1]) + J[0, 1] * (J[1, 2] * J[2, 0] - J[1, 0] * J[2, 2]) +
                 J[0, 2] * (J[1, 0] * J[2, 1] - J[1, 1] * J[2, 0]))


def _rank(A):
    """the device's rank rule in the pseudo-inverse band: at most two pivots, the second only above 1e-9 of the first"""
    A = np.array(A, float)
    rank, piv1 = 0, 0.0
    for k in range(2):
        i, j = np.unravel_index(np.argmax(np.abs(A)), A.shape)
        best = abs(A[i, j])
        if k == 0:
            piv1 = best
        if not (best > 0.0 if k == 0 else (rank == 1 and best > 1e-9 * piv1)):
            break
        A -= np.outer(A[:, j].copy(), A[i, :].copy() / A[i, j])
        rank = k + 1
    return rank


def force_from_torque(leg, q, tau, kin=DEFAULT_KIN):
    """(g, singular): g = J^-T tau inside the band (the leg's own: Kin.det_lo), pinv(J^T) tau with the device's rank rule outside"""
    J = jacobian(leg, q, kin)
    d = det3(J)
    if math.isnan(d):
        return np.full(3, np.nan), False
    if kin.det_lo(leg) <= abs(d) <= DET_HI:
        return np.linalg.solve(J.T, np.asarray(tau, float)), False
    rank = _rank(J.T)
    U, s, Vt = np.linalg.svd(J.T)
    g = np.zeros(3)
    for k in range(rank):
        g += Vt[k] * (U[:, k] @ tau) / s[k]
    return g, True


def knee_cosine(leg, p, kin=DEFAULT_KIN):
    """d of legInverseKinematics, rounded term by term as the reference's build does"""
    x, y, z = (float(v) for v in np.asarray(p, float) - kin.hip[leg])
    l1, l2, l3 = (abs(float(v)) for v in kin.links[leg])
    return (x * x + y * y + z * z - l1 * l1 - l2 * l2 - l3 * l3) / (2.0 * l2 * l3)


def _sqrt(v):
    return math.sqrt(v) if v >= 0.0 else float("nan")


def ik(leg, p, kin=DEFAULT_KIN):
    """(q, out_of_reach): kinematics.cpp:117-160"""
    x, y, z = (float(v) for v in np.asarray(p, float) - kin.hip[leg])
    l1, l2, l3 = (abs(float(v)) for v in kin.links[leg])
    d = knee_cosine(leg, p, kin)
    out = not (-1.0 <= d <= 1.0)
    if d > 1.0:
        d = 1.0
    rt = _sqrt(max(y * y + z * z - l1 * l1, 0.0))
    q = np.zeros(3)
    if kin.links[leg][0] < 0.0:
        q[0] = math.atan2(z, y) + math.atan2(rt, -l1)
    else:
        q[0] = -(math.atan2(z, -y) + math.atan2(rt, -l1))
    q[2] = math.atan2(-_sqrt(1.0 - d * d), d) if not math.isnan(d) else float("nan")
    if math.isnan(q[2]):
        q[1] = float("nan")
    else:
        q[1] = -math.atan2(x, rt) - math.atan2(l3 * math.sin(q[2]), l2 + l3 * math.cos(q[2]))
    return q, out


def wrap_pi(r):
    if not math.isfinite(r):
        return float("nan")
    s = r + PI
    s -= math.floor(s / (2.0 * PI)) * (2.0 * PI)
    if s < 0.0:
        s += 2.0 * PI
    return s - PI


# ------------------------------------------------------------------ the step, numpy
def leg_plant_step_np(mass, Ib, Rwb, x, xdot, w, joint_q, joint_qdot, joint_tau, mask, leg_inertia, dt, kin=DEFAULT_KIN):
    """One step for n robots; mask [n, 4] bool (contact_mask).  Returns a dict of NEW arrays Rwb, x, xdot, w, joint_q,
    joint_qdot, foot_world [n, 12], flags [n] int32 and the recovered forces g [n, 12] (0 for swing legs)."""
    n = x.shape[0]
    R = np.asarray(Rwb, np.float64).reshape(n, 3, 3)
    q, qd, tq = (np.array(a, np.float64).reshape(n, 4, 3) for a in (joint_q, joint_qdot, joint_tau))
    inertia = np.broadcast_to(np.asarray(leg_inertia, np.float64), (3,))
    g = np.zeros((n, 4, 3))
    c = np.zeros((n, 4, 3))
    flags = np.zeros(n, np.int32)
    qn, qdn = q.copy(), qd.copy()
    for i in range(n):
        for l in range(4):
            c[i, l] = x[i] + R[i] @ fk(l, q[i, l], kin)
            if mask[i, l]:
                g[i, l], singular = force_from_torque(l, q[i, l], tq[i, l], kin)
                flags[i] |= int(singular) << l
            else:
                qdn[i, l] = qd[i, l] + dt * (tq[i, l] / inertia)
                qn[i, l] = q[i, l] + dt * qdn[i, l]
    body = PR.plant_step_np(mass, Ib, Rwb, x, xdot, w, g.reshape(n, 12), c.reshape(n, 12), dt)
    R1 = body["Rwb"].reshape(n, 3, 3)
    for i in range(n):
        for l in range(4):
            if mask[i, l]:
                qn[i, l], out = ik(l, R1[i].T @ (c[i, l] - body["x"][i]), kin)
                flags[i] |= int(out) << (4 + l)
                qdn[i, l] = [wrap_pi(qn[i, l, k] - q[i, l, k]) / dt for k in range(3)]
    cc = np.ascontiguousarray
    return dict(Rwb=body["Rwb"], x=body["x"], xdot=body["xdot"], w=body["w"], joint_q=cc(qn.reshape(n, 12)), joint_qdot=cc(qdn.reshape(n, 12)),
                foot_world=cc(c.reshape(n, 12)), flags=flags, g=cc(g.reshape(n, 12)))


# ------------------------------------------------------------------ the step, 50 digits with bars
def _ik_mp(leg, p, kin=DEFAULT_KIN):
    """legInverseKinematics on 50-digit inputs, d taken as is (the pool keeps |d| <= 0.9: no clamp, no NaN)"""
    hx, hy, hz = (mpf(v) for v in kin.hip[leg])
    l1, l2, l3 = (abs(mpf(v)) for v in kin.links[leg])
    x, y, z = p[0] - hx, p[1] - hy, p[2] - hz
    d = (x * x + y * y + z * z - l1 * l1 - l2 * l2 - l3 * l3) / (2 * l2 * l3)
    assert -1 < d < 1, "the 50-digit IK is written for a bent leg in reach"
    sc = y * y + z * z - l1 * l1
    rt = mp.sqrt(sc) if sc > 0 else mp.mpf(0)
    if kin.links[leg][0] < 0.0:
        q1 = mp.atan2(z, y) + mp.atan2(rt, -l1)
    else:
        q1 = -(mp.atan2(z, -y) + mp.atan2(rt, -l1))
    q3 = mp.atan2(-mp.sqrt(1 - d * d), d)
    q2 = -mp.atan2(x, rt) - mp.atan2(l3 * mp.sin(q3), l2 + l3 * mp.cos(q3))
    return [q1, q2, q3], d


def _wrap_pi_mp(r):
    two_pi = 2 * mp.pi
    return r - mp.floor((r + mp.pi) / two_pi) * two_pi


def leg_plant_step_mp(mass, Ib, Rwb, x, xdot, w, joint_q, joint_qdot, joint_tau, mask, leg_inertia, dt, g=G, kin=DEFAULT_KIN):
    """One robot at 50 digits.  Returns {name: (value, bar)} for Rwb [9], x, xdot, w [3], foot_world, joint_q, joint_qdot [12].
    The bar of a stance leg's joint_q / joint_qdot entries is NaN here: stance_ik_bars measures it over the pool.  Also
    "knee" [4]: the 50-digit knee cosine d of the stance legs' IK (NaN for swing legs) and "det" [4]: det J of the stance legs."""
    Ibm = np.asarray(Ib, float).reshape(3, 3)
    assert np.count_nonzero(Ibm - np.diag(np.diagonal(Ibm))) == 0, "the roundings of Ib^-1 are counted for a diagonal Ib"
    inertia = np.broadcast_to(np.asarray(leg_inertia, float), (3,))
    with mp.workdps(DPS):
        def T(v):
            return Er(mpf(v))

        R = [T(v) for v in np.asarray(Rwb, float).reshape(9)]
        X, V, W = ([T(v) for v in np.asarray(a, float).reshape(3)] for a in (x, xdot, w))
        Q, QD, TQ = ([T(v) for v in np.asarray(a, float).reshape(12)] for a in (joint_q, joint_qdot, joint_tau))
        IB = [T(v) for v in Ibm.reshape(9)]
        inv = mp.inverse(mp.matrix([[mpf(v) for v in row] for row in Ibm]))
        IBI = [Er(inv[i, j], None, PR.IB_INV_ROUNDINGS * float(abs(inv[i, j]))) for i in range(3) for j in range(3)]
        m, dtm, gm = T(mass), T(dt), T(g)
        INER = [T(v) for v in inertia]

        fs, tau = [Er(mp.mpf(0))] * 3, [Er(mp.mpf(0))] * 3
        C, QN, QDN, det = [], list(Q), list(QD), [float("nan")] * 4
        for leg in range(4):
            q = Q[3 * leg:3 * leg + 3]
            sn = [Er(mp.sin(a.v), 1.0, SINCOS_EPS) for a in q]
            cs = [Er(mp.cos(a.v), 1.0, SINCOS_EPS) for a in q]
            s1, c1, s2, c2 = sn[0], cs[0], sn[1], cs[1]
            s23, c23 = s2 * cs[2] + c2 * sn[2], c2 * cs[2] - s2 * sn[2]
            l1, l2, l3 = (T(v) for v in kin.links[leg])
            hip = [T(v) for v in kin.hip[leg]]
            p = [l2 * s2 + l3 * s23 + hip[0], l1 * c1 - l2 * s1 * c2 - l3 * s1 * c23 + hip[1], l1 * s1 + l2 * c1 * c2 + l3 * c1 * c23 + hip[2]]
            r = PR._mat_vec(R, p)
            C += [X[k] + r[k] for k in range(3)]
            if mask[leg]:
                a, b = l2 * c2 + l3 * c23, l2 * s2 + l3 * s23
                zero = Er(mp.mpf(0))
                J = [zero, a, l3 * c23, -(l1 * s1) - a * c1, b * s1, l3 * s1 * s23, l1 * c1 - a * s1, -(b * c1), -(l3 * s23 * c1)]
                cof = [J[4] * J[8] - J[5] * J[7], J[5] * J[6] - J[3] * J[8], J[3] * J[7] - J[4] * J[6],
                       J[2] * J[7] - J[1] * J[8], J[0] * J[8] - J[2] * J[6], J[1] * J[6] - J[0] * J[7],
                       J[1] * J[5] - J[2] * J[4], J[2] * J[3] - J[0] * J[5], J[0] * J[4] - J[1] * J[3]]
                dj = J[1] * cof[1] + J[2] * cof[2]  # (J[0] = 0 exactly)
                det[leg] = float(dj.v)
                assert kin.det_lo(leg) <= abs(det[leg]) <= DET_HI, "the 50-digit step is written for the closed-form band"
                t = TQ[3 * leg:3 * leg + 3]
                gl = [(cof[3 * r_] * t[0] + cof[3 * r_ + 1] * t[1] + cof[3 * r_ + 2] * t[2]) / dj for r_ in range(3)]
                f = [-v for v in PR._mat_vec(R, gl)]
                mom = _cross(r, f)
                fs = [fs[k] + f[k] for k in range(3)]
                tau = [tau[k] + mom[k] for k in range(3)]
            else:
                for k in range(3):
                    QDN[3 * leg + k] = QD[3 * leg + k] + dtm * (TQ[3 * leg + k] / INER[k])
                    QN[3 * leg + k] = Q[3 * leg + k] + dtm * QDN[3 * leg + k]
        # the body: the chain of plant_restatement.plant_step_mp from fs, tau on
        Iw_w = PR._mat_vec(R, PR._mat_vec(IB, PR._mat_t_vec(R, W)))
        gyro = _cross(W, Iw_w)
        net = [tau[k] - gyro[k] for k in range(3)]
        wdot = PR._mat_vec(R, PR._mat_vec(IBI, PR._mat_t_vec(R, net)))
        acc = [fs[0] / m, fs[1] / m, fs[2] / m - gm]
        V1 = [V[k] + dtm * acc[k] for k in range(3)]
        X1 = [X[k] + dtm * V1[k] for k in range(3)]
        W1 = [W[k] + dtm * wdot[k] for k in range(3)]
        phi = [dtm * W1[k] for k in range(3)]
        sq = [p_ * p_ for p_ in phi]
        th = er_sqrt(sq[0] + sq[1] + sq[2])
        one = Er(mp.mpf(1))
        if th.v > 0:
            sc, ch = er_sinc_cos(th.half())
            A, B = sc * ch, (sc * sc).half()
        else:
            A, B = one, one.half()
        E = [one - B * (sq[1] + sq[2]), B * (phi[0] * phi[1]) - A * phi[2], B * (phi[0] * phi[2]) + A * phi[1],
             B * (phi[0] * phi[1]) + A * phi[2], one - B * (sq[0] + sq[2]), B * (phi[1] * phi[2]) - A * phi[0],
             B * (phi[0] * phi[2]) - A * phi[1], B * (phi[1] * phi[2]) + A * phi[0], one - B * (sq[0] + sq[1])]
        R1 = [E[3 * r_] * R[c_] + E[3 * r_ + 1] * R[3 + c_] + E[3 * r_ + 2] * R[6 + c_] for r_ in range(3) for c_ in range(3)]
        knee = [float("nan")] * 4
        nan_bar = set()
        for leg in range(4):
            if mask[leg]:
                pb = PR._mat_t_vec(R1, [C[3 * leg + k] - X1[k] for k in range(3)])
                qn, d = _ik_mp(leg, [v.v for v in pb], kin)
                knee[leg] = float(d)
                for k in range(3):
                    QN[3 * leg + k] = Er(qn[k])
                    QDN[3 * leg + k] = Er(_wrap_pi_mp(qn[k] - Q[3 * leg + k].v) / dtm.v)
                    nan_bar.add(3 * leg + k)
        out = dict(Rwb=PR._unpack(R1), x=PR._unpack(X1), xdot=PR._unpack(V1), w=PR._unpack(W1), foot_world=PR._unpack(C),
                   joint_q=PR._unpack(QN), joint_qdot=PR._unpack(QDN))
        for name in ("joint_q", "joint_qdot"):
            for k in nan_bar:
                out[name][1][k] = np.nan
        out["knee"], out["det"] = np.array(knee), np.array(det)
        return out


def stance_ik_bars(np_out, mp_val, mask):
    """The measured bars of a stance leg's joint_q and joint_qdot (module docstring): IK_BAR_MARGIN times the largest deviation of
    the numpy step from the 50-digit values over the pool's stance legs.  np_out: leg_plant_step_np's dict; mp_val: {name: values
    [n, 12]}; mask [n, 4]."""
    sel = np.repeat(np.asarray(mask, bool), 3, axis=1)
    return {k: IK_BAR_MARGIN * float(np.abs(np_out[k] - mp_val[k])[sel].max()) for k in ("joint_q", "joint_qdot")}


# ------------------------------------------------------------------ pools
STAND_Q = np.array([0.0, 0.8, -1.6])  # a bent leg on the IK branch (q3 <= 0), knee cosine d = cos q3 ~ -0.03, foot ~0.31 m under the hip


def bent_legs(rng, n):
    """[n, 12] joint angles on the reference IK's branch with the knee cosine d = cos q3 in [-0.85, 0.85] (the pools' margin to
    the reach limits) and the foot well under the trunk: |q1| <= 0.3, q3 in -[acos(0.85), acos(-0.85)], q2 = -q3 / 2 + [-0.3, 0.3]."""
    q = np.zeros((n, 4, 3))
    q[:, :, 0] = rng.uniform(-0.3, 0.3, (n, 4))
    q[:, :, 2] = -rng.uniform(math.acos(0.85), math.acos(-0.85), (n, 4))
    q[:, :, 1] = -q[:, :, 2] / 2 + rng.uniform(-0.3, 0.3, (n, 4))
    return q.reshape(n, 12)


def pool_margins(q, mask, kin=DEFAULT_KIN):
    """(max |d|, min |det J| / the leg's DET_LO) over the stance legs of joint angles q [n, 12]: the two margins of the pools"""
    q = np.asarray(q).reshape(-1, 4, 3)
    dmax, detmin = 0.0, np.inf
    for i in range(q.shape[0]):
        for l in range(4):
            if mask[i, l]:
                dmax = max(dmax, abs(knee_cosine(l, fk(l, q[i, l], kin), kin)))
                detmin = min(detmin, abs(det3(jacobian(l, q[i, l], kin))) / kin.det_lo(l))
    return dmax, detmin


def make_pool(n, seed, kin=DEFAULT_KIN):
    """n robots for the one-step tests: tilted up to 0.4 rad about a random axis on top of any yaw, near the stand height, moving
    and turning at a few dm/s and rad/s (every fourth one with w = 0 exactly); bent legs (bent_legs) with joint velocities up to
    2 rad/s; torques tau = J^T g of ground-reaction-sized forces g (|tau| < 20: inside the tick's clamp); uniformly random gait
    phases, so that the default duty 0.8 / 0.98 puts about one leg in five into swing."""
    from scipy.spatial.transform import Rotation

    rng = np.random.default_rng(seed)
    tilt = rng.normal(size=(n, 3))
    tilt *= (rng.uniform(0, 0.4, n) / np.linalg.norm(tilt, axis=1))[:, None]
    R = (Rotation.from_rotvec(tilt) * Rotation.from_euler("z", rng.uniform(-PI, PI, n))).as_matrix()
    q = bent_legs(rng, n)
    g = rng.uniform(-1, 1, (n, 4, 3)) * np.array([10.0, 10.0, 25.0]) - np.array([0.0, 0.0, 25.0])
    tau = np.array([[jacobian(l, q.reshape(n, 4, 3)[i, l], kin).T @ g[i, l] for l in range(4)] for i in range(n)])
    assert kin.tau_min < tau.min() and tau.max() < kin.tau_max  # (the default model's: |tau| < 20)
    w = rng.uniform(-2, 2, (n, 3))
    w[0::4] = 0.0
    c = np.ascontiguousarray
    return dict(Rwb=c(R.reshape(n, 9)), x=c(np.array([0.0, 0.0, 0.3]) + rng.uniform(-0.05, 0.05, (n, 3))), xdot=c(rng.uniform(-0.5, 0.5, (n, 3))), w=c(w),
                joint_q=c(q), joint_qdot=c(rng.uniform(-2, 2, (n, 12))), joint_tau=c(tau.reshape(n, 12)), gait_phase=c(rng.uniform(0, 1, (n, 4))))
