"""TEST INFRASTRUCTURE - numpy restatement of the device-side adjoint of the balance QP (csrc/qc_sensitivity.hpp,
qc_sensitivity_batch), and the same definitions for single robots at 50 digits.

Per robot the solve minimises (A f - b)^T S (A f - b) + f^T W f over the world-frame forces f; H = 2 (A^T S A + W).  The active
codes of the certificate (tests/kkt_certificate_restatement.foot_conditions) define the face f = Z y + f0:
  z code != 0: fz pinned; z code 0: fz free.  x (y) code 0: free; code 1 / 2: fx = -mu fz / +mu fz - a multiple of fz in the column
  of a free fz, pinned with a pinned fz.  Any code 3 on a stance foot: the whole foot pinned, bit 0 of flags.  Swing feet pinned.
With the cotangent grf_bar on grf_body (grf_body_i = -Rwb^T f_i, Rwb fixed):
  f_bar = -Rwb grf_bar,  z = Z (Z^T H Z)^-1 Z^T f_bar,  b_bar = 2 S A z,
  r_bar_i = -2 (z_i x v_ang + f_i x q_ang)  with v = S (A f - b), q = S A z,   feet_bar_i = Rwb^T r_bar_i,
and x_bar ... w_d_bar are b_bar pulled back through the PD law as tests/kkt_batch.wrench_data states it (Rwb, Rwb_d fixed):
  b_lin = m (kp_p (x_d - x) + kd_p (xdot_d - xdot) + (kff0 xdot_d0, kff1 xdot_d1, const) + g),
  b_ang = Iw al + w_d x (Iw w_d),  al = kp_w e + kd_w (w_d - w) + (kff3 w_d0, kff4 w_d1 + kff5 w_d2, 0),  Iw = Rwb Ib Rwb^T.

Here the reduced system is solved on the EXPLICIT variable-size Z (k = number of free coordinates, 0 ... 12), by numpy's
Cholesky; the device pads it to a fixed 12 x 12 with identity rows.  The two routes check each other.  A reduced matrix that is
not positive definite or not finite: every output NaN, bit 1 of flags.

sensitivity_mp() evaluates one robot at 50 digits (mpmath): b and r from device_math_reference.wrench_mp, the rest as above."""
from __future__ import annotations

import mpmath as mp
import numpy as np

from tests import device_math_reference as DMR
from tests import kkt_certificate_restatement as KR
from tests.kkt_certificate_restatement import distance, magnitude  # noqa: F401 - the one definition of each, under this module's name too
from tests.kkt_batch import wrench_data

OUTPUTS = ("adjoint", "b_bar", "feet_bar", "x_bar", "xdot_bar", "w_bar", "x_d_bar", "xdot_d_bar", "w_d_bar")


def face(active, mu):
    """Z [12, k] (float64: entries 0, 1, +-mu) and the one-sided flag of one robot's active codes [4]"""
    cols, flagged = [], False
    for l in range(4):
        code = int(active[l])
        if code & KR.SWING:
            continue
        cx, cy, cz = code & 3, (code >> 2) & 3, (code >> 4) & 3
        if 3 in (cx, cy, cz):
            flagged = True
            continue
        for axis, c in ((0, cx), (1, cy)):
            if c == 0:
                col = np.zeros(12)
                col[3 * l + axis] = 1.0
                cols.append(col)
        if cz == 0:
            col = np.zeros(12)
            col[3 * l + 2] = 1.0
            for axis, c in ((0, cx), (1, cy)):
                if c:
                    col[3 * l + axis] = -mu if c == 1 else mu
            cols.append(col)
    return (np.stack(cols, axis=1) if cols else np.zeros((12, 0))), flagged


def _pullback(P, R, wd, bb):
    """(x_bar, xdot_bar, w_bar, x_d_bar, xdot_d_bar, w_d_bar) of b_bar [6] through the PD law, one robot (works on numpy arrays of
    floats and of mpmath numbers alike)"""
    m = P["mass"]
    kff = P["kff"]
    bl, ba = bb[:3], bb[3:]
    x_d_bar = m * P["kp_p"] * bl
    xdot_d_bar = m * P["kd_p"] * bl
    xdot_d_bar = xdot_d_bar + m * np.array([kff[0] * bl[0], kff[1] * bl[1], 0 * bl[2]])
    Iw = R @ P["Ib"] @ R.T
    alb = Iw.T @ ba
    w_bar = -P["kd_w"] * alb
    w_d_bar = P["kd_w"] * alb + np.array([kff[3] * alb[0], kff[4] * alb[1], kff[5] * alb[1]])
    w_d_bar = w_d_bar + _cross(Iw @ wd, ba) + Iw.T @ _cross(ba, wd)
    return dict(x_bar=-x_d_bar, xdot_bar=-(m * P["kd_p"] * bl), w_bar=w_bar, x_d_bar=x_d_bar, xdot_d_bar=xdot_d_bar, w_d_bar=w_d_bar)


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _params(P, conv=float):
    arr = lambda k, shape: np.array([conv(v) for v in np.asarray(P[k], np.float64).reshape(-1)], dtype=object if conv is not float else float).reshape(shape)
    return dict(mass=conv(P["mass"]), kff=arr("kff", (6,)), kp_p=arr("kp_p", (3,)), kd_p=arr("kd_p", (3,)), kd_w=arr("kd_w", (3,)), Ib=arr("Ib", (3, 3)),
                S=arr("S", (6, 6)), W=arr("W", (12, 12)))


def sensitivity(P, b, grf_body, grf_bar, act_tol=1e-7, default_duty=KR.DEFAULT_DUTY):
    """dict of every output of qc_sensitivity_batch ([n, ...] float64), flags [n] int32, plus r_bar [n,4,3] (world frame) and
    active [n,4] (the codes the face was read from)."""
    with np.errstate(invalid="ignore"):
        b = KR.with_feet(b)
        n = b["x"].shape[0]
        Pn = _params(P)
        S, Wm, mu = Pn["S"], Pn["W"], float(P["mu"])
        A, bv = wrench_data(P, b)
        active = KR.certificate(P, b, grf_body, act_tol, default_duty=default_duty)["active"]
        out = {k: np.zeros((n,) + s) for k, s in (("adjoint", (12,)), ("b_bar", (6,)), ("feet_bar", (4, 3)), ("r_bar", (4, 3)))}
        out.update({k: np.zeros((n, 3)) for k in OUTPUTS[3:]})
        flags = np.zeros(n, np.int32)
        for i in range(n):
            R = b["Rwb"][i].reshape(3, 3)
            f = -(np.asarray(grf_body[i]).reshape(4, 3) @ R.T).reshape(12)
            fbar = -(np.asarray(grf_bar[i]).reshape(4, 3) @ R.T).reshape(12)
            Z, flagged = face(active[i], mu)
            z = np.zeros(12)
            bad = False
            if Z.shape[1]:
                H = 2.0 * (A[i].T @ S @ A[i] + Wm)
                M = Z.T @ H @ Z
                try:
                    if not np.isfinite(M).all():
                        raise np.linalg.LinAlgError
                    L = np.linalg.cholesky(M)
                    y = np.linalg.solve(L.T, np.linalg.solve(L, Z.T @ fbar))
                    z = Z @ y
                except np.linalg.LinAlgError:
                    bad = True
            if bad:
                z = np.full(12, np.nan)
            flags[i] = (1 if flagged else 0) | (2 if bad else 0)
            qv = S @ (A[i] @ z)
            v = S @ (A[i] @ f - bv[i])
            bb = 2.0 * qv
            rbar = np.array([-2.0 * (_cross(z[3 * l:3 * l + 3], v[3:]) + _cross(f[3 * l:3 * l + 3], qv[3:])) for l in range(4)])
            out["adjoint"][i], out["b_bar"][i], out["r_bar"][i], out["feet_bar"][i] = z, bb, rbar, rbar @ R
            for k, val in _pullback(Pn, R, b["w_d"][i], bb).items():
                out[k][i] = val
        out["flags"], out["active"] = flags, active
        return out


def reduced_condition(P, b, active, i):
    """cond_2 of robot i's reduced matrix Z^T H Z (1.0 where nothing is free): the scale of a double solve's rounding error"""
    b = KR.with_feet(b)
    A, _ = wrench_data(P, {k: v[i:i + 1] for k, v in b.items() if v is not None})
    Z, _ = face(active[i], float(P["mu"]))
    if not Z.shape[1]:
        return 1.0
    H = 2.0 * (A[0].T @ np.asarray(P["S"], float).reshape(6, 6) @ A[0] + np.asarray(P["W"], float).reshape(12, 12))
    return float(np.linalg.cond(Z.T @ H @ Z))


# ------------------------------------------------------------------ 50 digits, one robot
def sensitivity_mp(P, b, grf_body, grf_bar, i, active, kin=None):
    """Robot i at 50 digits with the active codes `active` [4] (as sensitivity() classified them).  kin = (hip [12], links [12]):
    the feet come from joint_q.  Returns dict(name -> flat list of mpmath numbers) for OUTPUTS and r_bar."""
    with mp.workdps(DMR.DPS):
        lift = lambda v: DMR.mpf(float(v))
        state = {k: np.asarray(b[k][i], np.float64) for k, _ in DMR.WRENCH_S_KEYS}
        w = DMR.wrench_mp(P, state, b["joint_q"][i] if kin is not None else b["feet"][i], kin)
        bw = mp.matrix([x for x in np.asarray(w["b"][0], dtype=object).reshape(-1)])
        r = [x for x in np.asarray(w["r"][0], dtype=object).reshape(-1)]
        A = mp.zeros(6, 12)
        for l in range(4):
            x, y, z_ = r[3 * l:3 * l + 3]
            for k in range(3):
                A[k, 3 * l + k] = mp.mpf(1)
            A[3, 3 * l + 1], A[3, 3 * l + 2] = -z_, y
            A[4, 3 * l], A[4, 3 * l + 2] = z_, -x
            A[5, 3 * l], A[5, 3 * l + 1] = -y, x
        tomat = lambda a: mp.matrix([[lift(x) for x in row] for row in np.atleast_2d(np.asarray(a, np.float64))])
        S, Wm = tomat(np.asarray(P["S"], float).reshape(6, 6)), tomat(np.asarray(P["W"], float).reshape(12, 12))
        R = tomat(np.asarray(b["Rwb"][i], float).reshape(3, 3))
        world = lambda g: mp.matrix([-(R * mp.matrix([lift(x) for x in g[3 * l:3 * l + 3]]))[k] for l in range(4) for k in range(3)])
        f, fbar = world(np.asarray(grf_body[i], float).reshape(-1)), world(np.asarray(grf_bar[i], float).reshape(-1))
        Zn, _ = face(active, float(P["mu"]))
        z = mp.zeros(12, 1)
        if Zn.shape[1]:
            Z = tomat(Zn)
            H = 2 * (A.T * S * A + Wm)
            z = Z * mp.lu_solve(Z.T * H * Z, Z.T * fbar)
        qv = S * (A * z)
        v = S * (A * f - bw)
        bb = 2 * qv
        tl = lambda m_: [m_[r_, c_] for r_ in range(m_.rows) for c_ in range(m_.cols)]
        zl, fl, ql, vl = tl(z), tl(f), tl(qv), tl(v)
        rbar, fbar_body = [], []
        for l in range(4):
            c = [-2 * (a_ + b_) for a_, b_ in zip(_cross(zl[3 * l:3 * l + 3], vl[3:]), _cross(fl[3 * l:3 * l + 3], ql[3:]))]
            rbar += c
            fbar_body += tl(R.T * mp.matrix(c))
        Pm = _params(P, conv=lift)
        Rm = np.array(tl(R), dtype=object).reshape(3, 3)
        wd = np.array([lift(x) for x in b["w_d"][i]], dtype=object)
        pb = _pullback(Pm, Rm, wd, np.array(tl(bb), dtype=object))
        out = dict(adjoint=zl, b_bar=tl(bb), feet_bar=fbar_body, r_bar=rbar)
        out.update({k: list(val) for k, val in pb.items()})
        return out
