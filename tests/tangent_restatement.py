"""TEST INFRASTRUCTURE - numpy restatement of the forward mode of the balance QP (csrc/qc_tangent.hpp, qc_tangent_batch,
include/qc_tangent.h), float64.

Per robot and direction, with R = Rwb, f_i = -R grf_body_i, v = S (A f - b), delta / delta_d the world-frame left tangents of Rwb / Rwb_d:
  dp_i = feet_tan_i + J(q_i) joint_q_tan_i,   dr_i = delta x r_i + R dp_i,
  db   = the forward derivative of the PD law as tests/kkt_batch.wrench_data states it (its kff lines included; dIw = [delta]x Iw -
         Iw [delta]x; e = log(Rd R^T) along dRe = [delta_d]x Re - Re [delta]x, through sensitivity_rotation_restatement.log_jacobian -
         the Jacobian of the Eigen-convention log on the branch taken, written there in forward mode),
  dg   = 2 (dA^T v + A^T S (dA f - db)),   df = -Z (Z^T H Z)^-1 Z^T dg,   grf_tan_i = -R^T df_i + R^T (delta x f_i),   b_tan = db.
Here dA is the explicit 6 x 12 matrix of the dr_i and the reduced system is solved on the EXPLICIT variable-size Z by numpy's Cholesky
(sensitivity_restatement.face); the device pads it to 12 x 12 and never forms dA.  A reduced matrix that is not positive definite or
not finite: every output of the robot NaN in all directions, bit 1 of flags.

tangent() also returns the CONDITION SUMS the rounding of its outputs is measured against, entry by entry: every term of the
expression with the absolute values of all its factors - |db| from the PD law's lines, |dg| = 2 (|dA|^T |v| + |A|^T |S| (|dA| |f| +
|db|)), and through the solve |Z| |M^-1| (|Z|^T |dg| + |M| |y|) with M = Z^T H Z and |M| = |Z|^T 2 (|A|^T |S| |A| + |W|) |Z|, the
componentwise first-order bound for a rounded right-hand side AND a rounded matrix, which carries the reduced system's conditioning -
then |R|^T (that + |delta| x |f|) for grf_tan.

tangent_mp() evaluates one robot and one direction at 50 digits (mpmath) on the exact doubles: b and r from
device_math_reference.wrench_mp, the log's Jacobian from sensitivity_rotation_restatement.log_jacobian_mp (central differences of the
50-digit log on the branch held - nothing of the float64 Jacobian), the reduced system by mpmath's LU.  C_TAN below is the float64
restatement's measured distance from it in EPS x condition sum."""
from __future__ import annotations

import mpmath as mp
import numpy as np

from tests import device_math_reference as DMR

from tests import kkt_certificate_restatement as KR
from tests import sensitivity_restatement as SR
from tests import sensitivity_rotation_restatement as RR
from tests.kkt_batch import wrench_data
from tests.leg_plant_restatement import jacobian as leg_jacobian

TANGENTS = {"x_tan": 3, "xdot_tan": 3, "w_tan": 3, "x_d_tan": 3, "xdot_d_tan": 3, "w_d_tan": 3, "Rwb_rot_tan": 3, "Rwb_d_rot_tan": 3,
            "feet_tan": 12, "joint_q_tan": 12}


EPS = 2.0 ** -52
# The measured constant of the dot-product identity in float64 numpy, the worst over tests/test_tangent_cpu.py's draws rounded up: 1.24 with every
# input at once (test_dot_product_identity_in_numpy), 0.56 ... 1.36 one input at a time (test_each_input_alone_in_numpy: w_tan 1.36,
# w_d_tan 1.34, Rwb_rot_tan 1.05); the device's bar is 4 x it (tests/test_gpu_tangent.py), the convention of every neighbour.
C_DOT = 1.4
# The same two measures at solved_batch_support.odd_law on odd_states (tests/test_odd_law_cpu.py::test_dot_product_identity_at_the_odd_law:
# 0.94 with every input at once; alone 0.61 ... 1.39: w_d_tan 1.39, Rwb_d_rot_tan 1.27, Rwb_rot_tan 1.11), rounded up;
# tests/test_gpu_odd_law.py's bar is 4 x it.
C_DOT_ODD = 1.4
# The float64 restatement's worst |value - 50-digit value| / (EPS x condition sum) over grf_tan and b_tan ON EVERY EIGHTH ROBOT (0, 8,
# ... 128) of the 130-robot placed-force batch, from `feet` (every tangent but joint_q_tan) and from joint_q (every tangent), two
# directions each (tests/test_tangent_cpu.py::test_restatement_against_50_digits prints it: grf_tan 0.52 from `feet`, 0.66 from
# joint_q; b_tan 1.06), rounded up; the device's bar is 4 x it.  A SAMPLE's worst, not the restatement's: see C_TAN_ALL.
C_TAN = 1.1
# The same measure over ALL 130 robots (tests/test_odd_law_cpu.py::test_tangent_restatement_against_50_digits_on_every_robot: b_tan
# 3.06, grf_tan 0.66 from `feet` and 0.77 from joint_q), rounded up.  No device bar is stated in it: 4 x C_TAN = 4.4 still holds it.
C_TAN_ALL = 3.1
# ... and at solved_batch_support.odd_law on odd_states, with the sums of log_formation=True (the log's Jacobian enters with the
# magnitude sum of its own formation): all 130 robots, every input at once, one direction
# (tests/test_odd_law_cpu.py::test_tangent_restatement_against_50_digits_at_the_odd_law: b_tan 1.14, grf_tan 0.80 from `feet` and 0.92
# from joint_q), AND one input alone with unit-axis seeds, where a line's rounding has only its own terms to be measured against
# (::test_tangent_restatement_against_50_digits_one_input_alone: b_tan 1.81 Rwb_d_rot_tan, 1.53 Rwb_rot_tan, 1.44 w_d_tan), rounded
# up; tests/test_gpu_odd_law.py's bar is 4 x it.
C_TAN_ODD = 1.9


def dot_gap(gbar, grf_tan, sens, rot, tans, k, cond):
    """(|<v, J u> - <J^T v, u>| in units of EPS x (the magnitudes of all terms on both sides) x the reduced condition number, <v, J u>)
    per robot, for direction k"""
    n = gbar.shape[0]
    prod = gbar * grf_tan[k].reshape(n, 12)
    rhs, rmag = pairing(sens, rot, tans, k)
    lhs, lmag = prod.sum(axis=1), np.abs(prod).sum(axis=1)
    return np.abs(lhs - rhs) / (EPS * np.maximum(lmag + rmag, 1e-300) * cond), lhs


def hat(d):
    return np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])


def random_tangents(n, K, seed, joint_q=False, names=None):
    """{name: [K, n, m]} standard-normal tangents (feet at 0.1 m, joint angles at 0.1 rad: the sizes a linearisation is used at)"""
    rng = np.random.default_rng(seed)
    out = {}
    for k, m in TANGENTS.items():
        if (k == "joint_q_tan" and not joint_q) or (names is not None and k not in names):
            continue
        out[k] = rng.normal(0.0, 0.1 if m == 12 else 1.0, (K, n, m))
    return out


def wrench_tangent(P, R, Rd, w, wd, t):
    """db [6] of one robot and one direction; t: name -> vector (missing: zero)"""
    z3 = np.zeros(3)
    g = lambda k: np.asarray(t.get(k, z3), float).reshape(-1)
    m, kff = float(P["mass"]), np.asarray(P["kff"], float)
    kp_p, kd_p, kp_w, kd_w = (np.asarray(P[k], float) for k in ("kp_p", "kd_p", "kp_w", "kd_w"))
    Ib = np.asarray(P["Ib"], float).reshape(3, 3)
    dvd, dwd, dl, dld = g("xdot_d_tan"), g("w_d_tan"), g("Rwb_rot_tan"), g("Rwb_d_rot_tan")
    da = kp_p * (g("x_d_tan") - g("x_tan")) + kd_p * (dvd - g("xdot_tan")) + np.array([kff[0] * dvd[0], kff[1] * dvd[1], 0.0])
    Re = Rd @ R.T
    e, J, _, _ = RR.log_jacobian(Re)
    dRe = hat(dld) @ Re - Re @ hat(dl)
    de = J @ dRe.reshape(9)
    al = kp_w * e + kd_w * (wd - w) + np.array([kff[3] * wd[0], kff[4] * wd[1] + kff[5] * wd[2], 0.0])
    dal = kp_w * de + kd_w * (dwd - g("w_tan")) + np.array([kff[3] * dwd[0], kff[4] * dwd[1] + kff[5] * dwd[2], 0.0])
    Iw = R @ Ib @ R.T
    dIw = hat(dl) @ Iw - Iw @ hat(dl)
    dba = dIw @ al + Iw @ dal + np.cross(dwd, Iw @ wd) + np.cross(wd, dIw @ wd + Iw @ dwd)
    return np.concatenate([m * da, dba])


def _across(a, b):
    """|a| x |b| with every product positive"""
    a, b = np.abs(a), np.abs(b)
    return np.array([a[1] * b[2] + a[2] * b[1], a[2] * b[0] + a[0] * b[2], a[0] * b[1] + a[1] * b[0]])


def wrench_tangent_sums(P, R, Rd, w, wd, t, log_formation=False):
    """the condition sums of wrench_tangent's db [6]: the same lines with the absolute values of all factors.  log_formation: the
    log's Jacobian enters with the magnitude sum of its own formation (sensitivity_rotation_restatement.log_jacobian_sum), not as an
    exact |J| - what a tangent along one axis needs; off by default, so that the sums of the cheetah-law tests stay what they were."""
    z3 = np.zeros(3)
    g = lambda k: np.abs(np.asarray(t.get(k, z3), float).reshape(-1))
    m, kff = abs(float(P["mass"])), np.abs(np.asarray(P["kff"], float))
    kp_p, kd_p, kp_w, kd_w = (np.abs(np.asarray(P[k], float)) for k in ("kp_p", "kd_p", "kp_w", "kd_w"))
    aR, aRd, aIb = np.abs(R), np.abs(Rd), np.abs(np.asarray(P["Ib"], float).reshape(3, 3))
    dvd, dwd, dl, dld = g("xdot_d_tan"), g("w_d_tan"), g("Rwb_rot_tan"), g("Rwb_d_rot_tan")
    da = kp_p * (g("x_d_tan") + g("x_tan")) + kd_p * (dvd + g("xdot_tan")) + np.array([kff[0] * dvd[0], kff[1] * dvd[1], 0.0])
    e, J, _, _ = RR.log_jacobian(Rd @ R.T)
    aRe = aRd @ aR.T
    ah = lambda d: np.abs(hat(d))
    aJ = RR.log_jacobian_sum(Rd @ R.T) if log_formation else np.abs(J)
    de = aJ @ (ah(dld) @ aRe + aRe @ ah(dl)).reshape(9)
    wd, w = np.abs(wd), np.abs(w)
    al = kp_w * np.abs(e) + kd_w * (wd + w) + np.array([kff[3] * wd[0], kff[4] * wd[1] + kff[5] * wd[2], 0.0])
    dal = kp_w * de + kd_w * (dwd + g("w_tan")) + np.array([kff[3] * dwd[0], kff[4] * dwd[1] + kff[5] * dwd[2], 0.0])
    Iw = aR @ aIb @ aR.T
    dIw = ah(dl) @ Iw + Iw @ ah(dl)
    dba = dIw @ al + Iw @ dal + _across(dwd, Iw @ wd) + _across(wd, dIw @ wd + Iw @ dwd)
    return np.concatenate([m * da, dba])


def tangent(P, b, grf_body, tans, act_tol=1e-7, kin=None, default_duty=KR.DEFAULT_DUTY, log_formation=False):
    """dict(grf_tan [K,n,4,3], b_tan [K,n,6], flags [n], active [n,4], grf_sum [K,n,4,3] and b_sum [K,n,6]: the condition sums of the
    two outputs (module docstring), cond [n]: the reduced condition number).  kin: the kinematic model (device_math_reference.Kin) of
    a batch with joint_q.  log_formation: see wrench_tangent_sums (it changes the sums only)."""
    with np.errstate(invalid="ignore"):
        has_q = b.get("feet") is None and b.get("joint_q") is not None
        q = np.asarray(b["joint_q"], float).reshape(-1, 4, 3) if has_q else None
        b = KR.with_feet(b, kin)
        n = b["x"].shape[0]
        K = next(iter(tans.values())).shape[0]
        S, Wm, mu = np.asarray(P["S"], float).reshape(6, 6), np.asarray(P["W"], float).reshape(12, 12), float(P["mu"])
        A, bv = wrench_data(P, b)
        active = KR.certificate(P, b, grf_body, act_tol, default_duty=default_duty)["active"]
        out = dict(grf_tan=np.zeros((K, n, 4, 3)), b_tan=np.zeros((K, n, 6)), flags=np.zeros(n, np.int32), active=active, grf_sum=np.zeros((K, n, 4, 3)),
                   b_sum=np.zeros((K, n, 6)), cond=np.ones(n))
        for i in range(n):
            R, Rd = b["Rwb"][i].reshape(3, 3), b["Rwb_d"][i].reshape(3, 3)
            p = b["feet"][i].reshape(4, 3)
            r = p @ R.T
            f = -(np.asarray(grf_body[i]).reshape(4, 3) @ R.T)
            v = S @ (A[i] @ f.reshape(12) - bv[i])
            Z, flagged = SR.face(active[i], mu)
            L, bad = None, False
            if Z.shape[1]:
                M = Z.T @ (2.0 * (A[i].T @ S @ A[i] + Wm)) @ Z
                try:
                    if not np.isfinite(M).all():
                        raise np.linalg.LinAlgError
                    L = np.linalg.cholesky(M)
                    Minv = np.abs(np.linalg.inv(M))
                    out["cond"][i] = np.linalg.cond(M)
                except np.linalg.LinAlgError:
                    bad = True
            out["flags"][i] = (1 if flagged else 0) | (2 if bad else 0)
            for k in range(K):
                t = {name: arr[k, i] for name, arr in tans.items()}
                db = wrench_tangent(P, R, Rd, b["w"][i], b["w_d"][i], t)
                dl = np.asarray(t.get("Rwb_rot_tan", np.zeros(3)), float)
                dp = np.asarray(t.get("feet_tan", np.zeros(12)), float).reshape(4, 3).copy()
                adp = np.abs(dp)
                if "joint_q_tan" in t:
                    dq = np.asarray(t["joint_q_tan"], float).reshape(4, 3)
                    for l in range(4):
                        Jl = leg_jacobian(l, q[i, l], *(() if kin is None else (kin,)))
                        dp[l] += Jl @ dq[l]
                        adp[l] += np.abs(Jl) @ np.abs(dq[l])
                dr = np.cross(dl, r) + dp @ R.T
                dA = np.zeros((6, 12))
                for l in range(4):
                    dA[3:, 3 * l:3 * l + 3] = hat(dr[l])
                dg = 2.0 * (dA.T @ v + A[i].T @ (S @ (dA @ f.reshape(12) - db)))
                zy = np.zeros(12)
                if bad:
                    zy = np.full(12, np.nan)
                elif L is not None:
                    y = np.linalg.solve(L.T, np.linalg.solve(L, Z.T @ dg))
                    zy = Z @ y
                cf = np.cross(dl, f)
                # the condition sums
                adb = wrench_tangent_sums(P, R, Rd, b["w"][i], b["w_d"][i], t, log_formation)
                adr = np.array([_across(dl, r[l]) for l in range(4)]) + adp @ np.abs(R).T
                adA = np.zeros((6, 12))
                for l in range(4):
                    adA[3:, 3 * l:3 * l + 3] = np.abs(hat(adr[l]))
                adg = 2.0 * (adA.T @ np.abs(v) + np.abs(A[i]).T @ (np.abs(S) @ (adA @ np.abs(f).reshape(12) + adb)))
                if L is not None:  # the right-hand side's terms and the reduced matrix's own: |M^-1| (|Z|^T |dg| + |M| |y|)
                    aM = np.abs(Z).T @ (2.0 * (np.abs(A[i]).T @ np.abs(S) @ np.abs(A[i]) + np.abs(Wm))) @ np.abs(Z)
                    azy = np.abs(Z) @ (Minv @ (np.abs(Z).T @ adg + aM @ np.abs(y)))
                else:
                    azy = np.zeros(12)
                acf = np.array([_across(dl, f[l]) for l in range(4)])
                out["grf_sum"][k, i] = (azy.reshape(4, 3) + acf) @ np.abs(R)
                out["b_sum"][k, i] = adb
                out["grf_tan"][k, i] = (zy.reshape(4, 3) + cf) @ R  # R^T (Z y + delta x f), row by row
                out["b_tan"][k, i] = db + (np.nan if bad else 0.0)
        return out


def pairing(sens, rot, tans, k):
    """sum over the inputs of <theta_bar, theta_tan> for direction k, per robot [n], and the sum of the magnitudes of its terms:
    sens / rot are the outputs of sensitivity_restatement.sensitivity / sensitivity_rotation_restatement.rotation_cotangents (or the
    device's, as numpy arrays)"""
    names = (("x_tan", sens, "x_bar"), ("xdot_tan", sens, "xdot_bar"), ("w_tan", sens, "w_bar"), ("x_d_tan", sens, "x_d_bar"),
             ("xdot_d_tan", sens, "xdot_d_bar"), ("w_d_tan", sens, "w_d_bar"), ("feet_tan", sens, "feet_bar"),
             ("Rwb_rot_tan", rot, "Rwb_rot_bar"), ("Rwb_d_rot_tan", rot, "Rwb_d_rot_bar"))
    n = sens["x_bar"].shape[0]
    total, mag = np.zeros(n), np.zeros(n)
    for tan, src, bar in names:
        if tan in tans:
            prod = np.asarray(src[bar]).reshape(n, -1) * tans[tan][k].reshape(n, -1)
            total += prod.sum(axis=1)
            mag += np.abs(prod).sum(axis=1)
    return total, mag


# ------------------------------------------------------------------ 50 digits, one robot and one direction
def tangent_mp(P, b, grf_body, tans, i, k, active, kin=None, memo=None):
    """Robot i, direction k at 50 digits on the exact doubles, with the active codes `active` [4] (as tangent() classified them).
    kin: the kinematic model (device_math_reference.Kin) of a batch whose feet come from joint_q.  Returns dict(grf_tan: 12 mpmath
    numbers, b_tan: 6).  memo: a dict of the caller's that keeps what does not depend on the direction - robot i's 50-digit wrench and
    the log with its Jacobian, two thirds of a pass - for further directions of the SAME P, b and kin."""
    with mp.workdps(DMR.DPS):
        lift = lambda v: DMR.mpf(float(v))
        mat = lambda a, shape: mp.matrix([[lift(x) for x in row] for row in np.asarray(a, np.float64).reshape(shape)])
        vec = lambda a: mp.matrix([lift(x) for x in np.asarray(a, np.float64).reshape(-1)])
        tv = lambda name, m: vec(tans[name][k, i]) if name in tans else mp.zeros(m, 1)
        cr = lambda a_, b_: mp.matrix([a_[1] * b_[2] - a_[2] * b_[1], a_[2] * b_[0] - a_[0] * b_[2], a_[0] * b_[1] - a_[1] * b_[0]])
        hatm = lambda d: mp.matrix([[0, -d[2], d[1]], [d[2], 0, -d[0]], [-d[1], d[0], 0]])
        had = lambda a_, b_: mp.matrix([a_[j] * b_[j] for j in range(3)])
        from_q = b.get("feet") is None
        state = {key: np.asarray(b[key][i], np.float64) for key, _ in DMR.WRENCH_S_KEYS}
        kin2 = None if not from_q else ((DMR.DEFAULT_KIN if kin is None else kin).hip.reshape(-1), (DMR.DEFAULT_KIN if kin is None else kin).links.reshape(-1))
        w = memo.get(("wrench", i)) if memo is not None else None
        if w is None:
            w = DMR.wrench_mp(P, state, b["joint_q"][i] if from_q else b["feet"][i], kin2)
            if memo is not None:
                memo["wrench", i] = w
        bw = mp.matrix([x for x in np.asarray(w["b"][0], dtype=object).reshape(-1)])
        r = [x for x in np.asarray(w["r"][0], dtype=object).reshape(-1)]
        R, Rd, Ib = mat(b["Rwb"][i], (3, 3)), mat(b["Rwb_d"][i], (3, 3)), mat(P["Ib"], (3, 3))
        S, Wm = mat(P["S"], (6, 6)), mat(P["W"], (12, 12))
        kff, kp_p, kd_p, kp_w, kd_w = (vec(P[key]) for key in ("kff", "kp_p", "kd_p", "kp_w", "kd_w"))
        m = lift(P["mass"])
        wv, wd = vec(b["w"][i]), vec(b["w_d"][i])
        A = mp.zeros(6, 12)
        for l in range(4):
            A[0, 3 * l] = A[1, 3 * l + 1] = A[2, 3 * l + 2] = mp.mpf(1)
            A[3:6, 3 * l:3 * l + 3] = hatm(r[3 * l:3 * l + 3])
        f = mp.matrix([-(R * vec(np.asarray(grf_body[i], float).reshape(4, 3)[l]))[c] for l in range(4) for c in range(3)])
        v = S * (A * f - bw)
        # db
        dvd, dwd, dl, dld = tv("xdot_d_tan", 3), tv("w_d_tan", 3), tv("Rwb_rot_tan", 3), tv("Rwb_d_rot_tan", 3)
        da = had(kp_p, tv("x_d_tan", 3) - tv("x_tan", 3)) + had(kd_p, dvd - tv("xdot_tan", 3)) + mp.matrix([kff[0] * dvd[0], kff[1] * dvd[1], 0])
        Re = Rd * R.T
        logs = memo.get(("log", i)) if memo is not None else None
        if logs is None:
            logs = RR.log_jacobian_mp(Re)
            if memo is not None:
                memo["log", i] = logs
        e, J, _ = logs
        dRe = hatm(dld) * Re - Re * hatm(dl)
        de = mp.matrix([sum(J[c][3 * a_ + b_] * dRe[a_, b_] for a_ in range(3) for b_ in range(3)) for c in range(3)])
        al = had(kp_w, mp.matrix(e)) + had(kd_w, wd - wv) + mp.matrix([kff[3] * wd[0], kff[4] * wd[1] + kff[5] * wd[2], 0])
        dal = had(kp_w, de) + had(kd_w, dwd - tv("w_tan", 3)) + mp.matrix([kff[3] * dwd[0], kff[4] * dwd[1] + kff[5] * dwd[2], 0])
        Iw = R * Ib * R.T
        dIw = hatm(dl) * Iw - Iw * hatm(dl)
        dba = dIw * al + Iw * dal + cr(dwd, Iw * wd) + cr(wd, dIw * wd + Iw * dwd)
        db = mp.matrix([m * da[c] for c in range(3)] + [dba[c] for c in range(3)])
        # dr, dA, dg, the solve
        dpt = tv("feet_tan", 12)
        dA = mp.zeros(6, 12)
        for l in range(4):
            dp = mp.matrix([dpt[3 * l + c] for c in range(3)])
            if "joint_q_tan" in tans:
                ql = [lift(x) for x in np.asarray(b["joint_q"][i], float).reshape(4, 3)[l]]
                dql = tv("joint_q_tan", 12)
                dp = dp + DMR._jacobian_mp(l, ql, *(() if kin is None else (kin,))) * mp.matrix([dql[3 * l + c] for c in range(3)])
            dr = cr(dl, r[3 * l:3 * l + 3]) + R * dp
            dA[3:6, 3 * l:3 * l + 3] = hatm(dr)
        dg = 2 * (dA.T * v + A.T * (S * (dA * f - db)))
        Zn, _ = SR.face(active, float(P["mu"]))
        zy = mp.zeros(12, 1)
        if Zn.shape[1]:
            Z = mat(Zn, Zn.shape)
            H = 2 * (A.T * S * A + Wm)
            zy = Z * mp.lu_solve(Z.T * H * Z, Z.T * dg)
        out = []
        for l in range(4):
            fl = [f[3 * l + c] for c in range(3)]
            cf = cr(dl, fl)
            g = R.T * mp.matrix([zy[3 * l + c] + cf[c] for c in range(3)])
            out += [g[c] for c in range(3)]
        return dict(grf_tan=out, b_tan=[db[c] for c in range(6)])
