"""TEST INFRASTRUCTURE - numpy restatement of the device-side KKT certificate (csrc/qc_certify.hpp, qc_certify_batch), and the
same formulas for single robots at 50 digits.

certificate() is tests/kkt_batch.py's kkt_batch - the same floating-point expressions, line for line, wherever no axis has both
of its rows active - extended by what the device adds: the contact mask from gait_phase, feet from joint_q, the multipliers,
the active codes, the gradient, the flags, the both-rows rule and the batch summary.

The both-rows rule.  At the apex of the pyramid (fz = 0 = fzmin) the rows fx <= mu fz and -fx <= mu fz are both active, and
with fzmin = fzmax both fz rows are.  kkt_batch's sign s = upper - lower is 0 there, which it reads as "no row": a false
failure.  With both x rows the foot's stationarity in x is g_x + l1 - l2 = 0, l1, l2 >= 0: solvable for every g_x, and the
pair of least sum is (0, g_x) or (-g_x, 0), sum |g_x| - least is what matters because the z row g_z - mu (sum of the four
pyramid multipliers) + l5 - l6 = 0 with only the lower fz row active needs l6 = g_z - mu sum >= 0.  So: lam = |g|, no
contribution.  Both z rows: l5 - l6 is free, no contribution, and lam_z reports the net value mu (lam_x + lam_y) - g_z.

certificate_mp() evaluates grad, lambda, primal and stationarity of one robot at 50 digits with device_math_reference's tracked
arithmetic (Tr): next to each value it returns the sum of the absolute values of the terms that made it, the scale a double
evaluation's rounding error is measured on."""
from __future__ import annotations

import mpmath as mp
import numpy as np

from tests import device_math_reference as DMR
from tests.kkt_batch import wrench_data
from tests.leg_plant_restatement import contact_mask, fk

DEFAULT_DUTY = 0.8 / (0.18 + 0.8)  # the handle's stance_phase (qc_host.hpp derive_params)
SWING = 0x80


def with_feet(b, kin=None):
    """the batch with `feet` made from joint_q by the reference's forward kinematics, if it has none.  kin: the kinematic model
    (device_math_reference.Kin; default the library's) - a test at another model hands the restatements with_feet(b, kin)"""
    if b.get("feet") is not None or b.get("joint_q") is None:
        return b
    q = np.asarray(b["joint_q"], np.float64).reshape(-1, 4, 3)
    feet = np.array([[fk(l, q[i, l], *(() if kin is None else (kin,))) for l in range(4)] for i in range(q.shape[0])]).reshape(-1, 12)
    return dict(b, feet=feet)


def summarize(primal, stationarity, swing_nonzero, primal_tol=1e-7, stat_tol=1e-8):
    """qc_certify_summary from the per-robot arrays (a dict of Python numbers)"""
    fail = ~(primal <= primal_tol) | ~(stationarity <= stat_tol) | swing_nonzero
    out = dict(n_fail=int(fail.sum()), n_nonfinite=int((~np.isfinite(primal) | ~np.isfinite(stationarity)).sum()),
               n_swing_nonzero=int(swing_nonzero.sum()))
    for name, v in (("primal", primal), ("stationarity", stationarity)):
        fin = np.isfinite(v)
        if fin.any():
            w = np.where(fin, v, -np.inf)
            out["worst_" + name], out["arg_" + name] = float(w.max()), int(w.argmax())  # argmax: the lowest index on a tie
        else:
            out["worst_" + name], out["arg_" + name] = float("nan"), -1
    return out


def foot_conditions(fw, g, st, mu, fzmin, fzmax, act_tol=1e-7):
    """The per-foot part of the certificate from world-frame forces fw [m,4,3], gradients g [m,4,3] and the contact mask st [m,4]:
    kkt_batch's expressions, plus the both-rows rule, the multipliers and the active codes."""
    with np.errstate(invalid="ignore"):
        fx, fy, fz = fw[..., 0], fw[..., 1], fw[..., 2]
        viol = np.stack([np.abs(fx) - mu * fz, np.abs(fy) - mu * fz, fzmin - fz, fz - fzmax], axis=-1).max(axis=-1)
        primal = np.where(st, viol, 0.0).max(axis=1)
        swing_bad = (np.where(st[..., None], 0.0, np.abs(fw)) != 0.0).any(axis=(1, 2))
        tol = act_tol * (1.0 + np.abs(fz) * mu)
        ux, lx_ = np.where(mu * fz - fx <= tol, 1, 0), np.where(mu * fz + fx <= tol, 1, 0)
        uy, ly_ = np.where(mu * fz - fy <= tol, 1, 0), np.where(mu * fz + fy <= tol, 1, 0)
        uz, lz_ = np.where(fzmax - fz <= act_tol * (1.0 + fzmax), 1, 0), np.where(fz - fzmin <= act_tol * (1.0 + fzmin), 1, 0)
        sx, sy, sz = ux - lx_, uy - ly_, uz - lz_
        cx, cy, cz = lx_ + 2 * ux, ly_ + 2 * uy, lz_ + 2 * uz
        lx = -sx * g[..., 0]
        ly = -sy * g[..., 1]
        rx = np.where(cx == 3, 0.0, np.where(sx == 0, np.abs(g[..., 0]), np.maximum(0.0, -lx)))
        ry = np.where(cy == 3, 0.0, np.where(sy == 0, np.abs(g[..., 1]), np.maximum(0.0, -ly)))
        lxa = np.where(cx == 3, np.abs(g[..., 0]), np.where(sx == 0, 0.0, lx))
        lya = np.where(cy == 3, np.abs(g[..., 1]), np.where(sy == 0, 0.0, ly))
        ez = mu * (lxa + lya) - g[..., 2]
        rz = np.where(cz == 3, 0.0, np.where(sz == 0, np.abs(ez), np.maximum(0.0, -sz * ez)))
        lza = np.where(cz == 3, ez, np.where(sz == 0, 0.0, sz * ez))
        foot_res = np.where(st, np.maximum(np.maximum(rx, ry), rz), 0.0)
        lam = np.where(st[..., None], np.stack([lxa, lya, lza], axis=-1), 0.0)
        active = np.where(st, cx | (cy << 2) | (cz << 4), SWING).astype(np.uint8)
    return dict(primal=primal, swing_nonzero=swing_bad, foot_res=foot_res, lam=lam, active=active)


def certificate(P, b, grf_body, act_tol=1e-7, primal_tol=1e-7, stat_tol=1e-8, default_duty=DEFAULT_DUTY):
    """dict(primal [n], stationarity [n], swing_nonzero [n] bool, lam [n,4,3], active [n,4] uint8, grad [n,12], flags [n] int32,
    foot_res [n,4] (each stance foot's own residual contribution, 0 for swing feet), summary)."""
    with np.errstate(invalid="ignore"):
        b = with_feet(b)
        m = b["x"].shape[0]
        S = np.asarray(P["S"], float).reshape(6, 6)
        Wm = np.asarray(P["W"], float).reshape(12, 12)
        mu, fzmin, fzmax = P["mu"], P["fzmin"], P["fzmax"]
        A, bv = wrench_data(P, b)
        R = b["Rwb"].reshape(m, 3, 3)
        fw = -np.einsum("nij,nkj->nki", R, np.asarray(grf_body).reshape(m, 4, 3))
        f = fw.reshape(m, 12)
        u = np.einsum("nij,nj->ni", A, f) - bv
        grad = 2.0 * (np.einsum("nji,nj->ni", A, u @ S.T) + f @ Wm.T)
        gn = 1.0 + np.linalg.norm(grad, axis=1)
        g = grad.reshape(m, 4, 3)
        st = contact_mask(m, b.get("stance"), b.get("gait_phase"), b.get("gait_duty"), default_duty)
        c = foot_conditions(fw, g, st, mu, fzmin, fzmax, act_tol)
        primal, swing_bad, foot_res = c["primal"], c["swing_nonzero"], c["foot_res"]
        stat = foot_res.max(axis=1) / gn
        lam, active = c["lam"], c["active"]
        flags = (swing_bad.astype(np.int32) | ((~np.isfinite(primal) | ~np.isfinite(stat)).astype(np.int32) << 1)).astype(np.int32)
    return dict(primal=primal, stationarity=stat, swing_nonzero=swing_bad, lam=lam, active=active, grad=grad, flags=flags, foot_res=foot_res,
                summary=summarize(primal, stat, swing_bad, primal_tol, stat_tol))


# ------------------------------------------------------------------ 50 digits, one robot
def _abs(t):
    return DMR.Tr(abs(t.v), t.c, t.k)


def _max(a, b):
    return a if a.v >= b.v else b


def certificate_mp(P, b, grf_body, i, active, kin=None):
    """Robot i at 50 digits, with the active codes `active` [4] (uint8, as certificate() classified them: the test's points are
    exactly on a face or 1e-3 N inside).  kin = (hip [12], links [12]): the feet come from joint_q.  Returns
    dict(name -> (values as mp numbers, sums of |terms| as floats)) for grad [12], lam [12], primal [1], stationarity [1]."""
    Tr = DMR.Tr
    with mp.workdps(DMR.DPS):
        lift = lambda v: Tr(DMR.mpf(v))
        Pl = {k: [lift(v) for v in np.asarray(P[k], np.float64).reshape(-1)] for k, _ in DMR.WRENCH_P_KEYS}
        Pl["mass"] = Pl["mass"][0]
        Sl = {k: [lift(v) for v in np.asarray(b[k][i], np.float64).reshape(-1)] for k, _ in DMR.WRENCH_S_KEYS}
        if kin is not None:
            q = [lift(v) for v in np.asarray(b["joint_q"][i], np.float64).reshape(-1)]
            hip, links = ([lift(v) for v in np.asarray(a, np.float64).reshape(-1)] for a in kin)
            feet = [DMR._fk_tr(l, q[3 * l:3 * l + 3], hip, links) for l in range(4)]
        else:
            p = [lift(v) for v in np.asarray(b["feet"][i], np.float64).reshape(-1)]
            feet = [p[3 * l:3 * l + 3] for l in range(4)]
        bw, r, _ = DMR._wrench_core(Pl, Sl, feet, DMR._log_mp, lift)
        R = Sl["Rwb"]
        gb = [lift(v) for v in np.asarray(grf_body[i], np.float64).reshape(-1)]
        f = [-DMR._dot(R[3 * k:3 * k + 3], gb[3 * l:3 * l + 3]) for l in range(4) for k in range(3)]
        u = [f[k] + f[3 + k] + f[6 + k] + f[9 + k] for k in range(3)]
        tq = [DMR._cross(r[3 * l:3 * l + 3], f[3 * l:3 * l + 3]) for l in range(4)]
        u += [tq[0][k] + tq[1][k] + tq[2][k] + tq[3][k] for k in range(3)]
        u = [u[k] - bw[k] for k in range(6)]
        Sm = [lift(v) for v in np.asarray(P["S"], np.float64).reshape(-1)]
        Wm = [lift(v) for v in np.asarray(P["W"], np.float64).reshape(-1)]
        two, one, zero = lift(2.0), lift(1.0), lift(0.0)

        def total(terms):
            s = terms[0]
            for t in terms[1:]:
                s = s + t
            return s

        v = [total([Sm[6 * a + c] * u[c] for c in range(6)]) for a in range(6)]
        grad = []
        for l in range(4):
            c = DMR._cross(v[3:6], r[3 * l:3 * l + 3])
            for k in range(3):
                wf = total([Wm[12 * (3 * l + k) + m] * f[m] for m in range(12)])
                grad.append(two * ((v[k] + c[k]) + wf))
        gn = one + DMR.tr_sqrt(total([x * x for x in grad]))
        mu, fzmin, fzmax = lift(P["mu"]), lift(P["fzmin"]), lift(P["fzmax"])
        lam, primal, res = [], None, zero
        for l in range(4):
            code = int(active[l])
            if code & SWING:
                lam += [zero, zero, zero]
                primal = zero if primal is None else _max(primal, zero)
                continue
            fx, fy, fz = f[3 * l:3 * l + 3]
            viol = _max(_max(_abs(fx) - mu * fz, _abs(fy) - mu * fz), _max(fzmin - fz, fz - fzmax))
            primal = viol if primal is None else _max(primal, viol)
            lxy, rxy = [], []
            for axis, cd in ((0, code & 3), (1, (code >> 2) & 3)):
                gk = grad[3 * l + axis]
                if cd == 0:
                    lxy.append(zero); rxy.append(_abs(gk))
                elif cd == 3:
                    lxy.append(_abs(gk)); rxy.append(zero)
                else:
                    one_row = gk if cd == 1 else -gk
                    lxy.append(one_row); rxy.append(_max(zero, -one_row))
            ez = mu * (lxy[0] + lxy[1]) - grad[3 * l + 2]
            cz = (code >> 4) & 3
            lz = zero if cz == 0 else (-ez if cz == 1 else ez)
            rz = _abs(ez) if cz == 0 else (zero if cz == 3 else _max(zero, ez if cz == 1 else -ez))
            lam += [lxy[0], lxy[1], lz]
            res = _max(res, _max(_max(rxy[0], rxy[1]), rz))
        stat = res / gn
        pack = lambda ts: ([t.v for t in ts], np.array([float(t.c) for t in ts]))
        return dict(grad=pack(grad), lam=pack(lam), primal=pack([primal]), stationarity=pack([stat]))


def distance(values, mp_values):
    """|double - 50-digit value| per entry, as floats"""
    with mp.workdps(DMR.DPS):
        return np.array([float(abs(DMR.mpf(float(a)) - m)) for a, m in zip(np.asarray(values, np.float64).reshape(-1), mp_values)])


def magnitude(mp_values):
    """the largest |entry| of a 50-digit result, as a float"""
    with mp.workdps(DMR.DPS):
        return max(float(abs(m)) for m in mp_values)
