"""The forward mode of the COM reference (qc_com_reference_tangent_batch, include/qc_tangent.h) restated on the CPU
(tests/test_com_reference_tangent_cpu.py, tests/test_gpu_com_reference_tangent.py), written from the model's equations and not from the
kernel, on top of tests/support_polygon_restatement.py (the robot, the ramps, the virtual points, the pool, the two arithmetics -
Python floats, and 50-digit values with condition sums) and tests/com_reference_restatement.py (the modes, the adjoint it pairs with).

The contact mask is HELD.  Per direction and leg l, r_l = Rwb p_l, e_i = exp(-a_i^2) / sqrt(pi):
  dp_l = feet_tan_l + J(q_l) joint_q_tan_l,   dP_l = (delta x r_l + Rwb dp_l + dx) in x and y
  dw_l = sgn (e1 / d1 - e2 / d2) dphi_l - sum_i e_i a_i sqrt(2) / d_i dsigma_i       over the two widths the leg's branch reads
  dzm = w dP + (1 - w) dP_m + (P - P_m) dw, dzp likewise;  dN, dD by the product rule;  dv = (dN - v dD) / D
  com_xy_tan = (dv_FL + dv_FR + dv_RL + dv_RR) / 4
  replace  x_d_out_tan = (com_xy_tan, x_d_in_tan.z);   offset  x_d_out_tan = x_d_in_tan + gain (com_xy_tan - mean dP, 0)
FLAGS  bit l: the forward rule; every row of the robot is NaN in every direction."""
from __future__ import annotations

import math

import mpmath as mp
import numpy as np

from tests import support_polygon_restatement as SP
from tests.device_math_reference import DEFAULT_KIN, DPS, EPS  # noqa: F401
from tests.leg_plant_adjoint_restatement import Cs, _cr, _Leg, _mv
from tests.swing_tangent_restatement import exp_rotation, skew_times

_F, _M = SP._F, SP._M
TANGENTS = {"x_d_in_tan": 3, "feet_tan": 12, "joint_q_tan": 12, "Rwb_rot_tan": 3, "x_tan": 3, "phase_tan": 4, "schedule_tan": 16}
OUTPUTS = {"x_d_out_tan": 3, "com_xy_tan": 2}
BAR_OF = {"x_d_in_tan": "x_d_in_bar", "x_tan": "x_bar", "phase_tan": "phase_bar", "schedule_tan": "schedule_bar"}
# C_MT: the worst |tangent_np - tangent_mp| / (EPS x condition sum) of x_d_out_tan / com_xy_tan over SP.pool(24, saturating=6), both
# input forms and both modes at gain 0.7, three directions, as tests/test_com_reference_tangent_cpu.py measures it on the CPU against
# 50 digits (printed there: 0.150 / 0.147 at worst, `feet`, per-robot schedule), rounded up with a little headroom; that test asserts the measurement stays below,
# tests/test_gpu_com_reference_tangent.py derives the device's bar (4 C_MT) from it.  Never measured on the device.
C_MT = {"x_d_out_tan": 0.2, "com_xy_tan": 0.2}
# C_MDOT: the worst gap of the pairing <x_d_out_bar, tangent_np's x_d_out_tan> = <reference_adjoint_np's outputs, tangents>, in EPS x
# the sum of the magnitudes of all terms on both sides, over the same pools the same way.  Measured: 4.834 (`feet`, a per-robot schedule, replace mode: a robot of
# the saturating family, whose width terms are quotients by d = 1e-12).
C_MDOT = 4.9


def random_tangents(n, K, seed=89, joint_q=False, shared=False):
    """{name: [K, n, m]} - feet_tan, or joint_q_tan for a batch with joint_q; schedule_tan [K, 16] for a shared schedule"""
    rng = np.random.default_rng(seed)
    scale = {"x_d_in_tan": 0.01, "feet_tan": 0.01, "joint_q_tan": 0.1, "Rwb_rot_tan": 0.1, "x_tan": 0.01, "phase_tan": 0.05, "schedule_tan": 0.05}
    t = {k: rng.normal(0.0, scale[k], (K, n, m)) for k, m in TANGENTS.items()}
    t.pop("feet_tan" if joint_q else "joint_q_tan")
    if shared:
        t["schedule_tan"] = np.ascontiguousarray(t["schedule_tan"][:, 0])
    return t


def _tangent_one(A, kin, b, sched, i, mask, mode, gain, t):
    """t: flat float arrays over TANGENTS (schedule_tan [16] of this robot).  Returns (x_d_out_tan [3], com_xy_tan [2]) A-values."""
    c = A.const
    vec = lambda a: [c(v) for v in np.asarray(a, float).reshape(-1)]
    pb, P, R, ramps = SP._robot(A, kin, b, sched, i, mask, True)
    w = [r[4] for r in ramps]
    xdt, ft, dq, dl, dx, dph, dsg = (vec(t[k]) for k in ("x_d_in_tan", "feet_tan", "joint_q_tan", "Rwb_rot_tan", "x_tan", "phase_tan", "schedule_tan"))
    one = c(1.0)
    isp, root2 = c(1.0 / math.sqrt(math.pi)) if A is _F else Cs(1 / mp.sqrt(mp.pi)), c(math.sqrt(2.0))
    dP, dw = [], []
    for l in range(4):
        dp = ft[3 * l:3 * l + 3]
        if b.get("joint_q") is not None:
            q = vec(b["joint_q"][i])
            jdq = _mv(_Leg(A, l, q[3 * l:3 * l + 3], kin).J, dq[3 * l:3 * l + 3])
            dp = [dp[k] + jdq[k] for k in range(3)]
        cr, rdp = _cr(dl, _mv(R, pb[l])), _mv(R, dp)
        dP.append([cr[k] + rdp[k] + dx[k] for k in range(2)])
        a1, a2, d1, d2, _ = ramps[l]
        e1, e2 = A.exp_neg_sq(a1) * isp, A.exp_neg_sq(a2) * isp
        ph = (e1 / d1 - e2 / d2) * dph[l]
        s = 0 if mask[l] else 2
        dw.append((ph if mask[l] else -ph) - (e1 * a1 * root2 / d1 * dsg[4 * l + s] + e2 * a2 * root2 / d2 * dsg[4 * l + s + 1]))
    dv = []
    for l in range(4):
        m, p = SP.MINUS[l], SP.PLUS[l]
        D, zm, zp, v = SP._point(A, P, w, l)
        dD = dw[l] + dw[m] + dw[p]
        row = []
        for k in range(2):
            dzm = w[l] * dP[l][k] + (one - w[l]) * dP[m][k] + (P[l][k] - P[m][k]) * dw[l]
            dzp = w[l] * dP[l][k] + (one - w[l]) * dP[p][k] + (P[l][k] - P[p][k]) * dw[l]
            dN = dw[l] * P[l][k] + w[l] * dP[l][k] + dw[m] * zm[k] + w[m] * dzm + dw[p] * zp[k] + w[p] * dzp
            row.append((dN - v[k] * dD) / D)
        dv.append(row)
    four = c(4.0)
    com = [(dv[SP.SUM_ORDER[0]][k] + dv[SP.SUM_ORDER[1]][k] + dv[SP.SUM_ORDER[2]][k] + dv[SP.SUM_ORDER[3]][k]) / four for k in range(2)]
    if mode == "offset":
        cen = [(dP[SP.SUM_ORDER[0]][k] + dP[SP.SUM_ORDER[1]][k] + dP[SP.SUM_ORDER[2]][k] + dP[SP.SUM_ORDER[3]][k]) / four for k in range(2)]
        out = [xdt[k] + c(float(gain)) * (com[k] - cen[k]) for k in range(2)] + [xdt[2]]
    else:
        out = com + [xdt[2]]
    return out, com


def _tangent(A, kin, b, sched, tans, mode, gain, duty):
    n = np.asarray(b["gait_phase"]).shape[0]
    sched = np.asarray(sched, float)
    shared = sched.ndim == 2
    K = next(np.asarray(t).shape[0] for t in tans.values() if t is not None)
    t = {k: (np.zeros((K, n, m)) if tans.get(k) is None else np.asarray(tans[k], np.float64)) for k, m in TANGENTS.items()}
    if shared and tans.get("schedule_tan") is not None:
        t["schedule_tan"] = np.broadcast_to(t["schedule_tan"].reshape(K, 1, 16), (K, n, 16))
    t = {k: np.asarray(v).reshape(K, n, TANGENTS[k]) for k, v in t.items()}
    val = {k: np.zeros((K, n, m)) for k, m in OUTPUTS.items()}
    cond = {k: np.zeros((K, n, m)) for k, m in OUTPUTS.items()} if A is _M else None
    flags = np.zeros(n, np.int32)
    for i in range(n):
        mask = SP.contact_mask(b, i, duty)
        _, _, _, ramps = SP._robot(A, kin, b, sched, i, mask, True)
        w = [r[4] for r in ramps]
        flags[i] = sum(1 << l for l in range(4) if SP._bad(A, w, l))
        if flags[i]:
            for k in OUTPUTS:
                val[k][:, i] = np.nan
            continue
        for kd in range(K):
            out, com = _tangent_one(A, kin, b, sched, i, mask, mode, gain, {name: t[name][kd, i] for name in TANGENTS})
            for name, vals in (("x_d_out_tan", out), ("com_xy_tan", com)):
                val[name][kd, i], cs = SP._split(A, vals)
                if cs is not None:
                    cond[name][kd, i] = cs
    if cond is not None:
        cond["x_d_out_tan"][:, :, 2] = 0.0  # a copy
    return val, cond, flags


def tangent_np(b, sched, tans, mode="replace", gain=1.0, duty=SP.TROT_DUTY, kin=DEFAULT_KIN):
    """float64: (dict over OUTPUTS of [K, n, m], flags [n] int32)"""
    val, _, flags = _tangent(_F, kin, b, sched, tans, mode, gain, duty)
    return val, flags


def tangent_mp(b, sched, tans, mode="replace", gain=1.0, duty=SP.TROT_DUTY, kin=DEFAULT_KIN):
    """50 digits: (values rounded to double, condition sums, flags)"""
    with mp.workdps(DPS):
        return _tangent(_M, kin, b, sched, tans, mode, gain, duty)


def feet_tangent(b, tans, kin=DEFAULT_KIN):
    """dp [K, n, 12] in float64: feet_tan + J(q) joint_q_tan - what the adjoint's feet_bar pairs with"""
    some = next(v for v in tans.values() if v is not None)
    K, n = np.asarray(some).shape[0], np.asarray(b["gait_phase"]).shape[0]
    dp = np.zeros((K, n, 12)) if tans.get("feet_tan") is None else np.asarray(tans["feet_tan"], np.float64).reshape(K, n, 12).copy()
    if tans.get("joint_q_tan") is not None:
        dq = np.asarray(tans["joint_q_tan"], np.float64).reshape(K, n, 12)
        for i in range(n):
            for l in range(4):
                J = np.array(_Leg(_F, l, [float(v) for v in np.asarray(b["joint_q"][i]).reshape(-1)[3 * l:3 * l + 3]], kin).J, float).reshape(3, 3)
                dp[:, i, 3 * l:3 * l + 3] += dq[:, i, 3 * l:3 * l + 3] @ J.T
    return dp


def pairing(bar, out_tan, tans, adj, b, shared_sum=None, kin=DEFAULT_KIN):
    """The two sides of <x_d_out_bar, x_d_out_tan> = <x_d_in_bar, x_d_in_tan> + <feet_bar, dp> + <Rwb_bar, [delta]x Rwb> + <x_bar, dx> +
    <phase_bar, dphi> + <schedule_bar, dsigma> per (direction, robot), and the sum of the magnitudes of all terms.  With `shared_sum`
    (schedule_bar_sum [16]; tans["schedule_tan"] is [K, 16]) the schedule's term is left out per robot and the totals over the batch
    are returned instead: (lhs [K], rhs [K], terms [K])."""
    K, n = np.asarray(out_tan).shape[:2]
    g = lambda a, m: np.broadcast_to(np.asarray(a, np.float64).reshape(1, n, m), (K, n, m))
    pairs_l = [(g(bar, 3), np.asarray(out_tan, np.float64).reshape(K, n, 3))]
    pairs_r = [(g(adj["feet_bar"], 12), feet_tangent(b, tans, kin))]
    for name, key in BAR_OF.items():
        if tans.get(name) is not None and not (name == "schedule_tan" and shared_sum is not None):
            pairs_r.append((g(adj[key], TANGENTS[name]), np.asarray(tans[name], np.float64).reshape(K, n, TANGENTS[name])))
    if tans.get("Rwb_rot_tan") is not None:
        pairs_r.append((g(adj["Rwb_bar"], 9), skew_times(np.asarray(tans["Rwb_rot_tan"], np.float64).reshape(K, n, 3), g(b["Rwb"], 9))))

    def side(pairs):
        tot, mag = np.zeros((K, n)), np.zeros((K, n))
        for a, t in pairs:
            tot += (a * t).sum(axis=2)
            mag += (np.abs(a) * np.abs(t)).sum(axis=2)
        return tot, mag

    (lhs, ml), (rhs, mr) = side(pairs_l), side(pairs_r)
    if shared_sum is None:
        return lhs, rhs, ml + mr
    s, dsg = np.asarray(shared_sum, np.float64).reshape(1, 16), np.asarray(tans["schedule_tan"], np.float64).reshape(K, 16)
    return lhs.sum(axis=1), rhs.sum(axis=1) + (s * dsg).sum(axis=1), (ml + mr).sum(axis=1) + (np.abs(s) * np.abs(dsg)).sum(axis=1)


def moved(b, sched, x_d, tans, k, h, kin=DEFAULT_KIN):
    """the batch, the schedule and x_d moved by h along direction k of `tans` (the rotation along its left tangent); the stance bytes
    are those of the unmoved batch: the mask is held"""
    n = np.asarray(b["gait_phase"]).shape[0]
    out = dict(b)
    if b.get("stance") is None:
        out["stance"] = np.array([SP.contact_mask(b, i, SP.TROT_DUTY) for i in range(n)], np.uint8)
    get = lambda name, m: np.zeros((n, m)) if tans.get(name) is None else np.asarray(tans[name], np.float64)[k].reshape(-1, m)
    for name, key, m in (("feet", "feet_tan", 12), ("joint_q", "joint_q_tan", 12), ("x", "x_tan", 3), ("gait_phase", "phase_tan", 4)):
        if b.get(name) is not None and tans.get(key) is not None:
            out[name] = np.asarray(b[name]) + h * get(key, m).reshape(np.asarray(b[name]).shape)
    d = get("Rwb_rot_tan", 3)
    out["Rwb"] = np.stack([exp_rotation(h * d[i]) @ np.asarray(b["Rwb"][i]).reshape(3, 3) for i in range(n)]).reshape(n, 9)
    sched = np.asarray(sched, float)
    if tans.get("schedule_tan") is not None:
        sched = sched + h * np.asarray(tans["schedule_tan"], np.float64)[k].reshape(sched.shape if sched.ndim == 2 else (n, 4, 4))
    return out, sched, np.asarray(x_d) + h * get("x_d_in_tan", 3)
