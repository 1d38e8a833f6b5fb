"""The desired COM of a step from the support polygon (qc_com_reference_batch) and its reverse pass (qc_com_reference_adjoint_batch)
restated on the CPU (tests/test_com_reference_cpu.py, tests/test_gpu_com_reference.py), written from include/qc_balance.h on top of
the polygon's restatement (tests/support_polygon_restatement.py: the robot, the ramps, the virtual points, the two arithmetics - Python
floats, and 50-digit values with condition sums) - not from the kernels.

reference_np / reference_adjoint_np in float64; reference_mp / reference_adjoint_mp at 50 digits on the exact double inputs with, per
output entry, the condition sum (the sum of the magnitudes of the terms).  ordered_sum repeats in numpy the order in which
schedule_bar_sum adds the rows (include/qc_balance.h, steps 1 to 3)."""
from __future__ import annotations

import math

import mpmath as mp
import numpy as np

from tests import support_polygon_restatement as SP
from tests.device_math_reference import DEFAULT_KIN, DPS
from tests.leg_plant_adjoint_restatement import Cs, _mtv

_F, _M = SP._F, SP._M
MODES = ("replace", "offset")
OUTPUTS = ("x_d_in_bar",) + SP.OUTPUTS
SIZES = dict(SP.SIZES, x_d_in_bar=3)
# C_FWD / C_REV: the worst |float64 restatement - 50-digit restatement| / (EPS x condition sum) of x_d_out and of the reverse outputs
# over SP.pool(24, saturating=6), both input forms and both modes at gain 0.7, as tests/test_com_reference_cpu.py measures it on the
# CPU (printed there: 0.299 forward - replace mode, the polygon's own figure; offset 0.241 - and 0.567 reverse, feet_bar in replace
# mode), rounded up with a little headroom; that test asserts the measurement stays below, tests/test_gpu_com_reference.py derives the
# device's bar (4 x) from it.
C_FWD, C_REV = 0.4, 0.7
# C_FWD_ODD / C_REV_ODD: the same measurement on the same draw at device_math_reference.ODD_KIN from joint_q (printed there: forward
# 0.284 replace, 0.157 offset; reverse 0.567, feet_bar in replace mode) - inside C_FWD and C_REV, so the odd model's bars are the
# default model's.
C_FWD_ODD, C_REV_ODD = C_FWD, C_REV
SUM_BLOCK, SUM_MAX_BLOCKS, SUM_GROUPS = 64, 1024, 16  # the wave, COM_SUM_MAX_BLOCKS and the finisher's groups


def _centroid(A, P):
    return [(P[SP.SUM_ORDER[0]][k] + P[SP.SUM_ORDER[1]][k] + P[SP.SUM_ORDER[2]][k] + P[SP.SUM_ORDER[3]][k]) / A.const(4.0) for k in range(2)]


def _forward(A, kin, b, sched, x_d, mode, gain, duty):
    n = np.asarray(b["gait_phase"]).shape[0]
    x_d = np.asarray(x_d, float)
    out, cc, com, flags = x_d.copy(), np.zeros((n, 3)), np.full((n, 2), np.nan), np.zeros(n, np.int32)
    for i in range(n):
        mask = SP.contact_mask(b, i, duty)
        _, P, _, ramps = SP._robot(A, kin, b, np.asarray(sched, float), i, mask, True)
        w = [r[4] for r in ramps]
        flags[i] = sum(1 << l for l in range(4) if SP._bad(A, w, l))
        if flags[i]:
            out[i, :2] = np.nan
            continue
        v = [SP._point(A, P, w, l)[3] for l in range(4)]
        c = [(v[SP.SUM_ORDER[0]][k] + v[SP.SUM_ORDER[1]][k] + v[SP.SUM_ORDER[2]][k] + v[SP.SUM_ORDER[3]][k]) / A.const(4.0) for k in range(2)]
        com[i] = SP._split(A, c)[0]
        if mode == "offset":
            cen = _centroid(A, P)
            c = [A.const(float(x_d[i, k])) + A.const(float(gain)) * (c[k] - cen[k]) for k in range(2)]
        out[i, :2], cond = SP._split(A, c)
        if cond is not None:
            cc[i, :2] = cond
    cc[:, 2] = np.abs(x_d[:, 2])
    return dict(x_d=out, com_xy=com, flags=flags), dict(x_d=cc)


def reference_np(b, sched, x_d, mode="replace", gain=1.0, duty=SP.TROT_DUTY, kin=DEFAULT_KIN):
    return _forward(_F, kin, b, sched, x_d, mode, gain, duty)[0]


def reference_mp(b, sched, x_d, mode="replace", gain=1.0, duty=SP.TROT_DUTY, kin=DEFAULT_KIN):
    with mp.workdps(DPS):
        return _forward(_M, kin, b, sched, x_d, mode, gain, duty)


def _adjoint(A, kin, b, sched, bar, mode, gain, duty, ins):
    n = np.asarray(b["gait_phase"]).shape[0]
    res = {k: np.full((n, SIZES[k]), np.nan) for k in OUTPUTS}
    cond = {k: np.zeros((n, SIZES[k])) for k in OUTPUTS}
    flags = np.zeros(n, np.int32)
    zero, one, four = A.const(0.0), A.const(1.0), A.const(4.0)
    for i in range(n):
        mask = SP.contact_mask(b, i, duty)
        pb, P, R, ramps = SP._robot(A, kin, b, np.asarray(sched, float), i, mask, True)
        w = [r[4] for r in ramps]
        flags[i] = sum(1 << l for l in range(4) if SP._bad(A, w, l))
        if flags[i]:
            continue
        acc = {k: [A.const(float(v)) for v in (np.asarray(ins[k + "_in"], float)[i].reshape(-1) if ins.get(k + "_in") is not None else np.zeros(SIZES[k]))]
               for k in SP.OUTPUTS}
        o = [A.const(float(v)) for v in bar[i]]
        if mode == "offset":
            acc["x_d_in_bar"] = list(o)
            g = [A.const(float(gain)) * o[k] / four for k in range(2)]
            Pb = [[-g[0], -g[1]] for _ in range(4)]  # the centroid: -gain o / 4 on every point
        else:
            acc["x_d_in_bar"] = [zero, zero, o[2]]
            g = [o[k] / four for k in range(2)]
            Pb = [[zero, zero] for _ in range(4)]
        wb = [zero] * 4
        for l in range(4):
            m, p = SP.MINUS[l], SP.PLUS[l]
            D, zm, zp, v = SP._point(A, P, w, l)
            Nb = [g[k] / D for k in range(2)]
            Db = -(g[0] * v[0] + g[1] * v[1]) / D
            dl = dm = dp = zero
            for k in range(2):
                dl = dl + Nb[k] * (P[l][k] + w[m] * (P[l][k] - P[m][k]) + w[p] * (P[l][k] - P[p][k]))
                dm = dm + Nb[k] * zm[k]
                dp = dp + Nb[k] * zp[k]
                Pb[l][k] = Pb[l][k] + (w[l] + w[l] * w[m] + w[l] * w[p]) * Nb[k]
                Pb[m][k] = Pb[m][k] + w[m] * (one - w[l]) * Nb[k]
                Pb[p][k] = Pb[p][k] + w[p] * (one - w[l]) * Nb[k]
            wb[l], wb[m], wb[p] = wb[l] + (Db + dl), wb[m] + (Db + dm), wb[p] + (Db + dp)
        isp, root2 = A.const(1.0 / math.sqrt(math.pi)) if A is _F else Cs(1 / mp.sqrt(mp.pi)), A.const(math.sqrt(2.0))
        for l in range(4):
            a1, a2, d1, d2, _ = ramps[l]
            e1, e2 = A.exp_neg_sq(a1) * isp, A.exp_neg_sq(a2) * isp
            ph = wb[l] * (e1 / d1 - e2 / d2)
            acc["phase_bar"][l] = acc["phase_bar"][l] + (ph if mask[l] else -ph)
            s = 0 if mask[l] else 2
            acc["schedule_bar"][4 * l + s] = acc["schedule_bar"][4 * l + s] + (-(wb[l] * e1 * a1 * root2 / d1))
            acc["schedule_bar"][4 * l + s + 1] = acc["schedule_bar"][4 * l + s + 1] + (-(wb[l] * e2 * a2 * root2 / d2))
            pw = [Pb[l][0], Pb[l][1], zero]
            ft = _mtv(R, pw)
            for k in range(3):
                acc["feet_bar"][3 * l + k] = acc["feet_bar"][3 * l + k] + ft[k]
                acc["Rwb_bar"][k] = acc["Rwb_bar"][k] + pw[0] * pb[l][k]
                acc["Rwb_bar"][3 + k] = acc["Rwb_bar"][3 + k] + pw[1] * pb[l][k]
            acc["x_bar"][0], acc["x_bar"][1] = acc["x_bar"][0] + pw[0], acc["x_bar"][1] + pw[1]
        for k in OUTPUTS:
            res[k][i], c = SP._split(A, acc[k])
            if c is not None:
                cond[k][i] = c
    return res, cond, flags


def reference_adjoint_np(b, sched, bar, mode="replace", gain=1.0, duty=SP.TROT_DUTY, kin=DEFAULT_KIN, **ins):
    res, _, flags = _adjoint(_F, kin, b, sched, np.asarray(bar, float), mode, gain, duty, ins)
    return res, flags


def reference_adjoint_mp(b, sched, bar, mode="replace", gain=1.0, duty=SP.TROT_DUTY, kin=DEFAULT_KIN, **ins):
    with mp.workdps(DPS):
        return _adjoint(_M, kin, b, sched, np.asarray(bar, float), mode, gain, duty, ins)


def ordered_sum(rows):
    """schedule_bar_sum of the rows [n, 16] (or [n, 4, 4]) in the kernel's documented order: B = min(ceil(n / 64), 1024) partials, each
    the rows of its 64-robot pieces b, b + B, ... added one by one in index order from 0.0; 16 groups, group w the partials w, w + 16,
    ... in rising order from 0.0; the groups in rising order."""
    rows = np.asarray(rows, np.float64).reshape(len(rows), 16)
    n = rows.shape[0]
    B = min((n + SUM_BLOCK - 1) // SUM_BLOCK, SUM_MAX_BLOCKS)
    partial = np.zeros((B, 16))
    for b in range(B):
        for base in range(b * SUM_BLOCK, n, B * SUM_BLOCK):
            for i in range(base, min(base + SUM_BLOCK, n)):
                partial[b] = partial[b] + rows[i]
    group = np.zeros((SUM_GROUPS, 16))
    for w in range(SUM_GROUPS):
        for p in range(w, B, SUM_GROUPS):
            group[w] = group[w] + partial[p]
    total = group[0].copy()
    for w in range(1, SUM_GROUPS):
        total = total + group[w]
    return total
