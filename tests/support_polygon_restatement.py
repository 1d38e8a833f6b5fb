"""The virtual support polygon (qc_support_polygon_batch) and its reverse pass (qc_support_polygon_adjoint_batch) restated on the CPU
(tests/test_support_polygon_cpu.py, tests/test_gpu_support_polygon.py), written from SupportPolygon::position (trajectory.cpp:81-147)
in its evaluation order and from include/qc_balance.h - not from the kernels.

One robot's forward and reverse pass are written ONCE over an arithmetic (tests/leg_plant_adjoint_restatement.py: `_Float`, Python
floats and libm's erf / exp; `_Mp`, 50-digit values with condition sums - a + b -> c_a + c_b, a * b -> c_a c_b, a / b -> c_a c_b / b^2;
erf(a) and exp(-a^2) enter with |f| + |f'(a)| c_a, their own magnitude and what the argument's rounding does to them) and evaluated
twice: reference_np / reference_adjoint_np in float64, reference_mp / reference_adjoint_mp at 50 digits on the exact double inputs
with, per output entry, the condition sum (the sum of the magnitudes of the terms).

What is DECIDED is decided in double in both arithmetics, as the kernels decide it: the contact mask (`stance` bytes, else the phase
rule with its 1e-12 slack).  A robot with a zero or non-finite denominator is flagged (bit l) and NaN.

Legs RL, FL, RR, FR = 0, 1, 2, 3.  The weight reads the RAW phase; the four widths of a leg are LegScheduledPhases' (stance_start,
stance_end, swing_start, swing_end), the sigma of the ramps."""
from __future__ import annotations

import math

import mpmath as mp
import numpy as np

from tests.device_math_reference import DEFAULT_KIN, DPS, EPS
from tests.leg_plant_adjoint_restatement import Cs, _Float, _Leg, _Mp, _mtv, _mv

MINUS, PLUS = (1, 3, 0, 2), (2, 0, 3, 1)  # adjacent_leg_map_ (trajectory.cpp:75-78): RL: (FL, RR), FL: (FR, RL), RR: (RL, FR), FR: (RR, FL)
SUM_ORDER = (1, 3, 0, 2)                  # std::map order of the names: FL, FR, RL, RR
OUTPUTS = ("feet_bar", "Rwb_bar", "x_bar", "phase_bar", "schedule_bar")
SIZES = {"feet_bar": 12, "Rwb_bar": 9, "x_bar": 3, "phase_bar": 4, "schedule_bar": 16}
INS = tuple(k + "_in" for k in OUTPUTS)
# C_FWD / C_REV: the worst |float64 restatement - 50-digit restatement| / (EPS x condition sum) of com_xy and of the reverse outputs
# over pool(24, saturating=6), both input forms and both modes, as tests/test_support_polygon_cpu.py measures it (printed there: 0.299
# and 0.640), rounded up with a little headroom; that test asserts the measurement stays below, tests/test_gpu_support_polygon.py
# derives the device's bar (4 x) from it.
C_FWD, C_REV = 0.4, 0.8
# C_FWD_ODD / C_REV_ODD: the same measurement on the same draw at device_math_reference.ODD_KIN from joint_q (printed there: forward
# 0.150 body, 0.284 world; reverse 0.590, feet_bar) - inside C_FWD and C_REV, so the odd model's bars are the default model's.
C_FWD_ODD, C_REV_ODD = C_FWD, C_REV
TROT_OFFSETS, TROT_DUTY = (0.0, 0.5, 0.5, 0.0), 0.5
# the test_node.cpp:41-57 vector, legs in this module's order
NODE_SCHEDULE = np.array([[0.0, 0.5, 0.5, 1.0], [0.5, 1.0, 0.0, 0.5], [0.5, 1.0, 0.0, 0.5], [0.0, 0.5, 0.5, 1.0]])
NODE_PHASE = np.array([0.2, 0.6, 0.6, 0.2])
NODE_STANCE = np.array([1, 0, 0, 1], np.uint8)
NODE_FEET = np.array([[-0.196, 0.050, 0.0], [0.196, 0.050, 0.0], [-0.196, -0.050, 0.0], [0.196, -0.050, 0.0]])
NODE_WEIGHTS = (0.945200708300191, 0.21185539858372443)  # (RL, FR) and (FL, RR)


class _F(_Float):
    erf = staticmethod(math.erf)

    @staticmethod
    def exp_neg_sq(a):
        s = a * a
        return math.exp(-s) if s < 745.0 else 0.0


class _M(_Mp):
    @staticmethod
    def erf(a):
        v = mp.erf(a.v)
        return Cs(v, abs(v) + 2 / mp.sqrt(mp.pi) * mp.exp(-a.v * a.v) * a.c)

    @staticmethod
    def exp_neg_sq(a):
        v = mp.exp(-a.v * a.v)
        return Cs(v, v + 2 * abs(a.v) * v * a.c)


def in_stance(ph, duty):
    almost = lambda a, b: abs(a - b) < 1.0e-12
    return (ph > 0.0 or almost(ph, 0.0)) and (ph < duty or almost(ph, duty))


def contact_mask(b, i, duty):
    if b.get("stance") is not None:
        return [bool(v) for v in b["stance"][i]]
    d = duty if b.get("gait_duty") is None else float(b["gait_duty"][i])
    return [in_stance(float(p), d) for p in b["gait_phase"][i]]


def _ramp(A, st, ph, c):
    """(a1, a2, d1, d2, w) of one leg: trajectory.cpp:93-113"""
    root2, eps, one = A.const(math.sqrt(2.0)), A.const(1.0e-12), A.const(1.0)
    d1 = (c[0] if st else c[2]) * root2 + eps
    d2 = (c[1] if st else c[3]) * root2 + eps
    if st:
        a1, a2 = ph / d1, (one - ph) / d2
        w = A.const(0.5) * (A.erf(a1) + A.erf(a2))
    else:
        a1, a2 = -ph / d1, (ph - one) / d2
        w = A.const(0.5) * (A.const(2.0) + A.erf(a1) + A.erf(a2))
    return a1, a2, d1, d2, w


def _robot(A, kin, b, sched, i, mask, world):
    """the body-frame feet, the four points, the rotation and the ramps of robot i"""
    cv = lambda a: [A.const(float(v)) for v in np.asarray(a, float).reshape(-1)]
    if b.get("joint_q") is not None:
        q = cv(b["joint_q"][i])
        pb = [_Leg(A, l, q[3 * l:3 * l + 3], kin).p for l in range(4)]
    else:
        f = cv(b["feet"][i])
        pb = [f[3 * l:3 * l + 3] for l in range(4)]
    R = cv(b["Rwb"][i]) if world else None
    if world:
        x = cv(b["x"][i])
        P = [[r + xx for r, xx in zip(_mv(R, p)[:2], x[:2])] for p in pb]
    else:
        P = [p[:2] for p in pb]
    ph = cv(b["gait_phase"][i])
    s = sched if sched.ndim == 2 else sched[i]
    ramps = [_ramp(A, mask[l], ph[l], cv(s[l])) for l in range(4)]
    return pb, P, R, ramps


def _point(A, P, w, l):
    m, p = MINUS[l], PLUS[l]
    one = A.const(1.0)
    D = w[l] + w[m] + w[p]
    zm = [P[l][k] * w[l] + P[m][k] * (one - w[l]) for k in range(2)]
    zp = [P[l][k] * w[l] + P[p][k] * (one - w[l]) for k in range(2)]
    v = [(one / D) * (w[l] * P[l][k] + w[m] * zm[k] + w[p] * zp[k]) for k in range(2)]
    return D, zm, zp, v


def _bad(A, w, l):
    D = A.val(w[l]) + A.val(w[MINUS[l]]) + A.val(w[PLUS[l]])
    return not (D != 0.0 and math.isfinite(D))


def _split(A, vals):
    """-> (values [k] float, condition sums [k] float or None)"""
    if A is _F:
        return np.array([float(v) for v in vals]), None
    return np.array([float(v.v) for v in vals]), np.array([v.c for v in vals])


def _forward(A, kin, b, sched, world, duty):
    n = np.asarray(b["gait_phase"]).shape[0]
    com, wts, cc, flags = np.full((n, 2), np.nan), np.zeros((n, 4)), np.zeros((n, 2)), np.zeros(n, np.int32)
    for i in range(n):
        mask = contact_mask(b, i, duty)
        _, P, _, ramps = _robot(A, kin, b, np.asarray(sched, float), i, mask, world)
        w = [r[4] for r in ramps]
        wts[i] = [A.val(v) for v in w]
        flags[i] = sum(1 << l for l in range(4) if _bad(A, w, l))
        if flags[i]:
            continue
        v = [_point(A, P, w, l)[3] for l in range(4)]
        out = [(v[SUM_ORDER[0]][k] + v[SUM_ORDER[1]][k] + v[SUM_ORDER[2]][k] + v[SUM_ORDER[3]][k]) / A.const(4.0) for k in range(2)]
        com[i], c = _split(A, out)
        if c is not None:
            cc[i] = c
    return dict(com_xy=com, weights=wts, flags=flags), dict(com_xy=cc)


def reference_np(b, sched, world=False, duty=TROT_DUTY, kin=DEFAULT_KIN):
    return _forward(_F, kin, b, sched, world, duty)[0]


def reference_mp(b, sched, world=False, duty=TROT_DUTY, kin=DEFAULT_KIN):
    with mp.workdps(DPS):
        return _forward(_M, kin, b, sched, world, duty)


def _adjoint(A, kin, b, sched, bar, world, duty, ins):
    n = np.asarray(b["gait_phase"]).shape[0]
    res = {k: np.full((n, SIZES[k]), np.nan) for k in OUTPUTS}
    cond = {k: np.zeros((n, SIZES[k])) for k in OUTPUTS}
    flags = np.zeros(n, np.int32)
    zero, one, quarter = A.const(0.0), A.const(1.0), A.const(4.0)
    for i in range(n):
        mask = contact_mask(b, i, duty)
        pb, P, R, ramps = _robot(A, kin, b, np.asarray(sched, float), i, mask, world)
        w = [r[4] for r in ramps]
        flags[i] = sum(1 << l for l in range(4) if _bad(A, w, l))
        if flags[i]:
            continue
        acc = {k: [A.const(float(v)) for v in (np.asarray(ins[k + "_in"], float)[i].reshape(-1) if ins.get(k + "_in") is not None else np.zeros(SIZES[k]))]
               for k in OUTPUTS}
        g = [A.const(float(v)) / quarter for v in bar[i]]
        wb, Pb = [zero] * 4, [[zero, zero] for _ in range(4)]
        for l in range(4):
            m, p = MINUS[l], PLUS[l]
            D, zm, zp, v = _point(A, P, w, l)
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
            o = 0 if mask[l] else 2
            acc["schedule_bar"][4 * l + o] = acc["schedule_bar"][4 * l + o] + (-(wb[l] * e1 * a1 * root2 / d1))
            acc["schedule_bar"][4 * l + o + 1] = acc["schedule_bar"][4 * l + o + 1] + (-(wb[l] * e2 * a2 * root2 / d2))
            pw = [Pb[l][0], Pb[l][1], zero]
            if world:
                ft = _mtv(R, pw)
                for k in range(3):
                    acc["feet_bar"][3 * l + k] = acc["feet_bar"][3 * l + k] + ft[k]
                    acc["Rwb_bar"][k] = acc["Rwb_bar"][k] + pw[0] * pb[l][k]
                    acc["Rwb_bar"][3 + k] = acc["Rwb_bar"][3 + k] + pw[1] * pb[l][k]
                acc["x_bar"][0], acc["x_bar"][1] = acc["x_bar"][0] + pw[0], acc["x_bar"][1] + pw[1]
            else:
                acc["feet_bar"][3 * l], acc["feet_bar"][3 * l + 1] = acc["feet_bar"][3 * l] + pw[0], acc["feet_bar"][3 * l + 1] + pw[1]
        for k in OUTPUTS:
            res[k][i], c = _split(A, acc[k])
            if c is not None:
                cond[k][i] = c
    return res, cond, flags


def reference_adjoint_np(b, sched, bar, world=False, duty=TROT_DUTY, kin=DEFAULT_KIN, **ins):
    res, _, flags = _adjoint(_F, kin, b, sched, np.asarray(bar, float), world, duty, ins)
    return res, flags


def reference_adjoint_mp(b, sched, bar, world=False, duty=TROT_DUTY, kin=DEFAULT_KIN, **ins):
    with mp.workdps(DPS):
        return _adjoint(_M, kin, b, sched, np.asarray(bar, float), world, duty, ins)


# ------------------------------------------------------------------ the input draw, shared with the GPU tests
HOME = (0.0, 0.8, -1.6)


def _rotation(rng):
    a = rng.uniform(-0.4, 0.4, 3)
    cx, sx, cy, sy, cz, sz = math.cos(a[0]), math.sin(a[0]), math.cos(a[1]), math.sin(a[1]), math.cos(a[2]), math.sin(a[2])
    Rx, Ry, Rz = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]), np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]), np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).reshape(9)


def pool(n=257, seed=61, saturating=0):
    """n robots of a trot (offsets TROT_OFFSETS, duty TROT_DUTY): phases at least 1e-3 from 0, the duty and 1, widths uniform in
    [0.05, 0.5] - no robot is flagged (the smallest denominator over 20 000 draws is 0.504).  The LAST `saturating` robots are the
    second family: widths in {0, 1e-3} and phases within +-3 ulp of 0 and of the duty (stance bytes follow the phase rule), where the
    erf arguments saturate.  -> (batch dict of numpy arrays: feet, joint_q, gait_phase, Rwb, x; schedule [n,4,4])"""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.0, 1.0, n)
    ph = np.mod(base[:, None] + np.array(TROT_OFFSETS)[None, :], 1.0)
    for edge in (0.0, TROT_DUTY, 1.0):
        near = np.abs(ph - edge) < 1e-3
        ph = np.where(near, edge + np.where(ph >= edge, 2e-3, -2e-3), ph)
    ph = np.mod(ph, 1.0)
    sched = rng.uniform(0.05, 0.5, (n, 4, 4))
    feet = NODE_FEET[None] + rng.uniform(-0.05, 0.05, (n, 4, 3)) + np.array([0.0, 0.0, -0.3])
    q = np.tile(np.array(HOME), (n, 4)).reshape(n, 4, 3) + rng.uniform(-0.3, 0.3, (n, 4, 3))
    for i in range(n - saturating, n):
        sched[i] = rng.choice([0.0, 1e-3], (4, 4))
        for l in range(4):
            edge = (0.0, TROT_DUTY)[int(rng.integers(2))]
            v = edge
            for _ in range(int(rng.integers(0, 4))):
                v = np.nextafter(v, 1.0 if rng.integers(2) or edge == 0.0 else 0.0)
            ph[i, l] = v
    return dict(feet=feet, joint_q=q, gait_phase=ph, Rwb=np.array([_rotation(rng) for _ in range(n)]), x=rng.uniform(-1.0, 1.0, (n, 3))), sched


TINY = 2.0 ** -1022  # the smallest normal double


def worst_ratio(val, ref, cond):
    """max |val - ref| / (EPS cond + TINY).  TINY: the condition sums model roundings that are relative; an erf argument of the
    saturating family (a phase 1 to 3 ulp above 0 over a width) lies BELOW the normal range, where a rounding is an absolute 2^-1075.
    The reverse pass multiplies such an argument by wb e sqrt2 / d <= 1e13 (d >= 1e-12), so what it leaves is below 1e-310 - far
    under TINY, which therefore bounds it without loosening anything of normal size."""
    val, ref, cond = (np.asarray(a, float).reshape(-1) for a in (val, ref, cond))
    return float(np.max(np.abs(val - ref) / (EPS * cond + TINY)))
