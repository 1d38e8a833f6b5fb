"""The reverse pass of the swing legs' PD torques (qc_sensitivity_swing_batch) restated on the CPU (tests/test_sensitivity_swing_cpu.py,
tests/test_gpu_sensitivity_swing.py), written from the model's equations - include/qc_balance.h, oracle/tick_restatement.py - and not
from the kernel.

One swing leg's forward chain and reverse pass are written ONCE over an arithmetic (tests/leg_plant_adjoint_restatement.py: `_Float`,
Python floats and libm; `_Mp`, 50-digit values with condition sums) and evaluated twice:
  swing_adjoint_np   plain float64, the IK end by the identity the kernel uses, p_b_bar = J(q_ref)^-T q_ref_bar
  swing_adjoint_mp   50 digits on the exact double inputs, the IK end by the derivative of legInverseKinematics AS WRITTEN - the
                     atan2 / sqrt chain of leg_plant_adjoint_restatement._ik, reversed operation by operation - and, per output
                     entry, the CONDITION SUM (that module's rules: a + b -> c_a + c_b, a * b -> c_a c_b, a / b -> c_a c_b / b^2,
                     a function value enters with its own magnitude)
(ik="chain" / ik="jacobian" selects the IK end in either arithmetic.)

Per swing leg: p_b = Rwb^T pos - x (sic), v_b = Rwb^T vel, q_ref = IK(p_b), qd = J(q_ref)^-1 v_b, e = q_ref - q + 2 pi k (the wrapped
error; k from the double evaluation of the reference's two wraps), tau_raw = kp e + kd (qd - qdot) + kff; m_c = not (tau_raw_c <
tau_min) and not (tau_raw_c > tau_max), s = m o joint_tau_bar;
  joint_q_bar = -kp s (+ in), joint_qdot_bar = -kd s, gain_bar = (s e, s (qd - qdot), s), g = J^-T (kd s),
  q_ref_bar = kp s - (sum_r g_r H_r) qd, p_b_bar = (dIK / dp)^T q_ref_bar, swing_pos_bar = Rwb p_b_bar, swing_vel_bar = Rwb g,
  Rwb_bar[r][i] += pos_r p_b_bar_i + vel_r g_i, x_bar -= p_b_bar.
A stance leg's rows are zero (+ in).  FLAGS: bit l - swing leg l's knee cosine d >= 1 or < -1, y^2 + z^2 - l1^2 < 0, a target that is
not finite, or det J(q_ref) outside [DET_LO, DET_HI]; the leg's rows and the robot's Rwb_bar and x_bar are then NaN."""
from __future__ import annotations

import math

import mpmath as mp
import numpy as np

from oracle import tick_restatement as TR
from tests import leg_plant_adjoint_restatement as LA
from tests.device_math_reference import DEFAULT_KIN, DPS, EPS, mpf
from tests.leg_plant_adjoint_restatement import Cs, _Float, _ik, _ik_reverse, _in_band, _Leg, _Mp, _mtv, _mv

PER_LEG = ("swing_pos_bar", "swing_vel_bar", "joint_q_bar", "joint_qdot_bar", "gain_bar")
PER_ROBOT = ("Rwb_bar", "x_bar")
OUTPUTS = PER_LEG + PER_ROBOT
SIZES = {"swing_pos_bar": (4, 3), "swing_vel_bar": (4, 3), "joint_q_bar": (4, 3), "joint_qdot_bar": (4, 3), "gain_bar": (4, 9), "Rwb_bar": (9,), "x_bar": (3,)}
INS = ("joint_q_bar_in", "Rwb_bar_in", "x_bar_in")
# the library's default kinematics (qc_default_kinematics; mit_cheetah_config.yaml:50-53, balance_control/torque_min, torque_max)
KP, KD, KFF = (40.0, 40.0, 50.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
TAU_MIN, TAU_MAX = -20.0, 20.0
# C_SWING: the worst |swing_adjoint_np - swing_adjoint_mp| / (EPS x condition sum) per output over the in-reach pool, as
# tests/test_sensitivity_swing_cpu.py measures it, rounded up to one decimal with a little headroom; that test asserts the measurement
# stays below, tests/test_gpu_sensitivity_swing.py derives the device's bar (4 C_SWING) from it.  Never measured on the device.
# Measured over the first 65 robots of the pool: 0.0032, 0.712, 0.978, 0 (kd = 1: exact), 1.081, 0.0011, 0.0006 - the outputs behind
# J^-T carry condition sums that compound through the cofactors, so their figures are small.
C_SWING = {"swing_pos_bar": 0.1, "swing_vel_bar": 0.8, "joint_q_bar": 1.0, "joint_qdot_bar": 0.1, "gain_bar": 1.2, "Rwb_bar": 0.1, "x_bar": 0.1}
# C_SWING_ODD: the same measurement at device_math_reference.ODD_KIN over the first 65 robots of model_pool(ODD_KIN) - clamped on both sides in
# every joint, torques within |kff| of a limit among them: 0.0021, 1.555, 0.985, 0 (one product, rounded once in either arithmetic),
# 1.163, 0.0005, 0.0003 (tests/test_sensitivity_swing_cpu.py::test_float64_against_50_digits_at_the_odd_model prints and asserts them).  Never
# measured on the device.
C_SWING_ODD = {"swing_pos_bar": 0.1, "swing_vel_bar": 1.7, "joint_q_bar": 1.0, "joint_qdot_bar": 0.1, "gain_bar": 1.2, "Rwb_bar": 0.1, "x_bar": 0.1}
C_SWING_OF = {"default": C_SWING, "odd": C_SWING_ODD}
TWO_PI = 2.0 * math.pi


def _wrap_turns(qr, q):
    """k with wrapPI(wrap2PI(qr) - wrap2PI(q)) = qr - q + 2 pi k, from the reference's two wraps in double"""
    e = TR.normalize_angle_PI(TR.normalize_angle_2PI(qr) - TR.normalize_angle_2PI(q))
    return int(round((e - (qr - q)) / TWO_PI))


def _two_pi(A, k):
    return Cs(2 * mp.pi * k) if A is _Mp else TWO_PI * k


def _swing_leg(A, leg, R, x, pos, vel, q, qdot, tb, ik, kp=None, kd=None, kff=None, tau_min=None, tau_max=None, kin=DEFAULT_KIN):
    """One swing leg in arithmetic A on flat float inputs.  Gains and limits left out are the model's (at the default model: KP, KD,
    KFF, TAU_MIN, TAU_MAX).  Returns (dict name -> list of A-values or None if flagged, flagged, tau_raw as floats or None)."""
    kp, kd, kff = (kin.jc_kp if kp is None else kp), (kin.jc_kd if kd is None else kd), (kin.jc_kff if kff is None else kff)
    tau_min, tau_max = (kin.tau_min if tau_min is None else tau_min), (kin.tau_max if tau_max is None else tau_max)
    if not all(math.isfinite(v) for v in list(R) + list(x) + list(pos) + list(vel)):
        return None, True, None
    c = A.const
    Rm, posA, velA = [c(v) for v in R], [c(v) for v in pos], [c(v) for v in vel]
    rp, vb = _mtv(Rm, posA), _mtv(Rm, velA)
    pb = [rp[k] - c(x[k]) for k in range(3)]
    qr, dv, tape = _ik(A, leg, pb, kin)
    if qr is None or not dv < 1.0:  # d >= 1: clamped, no slope; d < -1: NaN
        return None, True, None
    y, z, l1 = tape[1], tape[2], tape[6]
    if A.val(y * y + z * z - l1 * l1) < 0.0:
        return None, True, None
    L = _Leg(A, leg, qr, kin)
    if not _in_band(A.val(L.det), L.det_lo):
        return None, True, None
    qd = L.solve(vb)
    kpA, kdA, kffA = [c(v) for v in kp], [c(v) for v in kd], [c(v) for v in kff]
    e = [qr[k] - c(q[k]) + _two_pi(A, _wrap_turns(A.val(qr[k]), q[k])) if _wrap_turns(A.val(qr[k]), q[k]) else qr[k] - c(q[k]) for k in range(3)]
    dq = [qd[k] - c(qdot[k]) for k in range(3)]
    raw = [A.val(kpA[k] * e[k] + kdA[k] * dq[k] + kffA[k]) for k in range(3)]
    zero = c(0.0)
    s = [c(tb[k]) if (not raw[k] < tau_min and not raw[k] > tau_max) else zero for k in range(3)]
    ks, ps = [kdA[k] * s[k] for k in range(3)], [kpA[k] * s[k] for k in range(3)]
    g = L.solve_t(ks)
    hq = L.hessian_apply(g, qd)
    qrb = [ps[k] - hq[k] for k in range(3)]
    pbb = _ik_reverse(A, tape, qrb) if ik == "chain" else L.solve_t(qrb)
    out = {"swing_pos_bar": _mv(Rm, pbb), "swing_vel_bar": _mv(Rm, g), "joint_q_bar": [-v for v in ps], "joint_qdot_bar": [-v for v in ks],
           "gain_bar": [s[k] * e[k] for k in range(3)] + [s[k] * dq[k] for k in range(3)] + list(s),
           "Rwb_bar": [posA[r] * pbb[i] + velA[r] * g[i] for r in range(3) for i in range(3)], "x_bar": [-v for v in pbb]}
    return out, False, raw


def _swing_adjoint(A, b, swing, tau_bar, ins, ik, kin=DEFAULT_KIN):
    """The batch in arithmetic A.  b: dict of float arrays (Rwb [n,9], x [n,3], joint_q, joint_qdot, swing_pos, swing_vel [n,12]); swing:
    [n,4] bool; tau_bar [n,12]; ins: dict of the optional `_in` arrays.  Returns (values, condition sums or None, flags, tau_raw)."""
    n = b["x"].shape[0]
    arr = lambda k, m: np.asarray(b[k], np.float64).reshape(n, *m)
    R, x = arr("Rwb", (9,)), arr("x", (3,))
    q, qdot, pos, vel = (arr(k, (4, 3)) for k in ("joint_q", "joint_qdot", "swing_pos", "swing_vel"))
    tb = np.asarray(tau_bar, np.float64).reshape(n, 4, 3)
    val = {k: np.zeros((n,) + SIZES[k]) for k in OUTPUTS}
    cond = {k: np.zeros((n,) + SIZES[k]) for k in OUTPUTS} if A is _Mp else None
    given = {k: (None if ins.get(k + "_in") is None else np.asarray(ins[k + "_in"], np.float64).reshape(val[k].shape)) for k in ("joint_q_bar", "Rwb_bar", "x_bar")}
    flags = np.zeros(n, np.int32)
    raw = np.full((n, 4, 3), np.nan)

    def put(k, at, acc):
        """the sums of one row, formed in A and rounded once"""
        val[k][at] = [float(v.v) if A is _Mp else float(v) for v in acc]
        if cond is not None:
            cond[k][at] = [v.c for v in acc]

    for i in range(n):
        start = lambda k, at: [A.const(v) for v in (given[k][at] if given.get(k) is not None else np.zeros(val[k][at].shape))]
        body = {k: start(k, i) for k in PER_ROBOT}
        flagged = False
        for leg in range(4):
            rows = {k: start(k, (i, leg)) for k in PER_LEG}
            if swing[i, leg]:
                out, bad, tr = _swing_leg(A, leg, R[i], x[i], pos[i, leg], vel[i, leg], q[i, leg], qdot[i, leg], tb[i, leg], ik, kin=kin)
                if bad:
                    flags[i] |= 1 << leg
                    flagged = True
                    for k in PER_LEG:
                        val[k][i, leg] = np.nan
                    continue
                raw[i, leg] = tr
                rows = {k: [u + v for u, v in zip(rows[k], out[k])] for k in PER_LEG}
                body = {k: [u + v for u, v in zip(body[k], out[k])] for k in PER_ROBOT}
            for k in PER_LEG:
                put(k, (i, leg), rows[k])
        for k in PER_ROBOT:
            if flagged:
                val[k][i] = np.nan
            else:
                put(k, i, body[k])
    return val, cond, flags, raw


def swing_adjoint_np(b, swing, tau_bar, ik="jacobian", kin=DEFAULT_KIN, **ins):
    """float64: (dict of outputs, flags [n] int32, tau_raw [n,4,3] - NaN for stance and flagged legs)"""
    val, _, flags, raw = _swing_adjoint(_Float, b, np.asarray(swing, bool), tau_bar, ins, ik, kin)
    return val, flags, raw


def swing_adjoint_mp(b, swing, tau_bar, ik="chain", kin=DEFAULT_KIN, **ins):
    """50 digits: (dict of outputs rounded to double, dict of condition sums, flags, tau_raw)"""
    with mp.workdps(DPS):
        return _swing_adjoint(_Mp, b, np.asarray(swing, bool), tau_bar, ins, ik, kin)


# ------------------------------------------------------------------ the forward pass, from the oracle's own functions
def swing_torque(leg, R, x, pos, vel, q, qdot):
    """tau_raw of one swing leg as oracle/tick_restatement.py's Commander forms it (:309-314), unclamped"""
    Rm = np.asarray(R, float).reshape(3, 3)
    name = TR.LEGS[leg]
    pos_b = Rm.T @ np.asarray(pos, float) - np.asarray(x, float)
    vel_b = Rm.T @ np.asarray(vel, float)
    q_ref = TR.leg_inverse_kinematics(name, pos_b)
    qdot_ref = TR.leg_jacobian_inverse(name, q_ref) @ vel_b
    return TR.JointController().control({name: (q_ref, qdot_ref)}, {name: (np.asarray(q, float), np.asarray(qdot, float))})[name]


# ------------------------------------------------------------------ the pools, committed seeds
POOL = 257
PATTERNS = ((0, 0, 0, 0), (1, 0, 0, 1), (0, 1, 1, 0), (1, 1, 1, 0), (1, 1, 1, 1))  # stance bytes: all-swing, the two trot diagonals, one swing leg, all-stance
HOME = (0.0, 0.8, -1.6)


def _rotation(rng):
    """a rotation by up to ~0.5 rad about a random axis, orthonormal to rounding"""
    w = rng.uniform(-0.3, 0.3, 3)
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + (math.sin(th) / th) * K + ((1.0 - math.cos(th)) / th ** 2) * (K @ K)


def masks(n, seed=5):
    """[n,4] stance bytes: the five patterns in turn, then a per-robot mix"""
    rng = np.random.default_rng(seed)
    m = np.array([PATTERNS[i % len(PATTERNS)] for i in range(n)], np.uint8)
    mix = np.arange(n) % 2 == 1
    m[mix] = rng.integers(0, 2, (int(mix.sum()), 4), dtype=np.uint8)
    return m


def pool(n=POOL, seed=11, saturate=False, kin=DEFAULT_KIN, near_limit=False):
    """n robots whose four swing references are all inside reach: q_ref = HOME + U(-0.3, 0.3)^3, the target FK(q_ref) moved to the
    world frame the way the tick reads it back (pos = Rwb (p_b + x)), |q_ref - q| < 0.15 rad, |qdot| < 0.5 rad/s, |vel| < 0.1 m/s:
    kp |e| < 7.5 and kd |qd - qdot| stays below ~3, so every torque is strictly inside +-20 and no wrap is crossed.  saturate=True
    moves q of every third leg by +-0.8 rad in one joint: that torque is clamped (kp 0.65 - 3 > 20).  The targets are FK(q_ref) of
    `kin`, so the pool is rebuilt in reach under any model (the figures above are the default model's).  saturate="every joint"
    does the same with the joint moved taken in turn, so that every joint is clamped on both sides.  near_limit=True then moves one
    joint of every leg of every robot i = 5 mod 8 so that its raw torque (the float64 restatement's, the model's gains) lands half a
    |kff_c| beyond a limit: clamped with kff, passing without it - and, on alternate legs, inside it by as much.  A model with kff =
    0 has no such point (refused)."""
    rng = np.random.default_rng(seed)
    b = {"Rwb": np.zeros((n, 9)), "x": rng.uniform(-0.2, 0.2, (n, 3)), "joint_q": np.zeros((n, 12)), "joint_qdot": rng.uniform(-0.5, 0.5, (n, 12)),
         "swing_pos": np.zeros((n, 12)), "swing_vel": rng.uniform(-0.1, 0.1, (n, 12))}
    for i in range(n):
        R = np.eye(3) if i == 0 else _rotation(rng)
        b["Rwb"][i] = R.reshape(9)
        for leg in range(4):
            q_ref = np.asarray(HOME) + rng.uniform(-0.3, 0.3, 3)
            p_b = LA.LR.fk(leg, q_ref, kin)
            b["swing_pos"][i, 3 * leg:3 * leg + 3] = R @ (p_b + b["x"][i])
            qq = q_ref + rng.uniform(-0.15, 0.15, 3)
            if saturate and (4 * i + leg) % 3 == 0:
                # ((4 i + leg) % 3 == 0 makes (i + leg) % 3 == 0: saturate=True always moves joint 0; "every joint" takes them in turn)
                qq[(i + 2 * leg) % 3 if saturate == "every joint" else (i + leg) % 3] += 0.8 if i % 2 else -0.8
            b["joint_q"][i, 3 * leg:3 * leg + 3] = qq
    if near_limit:
        assert all(v != 0.0 for v in kin.jc_kff)
        for i, leg in ((i, leg) for i in range(5, n, 8) for leg in range(4)):
            c, sl = (i // 8 + leg) % 3, slice(3 * leg, 3 * leg + 3)
            _, bad, raw = _swing_leg(_Float, leg, b["Rwb"][i], b["x"][i], b["swing_pos"][i, sl], b["swing_vel"][i, sl], b["joint_q"][i, sl],
                                     b["joint_qdot"][i, sl], (1.0, 1.0, 1.0), "jacobian", kin=kin)
            assert not bad
            kff = kin.jc_kff[c]
            lim = kin.tau_max if kff > 0.0 else kin.tau_min  # the limit kff pushes towards
            target = lim + 0.5 * kff if leg % 2 == 0 else lim - 0.5 * kff  # beyond it by |kff| / 2, or inside it by as much
            b["joint_q"][i, 3 * leg + c] += (raw[c] - target) / kin.jc_kp[c]  # tau_raw_c falls by kp_c per radian of q_c
    return b


def model_pool(kin, n=POOL):
    """The pool of the 50-digit comparisons under `kin`: the default model's is pool() as it always was (unclamped); any other model's
    is clamped on both sides in every joint and has torques within |kff| of a limit."""
    return pool(n) if kin.name == "default" else pool(n, kin=kin, saturate="every joint", near_limit=True)


def cotangent(n, seed=23):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 12))


def accumulators(n, seed=29):
    rng = np.random.default_rng(seed)
    return {"joint_q_bar_in": rng.uniform(-1.0, 1.0, (n, 4, 3)), "Rwb_bar_in": rng.uniform(-1.0, 1.0, (n, 9)), "x_bar_in": rng.uniform(-1.0, 1.0, (n, 3))}


FLAGGED = ("stretched", "inside", "nonfinite", "folded")


def flagged_pool(kin=DEFAULT_KIN):
    """Four robots, all legs swinging, leg k of robot k constructed outside the smooth domain: stretched (a target 1 m below the hip: d
    > 1, clamped), inside the hip roll's cylinder (the target on the hip axis: y^2 + z^2 < l1^2), a non-finite target, and inside the
    inner reach limit (the target 1 cm from the hip-roll offset point: d < -1).  Returns (b, expected flags)."""
    b = pool(4, seed=31, kin=kin)
    R = b["Rwb"].reshape(4, 3, 3)
    place = lambda i, leg, p_b: b["swing_pos"][i].__setitem__(slice(3 * leg, 3 * leg + 3), R[i] @ (np.asarray(p_b) + b["x"][i]))
    place(0, 0, kin.hip[0] + np.array([0.0, 0.0, -1.0]))
    place(1, 1, kin.hip[1] + np.array([0.1, 0.0, -0.01]))
    b["swing_pos"][2, 6] = np.inf
    place(3, 3, kin.hip[3] + np.array([0.0, float(kin.links[3][0]), -0.01]))
    return b, np.array([1, 2, 4, 8], np.int32)


# ------------------------------------------------------------------ the closed loop through a trot
ROLLOUT_N, ROLLOUT_STEPS, ROLLOUT_H = 65, 3, 1e-4
ROLLOUT_DIRECTIONS = ("joint_q", "x", "swing_pos")
STATE = LA.INPUTS[:-1]
LIFT = 0.02


def trot_start(n=ROLLOUT_N, kin=DEFAULT_KIN):
    """leg_plant_adjoint_restatement.stand_start's generic standing placement on a trot mask - the two diagonals in turn -, the swing
    references HELD: every foot's world position at the start raised by LIFT, at rest.  The swing legs' errors stay below 0.2 rad, so
    their torques stay inside the limits."""
    b = LA.stand_start(n)
    b["stance"] = np.ascontiguousarray(np.array([PATTERNS[1 + i % 2] for i in range(n)], np.uint8))
    R = b["Rwb"].reshape(n, 3, 3)
    pos = np.zeros((n, 12))
    # (the tick reads the reference back as Rwb^T pos - x, sic: the held point is placed so that THAT lands LIFT above the foot)
    for i in range(n):
        for leg in range(4):
            p_b = LA.LR.fk(leg, b["joint_q"][i, 3 * leg:3 * leg + 3], kin) + R[i].T @ np.array([0.0, 0.0, LIFT])
            pos[i, 3 * leg:3 * leg + 3] = R[i] @ (p_b + b["x"][i])
    b["swing_pos"], b["swing_vel"] = np.ascontiguousarray(pos), np.zeros((n, 12))
    return b


def rollout_case():
    """(the start, the loss's coefficients c on the six final state arrays, the committed directions v in joint_q, x and swing_pos)"""
    b = trot_start()
    rng = np.random.default_rng(0x5E1D6)
    c = {k: rng.normal(0.0, 1.0, b[k].shape) for k in STATE}
    v = {k: rng.normal(0.0, 1.0, b[k].shape) for k in ROLLOUT_DIRECTIONS}
    return b, c, v


def cpu_rollout(P, b, steps):
    """The closed loop on the CPU: the C oracle's tick with swing references then leg_plant_step_np on the held mask, `steps` times.
    Returns (final state, per step (status, the certificate's working set of the oracle's forces, the torques' clamp mask, the plant's
    flags))."""
    from oracle import c_oracle
    from tests import kkt_certificate_restatement as KR

    lo, hi = LA.tau_limits()
    s = {k: np.array(b[k], np.float64) for k in STATE}
    mask = np.asarray(b["stance"]) != 0
    rec = []
    for _ in range(steps):
        bb = dict(b, **s)
        t = c_oracle.tick_swing_batch(P, bb)
        feet = c_oracle.tick_batch(P, bb)["feet"]
        active = KR.certificate(P, dict({k: v for k, v in bb.items() if k not in ("joint_qdot", "swing_pos", "swing_vel")}, feet=feet), t["grf_body"])["active"]
        tau = t["joint_tau"]
        o = LA.LR.leg_plant_step_np(P["mass"], P["Ib"], *(s[k] for k in STATE), tau, mask, LA.STAND_INERTIA, LA.DT)
        rec.append((t["status"].copy(), active.copy(), (tau <= lo) | (tau >= hi), o["flags"].copy()))
        s = {k: o[k] for k in STATE}
    return s, rec


def cpu_rollout_kept(P):
    """fd_support's keep rule on the CPU loop alone, on rollout_case: solved and unflagged at every step of every point, the working
    set and the clamp mask of every step those of the base point - at +-h, +-2h along the committed directions.  [ROLLOUT_N] bool."""
    b, _, v = rollout_case()
    _, r0 = cpu_rollout(P, b, ROLLOUT_STEPS)
    keep = np.ones(ROLLOUT_N, bool)
    for st, _, _, fl in r0:
        keep &= (st == 0) & (fl == 0)
    for k in (-2, -1, 1, 2):
        moved = dict(b, **{name: np.ascontiguousarray(b[name] + k * ROLLOUT_H * v[name]) for name in v})
        _, r = cpu_rollout(P, moved, ROLLOUT_STEPS)
        for (st, a, cl, fl), (_, a0, cl0, _) in zip(r, r0):
            keep &= (st == 0) & (fl == 0) & (a == a0).all(axis=1) & (cl == cl0).all(axis=1)
    return keep
