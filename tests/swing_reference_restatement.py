"""The swing references (qc_swing_reference_batch) and their reverse pass (qc_swing_reference_adjoint_batch) restated on the CPU
(tests/test_swing_reference_cpu.py, tests/test_gpu_swing_reference.py), written from the model's equations - include/qc_balance.h,
oracle/tick_restatement.py - and not from the kernels.

One robot's forward step and reverse pass are written ONCE over an arithmetic (tests/leg_plant_adjoint_restatement.py: `_Float`, Python
floats and libm; `_Mp`, 50-digit values with condition sums - a + b -> c_a + c_b, a * b -> c_a c_b, a / b -> c_a c_b / b^2, a function
value enters with its own magnitude) and evaluated twice: reference_np / reference_adjoint_np in float64, reference_mp /
reference_adjoint_mp at 50 digits on the exact double inputs with, per output entry, the condition sum.

What is DECIDED is decided in double in both arithmetics, as the kernels decide it: the advanced phase (fmod), the contact mask (the
phase rule with its 1e-12 slack) and the plan decision.  The trajectory time t = clamp(slope phase + y_int, 0, 1) takes the manager's
double slope and intercept; the 50-digit pass evaluates it exactly (traj_time).

FORWARD  clock (gait_dt), mask, plan (stance -> swing edge, or any swinging leg on the first call: p_start = Rwb FK(q) + x, p_final =
         the foothold; any replan clears every other leg's trajectory), track (swing leg with a trajectory: the sextic at the leg's
         phase; every other leg: zeros).
REVERSE  per leg, with (h, h') the basis at t if the leg swings and has a trajectory after the call, else zero:
           a_r = (h0 + h2 / 2) pos_bar_r + (h0' + h2' / 2) vel_bar_r, c_r with h1 (r = 0, 1); a_2 = h0 pos_bar_2 + h0' vel_bar_2, c_2 with h1
           A = a + p_start_next_bar, C = c + p_final_next_bar
           not replanned: p_start_bar = A, p_final_bar = C
           replanned: p_start_bar = p_final_bar = 0, C_2 := 0, p = FK(q), r = Rwb p, half = t_stance / 2, lip = sqrt(x_z / 9.81) / 2:
             x_bar += A + C, x_bar[2] += 0.25 / (9.81 sqrt(x_z / 9.81)) <C, xdot>, xdot_bar += (half + k + lip) C, xdot_d_bar -= k C,
             w_bar += half (r x C), r_bar = A + half (C x w), Rwb_bar += r_bar p^T + C hip^T, joint_q_bar_l += J^T Rwb^T r_bar
FLAGS    bit l: leg l replanned and x_z not finite and > 0; the robot's rows are NaN."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import mpmath as mp
import numpy as np

from oracle import tick_restatement as TR
from tests import device_math_reference as DMR
from tests.device_math_reference import DEFAULT_KIN, DPS, EPS, ODD_KIN
from tests.leg_plant_adjoint_restatement import Cs, _Float, _Leg, _Mp, _cr, _mtv, _mv

G = 9.81
OUTPUTS = ("Rwb_bar", "x_bar", "xdot_bar", "w_bar", "xdot_d_bar", "joint_q_bar", "p_start_bar", "p_final_bar")
SIZES = {"Rwb_bar": 9, "x_bar": 3, "xdot_bar": 3, "w_bar": 3, "xdot_d_bar": 3, "joint_q_bar": 12, "p_start_bar": 12, "p_final_bar": 12}
INS = ("Rwb_bar_in", "x_bar_in", "xdot_bar_in", "w_bar_in", "joint_q_bar_in")
COTANGENTS = ("swing_pos", "swing_vel", "p_start", "p_final")
# C_REF: the worst |reference_adjoint_np - reference_adjoint_mp| / (EPS x condition sum) per output over pool(ODD_MODEL, 257), as
# tests/test_swing_reference_cpu.py measures it (printed there: 0.964, 1.018, 0.713, 0.526, 0.736, 2.164, 1.126, 0.890), rounded up to one
# decimal with a little headroom; that test asserts the measurement stays below, tests/test_gpu_swing_reference.py derives the device's
# bar (4 C_REF) from it.  C_FWD: the same for the forward outputs swing_pos, swing_vel, p_start, p_final (2.275, 1.803, 1.005, 1.335).
# The rounding of the trajectory time t in double is in these figures (traj_time).  Never measured on the device.
C_REF = {"Rwb_bar": 1.0, "x_bar": 1.1, "xdot_bar": 0.8, "w_bar": 0.6, "xdot_d_bar": 0.8, "joint_q_bar": 2.3, "p_start_bar": 1.2, "p_final_bar": 1.0}
C_FWD = {"swing_pos": 2.4, "swing_vel": 1.9, "p_start": 1.1, "p_final": 1.4}


def handle_basis():
    """The sextic basis AS A HANDLE HOLDS IT, [7, 3] doubles: qc_create inverts the 7x7 system of trajectory.cpp:256-277 by Gauss-Jordan
    elimination with partial pivoting in double (csrc/qc_host.hpp, sextic_basis), and twelve of its 21 entries come out up to 4e-12 off the
    integers the exact inverse has.  They are constants of the model - exact double INPUTS of both arithmetics here -, so the same
    elimination is made here, operation by operation in IEEE double; tests/test_swing_reference_cpu.py holds it within 1e-9 of
    device_math_reference.sextic_basis_mp."""
    A = [[1.0, 0, 0, 0, 0, 0, 0], [1.0] * 7, [0.5 ** k for k in range(7)], [0, 1.0, 0, 0, 0, 0, 0], [0, 1.0, 2, 3, 4, 5, 6], [0, 0, 2.0, 0, 0, 0, 0],
         [0, 0, 2.0, 6, 12, 20, 30]]
    Mx = [[float(v) for v in A[i]] + [1.0 if i == k else 0.0 for k in range(3)] for i in range(7)]
    for c in range(7):
        p = c
        for r in range(c + 1, 7):
            if abs(Mx[r][c]) > abs(Mx[p][c]):
                p = r
        Mx[c], Mx[p] = Mx[p], Mx[c]
        piv = Mx[c][c]
        Mx[c] = [v / piv for v in Mx[c]]
        for r in range(7):
            if r != c:
                m = Mx[r][c]
                Mx[r] = [Mx[r][j] - m * Mx[c][j] for j in range(10)]
    return np.array([[Mx[j][7 + k] for k in range(3)] for j in range(7)])


@dataclass(frozen=True)
class Model:
    """The constants of the swing reference generator as a handle holds them: the kinematic model, the planner's hips, gain and
    swing height (set_kinematics) and the gait's periods (set_gait)."""
    name: str
    kin: object
    planner_hip: np.ndarray
    planner_k: float
    swing_height: float
    t_swing: float
    t_stance: float
    basis: np.ndarray = field(default_factory=handle_basis)

    @property
    def duty(self):
        return self.t_stance / (self.t_swing + self.t_stance)

    def handle_arguments(self):
        return dict(self.kin.handle_arguments(), planner_hip=self.planner_hip.reshape(12), planner_k=self.planner_k, swing_height=self.swing_height)


DEFAULT_MODEL = Model("default", DEFAULT_KIN, np.array([TR.HIP_MAP[l] for l in TR.LEGS]), TR.PLANNER_K, 0.08, 0.18, 0.8)
# a second model, committed as literal numbers: the odd kinematics, planner hips that differ from leg to leg and have a z, another gain,
# height and gait (duty 0.6)
ODD_MODEL = Model("odd", ODD_KIN, np.array([[-0.21, 0.113, 0.012], [0.183, 0.141, -0.02], [-0.17, -0.135, 0.03], [0.224, -0.119, -0.011]]),
                  0.037, 0.065, 0.24, 0.36)
MODELS = {"default": DEFAULT_MODEL, "odd": ODD_MODEL}


# ------------------------------------------------------------------ what is decided in double
def advance(phase, dt, M):
    """GaitScheduler::update on four phases"""
    v = np.asarray(phase, float) + 1.0 / (M.t_swing + M.t_stance) * dt
    return np.array([math.fmod(p, 1.0) if math.isfinite(p) else float("nan") for p in v])


def in_stance(ph, duty):
    almost = lambda a, b: abs(a - b) < 1.0e-12
    return (ph > 0.0 or almost(ph, 0.0)) and (ph < duty or almost(ph, duty))


def decide(leg_state, has_traj, mask):
    """(plan [4] bool, has_traj after [4] int) from the record before the call and the contact mask (True = stance)"""
    first = leg_state[0] < 0
    plan = [(not mask[l]) and (first or leg_state[l] == 1) for l in range(4)]
    has = [int(plan[l]) if any(plan) else int(has_traj[l]) for l in range(4)]
    return plan, has


def traj_time(ph, M, A=_Float):
    """t = clamp(slope phase + y_int, 0, 1) from the manager's DOUBLE slope and intercept (trajectory.cpp:303-305): in float64 rounded
    as written; at 50 digits exactly - t then enters with its own magnitude, as a function value does, so what the rounding of
    slope phase + y_int (a sum of terms ~5 and ~-4 for a t in [0, 1]) does to the result is part of what C_REF / C_FWD measure."""
    duty = M.t_stance / (M.t_swing + M.t_stance)
    slope = 1.0 / (1.0 - duty)
    yint = 1.0 - slope
    if A is _Mp and not math.isnan(ph):
        u = DMR.mpf(slope) * DMR.mpf(ph) + DMR.mpf(yint)
        return Cs(min(max(u, mp.mpf(0)), mp.mpf(1)))
    u = slope * ph + yint
    return A.const(u if math.isnan(u) else min(max(u, 0.0), 1.0))


def _basis(A, tt, M):
    """h_k(t), h_k'(t), k = start, final, centre, in arithmetic A from the model's basis (exact doubles) and t = traj_time(., ., A)"""
    c = A.const
    h, dh = [c(0.0)] * 3, [c(0.0)] * 3
    tp, tpm = c(1.0), None
    for j in range(7):
        for k in range(3):
            b = c(M.basis[j, k])
            h[k] = h[k] + b * tp
            if tpm is not None:
                dh[k] = dh[k] + c(float(j)) * b * tpm
        tpm, tp = tp, tp * tt
    return h, dh


def _sqrt(A, v):
    return A.sqrt(v) if A.val(v) >= 0.0 else A.const(float("nan"))


def _foothold(A, M, leg, R, x, xdot, w, xdd, r):
    c = A.const
    hip = [c(v) for v in M.planner_hip[leg]]
    pt = [a + b for a, b in zip(_mv(R, hip), x)]
    tv = _cr(w, r)
    half, k = c(0.5) * c(M.t_stance), c(M.planner_k)
    lip = c(0.5) * _sqrt(A, x[2] / c(G))
    fh = [pt[i] + (half * xdot[i] + k * (xdot[i] - xdd[i])) + half * tv[i] + lip * xdot[i] for i in range(3)]
    fh[2] = c(0.0)
    return fh


def _out(A, vals):
    return [float(v.v) if A is _Mp else float(v) for v in vals], ([v.c for v in vals] if A is _Mp else None)


# ------------------------------------------------------------------ one robot, forward
def _forward_one(A, M, b, rec, mask, phase):
    """b: flat float arrays Rwb, x, xdot, w, xdot_d, joint_q; rec: (leg_state, has_traj, p_start [12], p_final [12]) before the call;
    mask [4] (True = stance), phase [4]: as decided.  Returns (dict of A-value lists: swing_pos, swing_vel, p_start, p_final; plan; has)."""
    c = A.const
    vec = lambda k: [c(v) for v in np.asarray(b[k], float).reshape(-1)]
    R, x, xdot, w, xdd, q = vec("Rwb"), vec("x"), vec("xdot"), vec("w"), vec("xdot_d"), vec("joint_q")
    plan, has = decide(rec[0], rec[1], mask)
    ps, pf = [c(v) for v in rec[2]], [c(v) for v in rec[3]]
    pos, vel = [c(0.0)] * 12, [c(0.0)] * 12
    for l in range(4):
        sl = slice(3 * l, 3 * l + 3)
        if plan[l]:
            r = _mv(R, _Leg(A, l, q[sl], M.kin).p)
            ps[sl] = [r[i] + x[i] for i in range(3)]
            pf[sl] = _foothold(A, M, l, R, x, xdot, w, xdd, r)
        if not mask[l] and has[l]:
            h, dh = _basis(A, traj_time(phase[l], M, A), M)
            p0, p1 = ps[sl], pf[sl]
            pc = [c(0.5) * (p0[0] + p1[0]), c(0.5) * (p0[1] + p1[1]), c(M.swing_height)]
            pos[sl] = [h[0] * p0[i] + h[1] * p1[i] + h[2] * pc[i] for i in range(3)]
            vel[sl] = [dh[0] * p0[i] + dh[1] * p1[i] + dh[2] * pc[i] for i in range(3)]
    return {"swing_pos": pos, "swing_vel": vel, "p_start": ps, "p_final": pf}, plan, has


def _forward(A, M, b, state, gait_dt=None):
    """The batch.  b: dict of float arrays plus gait_phase [n,4] and optionally stance [n,4] uint8, gait_duty [n]; state: a
    SWING_STATE-shaped structured array (leg_state, has_traj, p_start, p_final) BEFORE the call.  Returns (values, condition sums or
    None, state after, phases after, planned bits [n] uint8)."""
    n = b["x"].shape[0]
    after = state.copy()
    phases = np.array(b["gait_phase"], float).reshape(n, 4)
    val = {k: np.zeros((n, 12)) for k in ("swing_pos", "swing_vel", "p_start", "p_final")}
    cond = {k: np.zeros((n, 12)) for k in val} if A is _Mp else None
    planned = np.zeros(n, np.uint8)
    for i in range(n):
        if gait_dt is not None:
            phases[i] = advance(phases[i], float(np.asarray(gait_dt).reshape(-1)[i]), M)
        duty = M.duty if b.get("gait_duty") is None else float(b["gait_duty"][i])
        mask = [bool(v) for v in b["stance"][i]] if b.get("stance") is not None else [in_stance(p, duty) for p in phases[i]]
        rec = (state["leg_state"][i], state["has_traj"][i], state["p_start"][i], state["p_final"][i])
        out, plan, has = _forward_one(A, M, {k: b[k][i] for k in ("Rwb", "x", "xdot", "w", "xdot_d", "joint_q")}, rec, mask, phases[i])
        for k in val:
            v, cs = _out(A, out[k])
            val[k][i] = v
            if cond is not None:
                cond[k][i] = cs
        after["leg_state"][i] = [int(m) for m in mask]
        after["has_traj"][i] = has
        for l in range(4):
            if plan[l]:
                planned[i] |= 1 << l
                after["p_start"][i, 3 * l:3 * l + 3] = val["p_start"][i, 3 * l:3 * l + 3]
                after["p_final"][i, 3 * l:3 * l + 3] = val["p_final"][i, 3 * l:3 * l + 3]
    return val, cond, after, phases, planned


def reference_np(M, b, state, gait_dt=None):
    val, _, after, phases, planned = _forward(_Float, M, b, state, gait_dt)
    return val, after, phases, planned


def reference_mp(M, b, state, gait_dt=None):
    with mp.workdps(DPS):
        return _forward(_Mp, M, b, state, gait_dt)


# ------------------------------------------------------------------ one robot, reverse
def _adjoint_one(A, M, b, rec, mask, phase, bars, ins):
    c = A.const
    vec = lambda a: [c(v) for v in np.asarray(a, float).reshape(-1)]
    R, x, xdot, w, q = vec(b["Rwb"]), vec(b["x"]), vec(b["xdot"]), vec(b["w"]), vec(b["joint_q"])
    bar = lambda k: vec(np.zeros(12) if bars.get(k) is None else bars[k])
    pos_b, vel_b, sA, sC = bar("swing_pos"), bar("swing_vel"), bar("p_start"), bar("p_final")
    acc = {k: vec(np.zeros(SIZES[k]) if ins.get(k + "_in") is None else ins[k + "_in"]) for k in ("Rwb_bar", "x_bar", "xdot_bar", "w_bar", "joint_q_bar")}
    acc["xdot_d_bar"] = vec(np.zeros(3))
    plan, has = decide(rec[0], rec[1], mask)
    flags = 0
    x2 = float(b["x"][2])
    half, kk, zero = c(0.5) * c(M.t_stance), c(M.planner_k), c(0.0)
    for l in range(4):
        sl = slice(3 * l, 3 * l + 3)
        Al, Cl = sA[sl], sC[sl]
        if not mask[l] and has[l]:
            h, dh = _basis(A, traj_time(phase[l], M, A), M)
            hf = c(0.5)
            for r in range(3):
                m0 = (h[0] + hf * h[2], dh[0] + hf * dh[2], h[1] + hf * h[2], dh[1] + hf * dh[2]) if r < 2 else (h[0], dh[0], h[1], dh[1])
                Al[r] = Al[r] + (m0[0] * pos_b[3 * l + r] + m0[1] * vel_b[3 * l + r])
                Cl[r] = Cl[r] + (m0[2] * pos_b[3 * l + r] + m0[3] * vel_b[3 * l + r])
        if not plan[l]:
            sA[sl], sC[sl] = Al, Cl
            continue
        sA[sl], sC[sl] = [zero] * 3, [zero] * 3
        if not (math.isfinite(x2) and x2 > 0.0):
            flags |= 1 << l
            continue
        Cl = [Cl[0], Cl[1], zero]
        L = _Leg(A, l, q[sl], M.kin)
        p = L.p
        r = _mv(R, p)
        root = A.sqrt(x[2] / c(G))
        lip = c(0.5) * root
        cv = Cl[0] * xdot[0] + Cl[1] * xdot[1] + Cl[2] * xdot[2]
        rxc, cxw = _cr(r, Cl), _cr(Cl, w)
        gain = half + kk + lip
        rbar = [Al[i] + half * cxw[i] for i in range(3)]
        for i in range(3):
            acc["x_bar"][i] = acc["x_bar"][i] + (Al[i] + Cl[i])
            acc["xdot_bar"][i] = acc["xdot_bar"][i] + gain * Cl[i]
            acc["xdot_d_bar"][i] = acc["xdot_d_bar"][i] - kk * Cl[i]
            acc["w_bar"][i] = acc["w_bar"][i] + half * rxc[i]
        acc["x_bar"][2] = acc["x_bar"][2] + (c(0.25) / (c(G) * root)) * cv
        hip = [c(v) for v in M.planner_hip[l]]
        for rr in range(3):
            for i in range(3):
                acc["Rwb_bar"][3 * rr + i] = acc["Rwb_bar"][3 * rr + i] + (rbar[rr] * p[i] + Cl[rr] * hip[i])
        jq = _mtv(L.J, _mtv(R, rbar))
        for i in range(3):
            acc["joint_q_bar"][3 * l + i] = acc["joint_q_bar"][3 * l + i] + jq[i]
    acc["p_start_bar"], acc["p_final_bar"] = sA, sC
    return acc, flags


def _adjoint(A, M, b, state_before, bars, ins):
    """b: the batch with gait_phase AS THE FORWARD CALL LEFT IT; bars: dict over COTANGENTS of [n,12] arrays or None; ins: dict over INS.
    Returns (values, condition sums or None, flags)."""
    n = b["x"].shape[0]
    phases = np.asarray(b["gait_phase"], float).reshape(n, 4)
    val = {k: np.zeros((n, SIZES[k])) for k in OUTPUTS}
    cond = {k: np.zeros((n, SIZES[k])) for k in OUTPUTS} if A is _Mp else None
    flags = np.zeros(n, np.int32)
    row = lambda d, i: {k: (None if v is None else np.asarray(v, float).reshape(n, -1)[i]) for k, v in d.items()}
    for i in range(n):
        duty = M.duty if b.get("gait_duty") is None else float(b["gait_duty"][i])
        mask = [bool(v) for v in b["stance"][i]] if b.get("stance") is not None else [in_stance(p, duty) for p in phases[i]]
        rec = (state_before["leg_state"][i], state_before["has_traj"][i])
        acc, fl = _adjoint_one(A, M, {k: np.asarray(b[k], float)[i] for k in ("Rwb", "x", "xdot", "w", "joint_q")}, rec, mask, phases[i], row(bars, i), row(ins, i))
        flags[i] = fl
        for k in OUTPUTS:
            if fl:
                val[k][i] = np.nan
                continue
            v, cs = _out(A, acc[k])
            val[k][i] = v
            if cond is not None:
                cond[k][i] = cs
    return val, cond, flags


def reference_adjoint_np(M, b, state_before, bars, **ins):
    val, _, flags = _adjoint(_Float, M, b, state_before, bars, ins)
    return val, flags


def reference_adjoint_mp(M, b, state_before, bars, **ins):
    with mp.workdps(DPS):
        return _adjoint(_Mp, M, b, state_before, bars, ins)


# ------------------------------------------------------------------ the pools, committed seeds
STATE_DTYPE = np.dtype([("leg_state", np.int32, 4), ("has_traj", np.int32, 4), ("p_start", np.float64, 12), ("p_final", np.float64, 12)])  # == qc_swing_state
HOME = (0.0, 0.8, -1.6)
KINDS = ("first", "edge1", "edge2", "carried", "cleared", "stance")


def _rotation(rng):
    w = rng.uniform(-0.3, 0.3, 3)
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + (math.sin(th) / th) * K + ((1.0 - math.cos(th)) / th ** 2) * (K @ K)


def pool(M, n=257, seed=41):
    """n robots whose kind is KINDS[i % 6], the phases AFTER the clock's step of GAIT_DT decided per kind (swing phases well inside (duty,
    1), stance phases well inside (0, duty)):
      first    leg_state = -1 everywhere, a trot diagonal (or, every other one, three legs) swinging: every swinging leg is replanned
      edge1    one leg stance -> swing; another leg mid-swing with a trajectory, which the replan CLEARS
      edge2    two legs stance -> swing, the other two in stance
      carried  two legs mid-swing with trajectories, no edge: the records pass through
      cleared  one leg mid-swing WITHOUT a trajectory (cleared earlier), one with: no edge
      stance   all four legs in stance before and after
    Returns (b, state, gait_dt): the batch with gait_phase BEFORE the step, the records before the call, the step [n]."""
    rng = np.random.default_rng(seed)
    duty, period = M.duty, M.t_swing + M.t_stance
    b = {"Rwb": np.zeros((n, 9)), "x": np.c_[rng.uniform(-0.2, 0.2, (n, 2)), rng.uniform(0.2, 0.35, n)], "xdot": rng.uniform(-0.5, 0.5, (n, 3)),
         "w": rng.uniform(-0.5, 0.5, (n, 3)), "xdot_d": rng.uniform(-0.5, 0.5, (n, 3)),
         "joint_q": (np.tile(HOME, (n, 4)) + rng.uniform(-0.3, 0.3, (n, 12)))}
    state = np.zeros(n, STATE_DTYPE)
    state["p_start"], state["p_final"] = rng.uniform(-0.3, 0.3, (n, 12)), rng.uniform(-0.3, 0.3, (n, 12))
    after = np.zeros((n, 4))
    sw = lambda: rng.uniform(duty + 0.05 * (1 - duty), 1.0 - 0.05 * (1 - duty))  # a swing phase, inside the clamp's open interval
    st = lambda: rng.uniform(0.05 * duty, 0.95 * duty)
    for i in range(n):
        b["Rwb"][i] = (np.eye(3) if i == 0 else _rotation(rng)).reshape(9)
        kind = KINDS[i % len(KINDS)]
        legs = rng.permutation(4)
        swing, prev, has = np.zeros(4, bool), np.ones(4, np.int32), np.zeros(4, np.int32)
        if kind == "first":
            swing[[0, 3] if (i // 6) % 3 == 0 else ([1, 2] if (i // 6) % 3 == 1 else [0, 1, 3])] = True
            prev[:] = -1
        elif kind == "edge1":
            swing[legs[:2]] = True
            prev[legs[1]], has[legs[1]] = 0, 1  # legs[0]: the edge; legs[1]: mid-swing, cleared by the replan
        elif kind == "edge2":
            swing[legs[:2]] = True
        elif kind == "carried":
            swing[legs[:2]] = True
            prev[legs[:2]], has[legs[:2]] = 0, 1
        elif kind == "cleared":
            swing[legs[:2]] = True
            prev[legs[:2]] = 0
            has[legs[0]] = 1
        state["leg_state"][i], state["has_traj"][i] = prev, has
        after[i] = [sw() if swing[l] else st() for l in range(4)]
    gait_dt = np.full(n, 0.013 * period)
    b["gait_phase"] = np.mod(after - gait_dt[:, None] / period, 1.0)
    # (the phases AFTER the step are advance(before), decided in double by the code under test: the margins above are 5 % of an interval)
    return b, state, gait_dt


def cotangents(n, seed=43):
    rng = np.random.default_rng(seed)
    return {k: rng.uniform(-1.0, 1.0, (n, 12)) for k in COTANGENTS}


def accumulators(n, seed=47):
    rng = np.random.default_rng(seed)
    return {k: rng.uniform(-1.0, 1.0, (n, SIZES[k[:-3]])) for k in INS}


def worst_ratio(val, ref, cond):
    """max |val - ref| / (EPS cond) over the entries with cond > 0; an entry with cond = 0 must be equal"""
    val, ref, cond = (np.asarray(a, float).reshape(-1) for a in (val, ref, cond))
    ok = cond > 0.0
    assert np.array_equal(val[~ok], ref[~ok]), "an entry with no rounding behind it differs"
    return float(np.max(np.abs(val[ok] - ref[ok]) / (EPS * cond[ok]))) if ok.any() else 0.0
