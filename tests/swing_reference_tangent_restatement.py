"""The forward mode of the swing references (qc_swing_reference_tangent_batch, include/qc_tangent.h) restated on the CPU
(tests/test_swing_reference_tangent_cpu.py, tests/test_gpu_swing_reference_tangent.py), written from the model's equations and not from
the kernel, on top of tests/swing_reference_restatement.py: its models (default / odd), its pool of six kinds (first, edge1, edge2,
carried, cleared, stance), its `decide`, its basis and trajectory time.

One robot's derivative is written ONCE over an arithmetic (tests/leg_plant_adjoint_restatement.py: `_Float`, Python floats and libm;
`_Mp`, 50-digit values with condition sums - a + b -> c_a + c_b, a * b -> c_a c_b, a / b -> c_a c_b / b^2, a function value enters with
its own magnitude) and evaluated twice: reference_tangent_np in float64, reference_tangent_mp at 50 digits on the exact double inputs
with, per output entry, the condition sum: the sum of the magnitudes of the terms added.

HELD, decided in double as the kernels decide it: the contact mask (the phases as the forward call left them) and the plan decision
from the record BEFORE the forward call.  Per direction and leg l, p = FK(q_l), r = Rwb p, half = t_stance / 2, k = planner_k,
lip = sqrt(x_z / 9.81) / 2, hip = planner_hip[l], delta the world-frame left tangent of Rwb:
  replanned      dr = delta x r + Rwb J(q_l) dq_l,  dps = dr + dx,
                 dpf = delta x (Rwb hip) + dx + (half + k + lip) dxdot - k dxdot_d + (0.25 / (9.81 sqrt(x_z / 9.81))) dx_z xdot
                       + half (dw x r + w x dr),  dpf_z := 0
  not replanned  dps = p_start_tan_l, dpf = p_final_tan_l
  track          swing leg with a trajectory after the call: dpos_r = (h0 + m h2) dps_r + (h1 + m h2) dpf_r, dvel_r with h';
                 m = 1/2 for x, y and 0 for z; every other leg: zeros
FLAGS  bit l: leg l replanned and x_z not finite and > 0; every row of the robot is NaN in every direction."""
from __future__ import annotations

import math

import mpmath as mp
import numpy as np

from tests import swing_reference_restatement as RR
from tests.device_math_reference import DPS, EPS  # noqa: F401
from tests.leg_plant_adjoint_restatement import _cr, _Float, _Leg, _Mp, _mv
from tests.swing_tangent_restatement import exp_rotation, skew_times

G = RR.G
TANGENTS = {"Rwb_rot_tan": 3, "x_tan": 3, "xdot_tan": 3, "w_tan": 3, "xdot_d_tan": 3, "joint_q_tan": 12, "p_start_tan": 12, "p_final_tan": 12}
OUTPUTS = ("swing_pos_tan", "swing_vel_tan", "p_start_next_tan", "p_final_next_tan")
# the adjoint's cotangent (RR.COTANGENTS) that pairs with each output, and its output that pairs with each input tangent
COTANGENT_OF = {"swing_pos_tan": "swing_pos", "swing_vel_tan": "swing_vel", "p_start_next_tan": "p_start", "p_final_next_tan": "p_final"}
BAR_OF = {"x_tan": "x_bar", "xdot_tan": "xdot_bar", "w_tan": "w_bar", "xdot_d_tan": "xdot_d_bar", "joint_q_tan": "joint_q_bar",
          "p_start_tan": "p_start_bar", "p_final_tan": "p_final_bar"}
# C_RT: the worst |reference_tangent_np - reference_tangent_mp| / (EPS x condition sum) per output over RR.pool(M, 257) of both models,
# three directions, as tests/test_swing_reference_tangent_cpu.py measures it on the CPU against 50 digits (printed there: default
# 7.039, 21.972, 1.451, 1.295; odd 1.482, 4.883, 1.064, 1.329), the larger of the two models rounded up with a little headroom; that
# test asserts the measurement stays below, tests/test_gpu_swing_reference_tangent.py derives the device's bar (4 C_RT) from it.
# The two references' figures are the rounding of the trajectory time t in double (RR.traj_time: slope phase + y_int, terms of 4.5
# and -4.4, is off by up to 2 EPS): early in a swing - the pool goes down to t = 0.055 - the basis' derivatives go like t^2, so that
# error is 2 x 2 EPS / t = 73 EPS of an entry whose condition sum is a few times its value.  The worst entries are z rows at
# t = 0.059 (default) and t = 0.06 ... 0.17.  Never measured on the device.
C_RT = {"swing_pos_tan": 7.2, "swing_vel_tan": 22.5, "p_start_next_tan": 1.5, "p_final_next_tan": 1.4}
# C_RDOT: the worst gap of the pairing <cotangents, reference_tangent_np's outputs> = <reference_adjoint_np's outputs, tangents>, in EPS
# x the sum of the magnitudes of all terms on both sides, over the same pools the same way.  Measured: 0.640 (default), 0.790 (odd).
C_RDOT = 0.8


def random_tangents(n, K, seed=71):
    """{name: [K, n, m]}: 0.1 rad, 1 cm, 0.1 m/s, 0.1 rad/s, 0.1 m/s, 0.1 rad, 1 cm and 1 cm normal draws"""
    rng = np.random.default_rng(seed)
    scale = {"Rwb_rot_tan": 0.1, "x_tan": 0.01, "xdot_tan": 0.1, "w_tan": 0.1, "xdot_d_tan": 0.1, "joint_q_tan": 0.1, "p_start_tan": 0.01, "p_final_tan": 0.01}
    return {k: rng.normal(0.0, scale[k], (K, n, m)) for k, m in TANGENTS.items()}


def undefined(x2):
    """the LIP square root has no derivative at this x_z"""
    return not (math.isfinite(x2) and x2 > 0.0)


# ------------------------------------------------------------------ one robot, one direction
def _tangent_one(A, M, b, rec, mask, phase, t):
    """b: flat float arrays Rwb, x, xdot, w, joint_q; rec: (leg_state, has_traj) BEFORE the forward call; mask [4] (True = stance),
    phase [4] as the forward call left them; t: flat float arrays over TANGENTS.  Returns (dict over OUTPUTS of A-value lists, flags)."""
    c = A.const
    vec = lambda a: [c(v) for v in np.asarray(a, float).reshape(-1)]
    R, x, xdot, w, q = vec(b["Rwb"]), vec(b["x"]), vec(b["xdot"]), vec(b["w"]), vec(b["joint_q"])
    dl, dx, dv, dw, dvd, dq = (vec(t[k]) for k in ("Rwb_rot_tan", "x_tan", "xdot_tan", "w_tan", "xdot_d_tan", "joint_q_tan"))
    dps, dpf = vec(t["p_start_tan"]), vec(t["p_final_tan"])
    plan, has = RR.decide(rec[0], rec[1], mask)
    flags = sum(1 << l for l in range(4) if plan[l]) if undefined(float(b["x"][2])) else 0
    zero = c(0.0)
    pos, vel = [zero] * 12, [zero] * 12
    if flags:
        return {"swing_pos_tan": pos, "swing_vel_tan": vel, "p_start_next_tan": dps, "p_final_next_tan": dpf}, flags
    half, kk = c(0.5) * c(M.t_stance), c(M.planner_k)
    for l in range(4):
        sl = slice(3 * l, 3 * l + 3)
        if plan[l]:
            L = _Leg(A, l, q[sl], M.kin)
            r = _mv(R, L.p)
            rh = _mv(R, [c(v) for v in M.planner_hip[l]])
            rj = _mv(R, _mv(L.J, dq[sl]))
            cr = _cr(dl, r)
            dr = [cr[i] + rj[i] for i in range(3)]
            root = A.sqrt(x[2] / c(G))
            gain = half + kk + c(0.5) * root
            dz = (c(0.25) / (c(G) * root)) * dx[2]
            ch, dwr, wdr = _cr(dl, rh), _cr(dw, r), _cr(w, dr)
            dps[sl] = [dr[i] + dx[i] for i in range(3)]
            f = [ch[i] + dx[i] + gain * dv[i] - kk * dvd[i] + dz * xdot[i] + half * (dwr[i] + wdr[i]) for i in range(3)]
            f[2] = zero  # the foothold's z is the constant 0
            dpf[sl] = f
        if not mask[l] and has[l]:
            h, dh = RR._basis(A, RR.traj_time(phase[l], M, A), M)
            hf = c(0.5)
            for r_ in range(3):
                m = (h[0] + hf * h[2], h[1] + hf * h[2], dh[0] + hf * dh[2], dh[1] + hf * dh[2]) if r_ < 2 else (h[0], h[1], dh[0], dh[1])
                pos[3 * l + r_] = m[0] * dps[3 * l + r_] + m[1] * dpf[3 * l + r_]
                vel[3 * l + r_] = m[2] * dps[3 * l + r_] + m[3] * dpf[3 * l + r_]
    return {"swing_pos_tan": pos, "swing_vel_tan": vel, "p_start_next_tan": dps, "p_final_next_tan": dpf}, flags


def _tangent(A, M, b, state_before, tans):
    """The batch in arithmetic A.  b: the batch with gait_phase AS THE FORWARD CALL LEFT IT (and optionally stance [n,4], gait_duty [n]);
    state_before: the records before the forward call; tans: dict over TANGENTS of [K, n, m] arrays (a missing one is zero).  Returns
    (dict over OUTPUTS of [K, n, 12] values, condition sums or None, flags [n] int32)."""
    n = b["x"].shape[0]
    K = next(np.asarray(t).shape[0] for t in tans.values() if t is not None)
    t = {k: (np.zeros((K, n, m)) if tans.get(k) is None else np.asarray(tans[k], np.float64).reshape(K, n, m)) for k, m in TANGENTS.items()}
    phases = np.asarray(b["gait_phase"], float).reshape(n, 4)
    val = {k: np.zeros((K, n, 12)) for k in OUTPUTS}
    cond = {k: np.zeros((K, n, 12)) for k in OUTPUTS} if A is _Mp else None
    flags = np.zeros(n, np.int32)
    for i in range(n):
        duty = M.duty if b.get("gait_duty") is None else float(b["gait_duty"][i])
        mask = [bool(v) for v in b["stance"][i]] if b.get("stance") is not None else [RR.in_stance(p, duty) for p in phases[i]]
        rec = (state_before["leg_state"][i], state_before["has_traj"][i])
        bi = {k: np.asarray(b[k], float)[i] for k in ("Rwb", "x", "xdot", "w", "joint_q")}
        for k in range(K):
            out, fl = _tangent_one(A, M, bi, rec, mask, phases[i], {name: t[name][k, i] for name in TANGENTS})
            flags[i] = fl
            for name in OUTPUTS:
                if fl:
                    val[name][k, i] = np.nan
                    continue
                v, cs = RR._out(A, out[name])
                val[name][k, i] = v
                if cond is not None:
                    cond[name][k, i] = cs
    return val, cond, flags


def reference_tangent_np(M, b, state_before, tans):
    """float64: (dict over OUTPUTS of [K, n, 12], flags [n] int32)"""
    val, _, flags = _tangent(_Float, M, b, state_before, tans)
    return val, flags


def reference_tangent_mp(M, b, state_before, tans):
    """50 digits: (values rounded to double, condition sums, flags)"""
    with mp.workdps(DPS):
        return _tangent(_Mp, M, b, state_before, tans)


# ------------------------------------------------------------------ the pool after the clock's step, the pairing, central differences
def pool_after(M, n=257, seed=41):
    """RR.pool(M, n) with the phases as the forward call leaves them: (b with gait_phase advanced, the records BEFORE the call, the
    records after it, the planned bits, the kinds' names per robot)"""
    b, state, gait_dt = RR.pool(M, n, seed)
    _, after, phases, planned = RR.reference_np(M, b, state, gait_dt)
    return dict(b, gait_phase=phases), state, after, planned, [RR.KINDS[i % len(RR.KINDS)] for i in range(n)]


def pairing(bars, outs, tans, adj, Rwb, exact=False):
    """The two sides of <swing_pos_bar, dpos> + <swing_vel_bar, dvel> + <p_start_next_bar, dps'> + <p_final_next_bar, dpf'> = <the
    adjoint's outputs, the input tangents> (Rwb_bar with [delta]x Rwb) per (direction, robot), and the sum of the magnitudes of all
    terms on both sides.  bars: dict over RR.COTANGENTS of [n, 12]; outs: dict over OUTPUTS of [K, n, 12]; tans: [K, n, m] arrays;
    adj: the adjoint's [n, ...] outputs.  exact=True sums the products of the doubles at 50 digits.  Returns (lhs, rhs, terms), [K, n]."""
    K, n = next(iter(outs.values())).shape[:2]
    pairs_l = [(np.asarray(bars[COTANGENT_OF[k]], np.float64).reshape(1, n, 12), np.asarray(outs[k], np.float64).reshape(K, n, 12)) for k in OUTPUTS]
    pairs_r = [(np.asarray(adj[bar], np.float64).reshape(1, n, TANGENTS[name]), np.asarray(tans[name], np.float64).reshape(K, n, TANGENTS[name]))
               for name, bar in BAR_OF.items() if tans.get(name) is not None]
    if tans.get("Rwb_rot_tan") is not None:
        d = np.asarray(tans["Rwb_rot_tan"], np.float64).reshape(K, n, 3)
        pairs_r.append((np.asarray(adj["Rwb_bar"], np.float64).reshape(1, n, 9), skew_times(d, np.broadcast_to(np.asarray(Rwb, np.float64).reshape(1, n, 9), (K, n, 9)))))

    def side(pairs):
        tot, mag = np.zeros((K, n)), np.zeros((K, n))
        for g, t in pairs:
            g = np.broadcast_to(g, t.shape)
            mag += (np.abs(g) * np.abs(t)).sum(axis=2)
            if exact:
                with mp.workdps(DPS):
                    tot = tot + np.array([[mp.fdot(g[k, i].tolist(), t[k, i].tolist()) for i in range(n)] for k in range(K)], dtype=object)
            else:
                tot += (g * t).sum(axis=2)
        return tot, mag

    (lhs, ml), (rhs, mr) = side(pairs_l), side(pairs_r)
    return lhs, rhs, ml + mr


def moved(b, state, tans, k, h):
    """the batch and the records moved by h along direction k of `tans` (the rotation along its left tangent)"""
    n = b["x"].shape[0]
    out, rec = dict(b), state.copy()
    for name in ("x", "xdot", "w", "xdot_d", "joint_q"):
        if tans.get(name + "_tan") is not None:
            out[name] = np.asarray(b[name]) + h * np.asarray(tans[name + "_tan"])[k].reshape(np.asarray(b[name]).shape)
    if tans.get("Rwb_rot_tan") is not None:
        R = np.asarray(b["Rwb"]).reshape(n, 3, 3)
        out["Rwb"] = np.stack([exp_rotation(h * np.asarray(tans["Rwb_rot_tan"])[k, i]) @ R[i] for i in range(n)]).reshape(n, 9)
    for name in ("p_start", "p_final"):
        if tans.get(name + "_tan") is not None:
            rec[name] = state[name] + h * np.asarray(tans[name + "_tan"])[k].reshape(n, 12)
    return out, rec
