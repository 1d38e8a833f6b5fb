"""numpy restatement of the reference's commander loop body (test infrastructure, not the product): what qc_tick_batch
computes before the controller runs, for n robots per tick.

Written from the reference:
  commander_node.cpp:191-202   cmdCallback: Vb = command, cmd_vel_received = true
  commander_node.cpp:344-367   initial state: Rwb_d = I, x_d = x_stand = (0, 0, 0.26), xdot_d = w_d = 0, dt = 0.001
  commander_node.cpp:386-391   standing latches when almost_equal(x(2), x_stand(2), 0.005) (strict |a - b| < eps)
  commander_node.cpp:395-478   standing: if gait_running { apply a pending command; schedule + plan } else { start the gait }
  trajectory.cpp:29-69         integrate_twist_yaw (angle-axis increment, translation rotated by it, yaw of Rwb only)
  rigid3d.cpp:259-271          Transform3d::adjoint = [[R^T, -R^T [p]x], [0, R^T]] of the CURRENT pose
The rest of the tick (gait clock, contact rule, planner, QP, J^T) is checked with oracle.c_oracle.
"""
from __future__ import annotations

import numpy as np

X_STAND = (0.0, 0.0, 0.26)
STAND_TOL = 0.005
CMD_DT = 0.001


def rodrigues(delta):
    """Rbb' for angle-axis increments delta [n,3]: identity where |delta| < 1e-12 (almost_equal(angle, 0.0))."""
    delta = np.asarray(delta, np.float64).reshape(-1, 3)
    th = np.sqrt(np.sum(delta * delta, axis=1))
    small = np.abs(th) < 1e-12
    R = np.tile(np.eye(3), (delta.shape[0], 1, 1))
    big = ~small
    if big.any():
        a = delta[big] / th[big, None]
        s, c = np.sin(th[big]), np.cos(th[big])
        K = np.zeros((a.shape[0], 3, 3))
        K[:, 0, 1], K[:, 0, 2] = -a[:, 2], a[:, 1]
        K[:, 1, 0], K[:, 1, 2] = a[:, 2], -a[:, 0]
        K[:, 2, 0], K[:, 2, 1] = -a[:, 1], a[:, 0]
        R[big] = (c[:, None, None] * np.eye(3) + s[:, None, None] * K + (1.0 - c)[:, None, None] * np.einsum("ni,nj->nij", a, a))
    return R, small


def yaw_rotation(Rwb):
    """Rz(yaw) of Rwb [n,3,3], yaw = atan2(R10, R00) (Drake's RollPitchYaw away from pitch = +-pi/2).  At gimbal lock (h = 0)
    the device takes yaw = 0; what Drake does there is not pinned."""
    Rwb = np.asarray(Rwb, np.float64).reshape(-1, 3, 3)
    h = np.sqrt(Rwb[:, 0, 0] ** 2 + Rwb[:, 1, 0] ** 2)
    ok = (h > 0.0) & (h < 1e300)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.where(ok, Rwb[:, 0, 0] / np.where(ok, h, 1.0), 1.0)
        s = np.where(ok, Rwb[:, 1, 0] / np.where(ok, h, 1.0), 0.0)
    Rz = np.zeros_like(Rwb)
    Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = c, -s, s, c, 1.0
    return Rz


def integrate_twist_yaw(Rwb, x, Vb, dt=CMD_DT):
    """trajectory.cpp:29-69 for n poses: returns (Rwb_d [n,3,3], x_d [n,3]) - before the commander overwrites x_d(2)."""
    Rwb = np.asarray(Rwb, np.float64).reshape(-1, 3, 3)
    x = np.asarray(x, np.float64).reshape(-1, 3)
    Vb = np.asarray(Vb, np.float64).reshape(-1, 6)
    Rb, small = rodrigues(Vb[:, 3:6] * dt)
    t = np.where(small[:, None], Vb[:, 0:3] * dt, np.einsum("nij,nj->ni", Rb, Vb[:, 0:3]) * dt)  # the translation IS rotated
    Rz = yaw_rotation(Rwb)
    return Rz @ Rb, x + np.einsum("nij,nj->ni", Rz, t)


def adjoint_twist(Rwb, x, Vb):
    """Transform3d(Rwb, x).adjoint() * Vb (rigid3d.cpp:259-271): (R^T (v - x x w), R^T w) - not the world-frame twist."""
    Rwb = np.asarray(Rwb, np.float64).reshape(-1, 3, 3)
    x = np.asarray(x, np.float64).reshape(-1, 3)
    Vb = np.asarray(Vb, np.float64).reshape(-1, 6)
    Rt = np.transpose(Rwb, (0, 2, 1))
    u = Vb[:, 0:3] - np.cross(x, Vb[:, 3:6])
    return np.einsum("nij,nj->ni", Rt, u), np.einsum("nij,nj->ni", Rt, Vb[:, 3:6])


class Commander:
    """The commander loop's per-robot state for n robots, stepped once per tick like qc_tick_batch steps it."""

    def __init__(self, n, x_stand=X_STAND, stand_tol=STAND_TOL, cmd_dt=CMD_DT):
        self.n = n
        self.stand_height = float(x_stand[2])
        self.stand_tol = float(stand_tol)
        self.cmd_dt = float(cmd_dt)
        self.standing = np.zeros(n, np.int32)
        self.gait_running = np.zeros(n, np.int32)
        self.cmd_pending = np.zeros(n, np.int32)
        self.Vb = np.zeros((n, 6))
        self.Rwb_d = np.tile(np.eye(3).reshape(9), (n, 1))
        self.x_d = np.tile(np.asarray(x_stand, np.float64), (n, 1))
        self.xdot_d = np.zeros((n, 3))
        self.w_d = np.zeros((n, 3))

    def step(self, Rwb, x, twist=None, fresh=None):
        """One tick.  Returns (run, applied): `run` - the gait clock advances and the contact rule and planner run this tick;
        `applied` - a held command became the desired state this tick."""
        Rwb = np.asarray(Rwb, np.float64).reshape(self.n, 9)
        x = np.asarray(x, np.float64).reshape(self.n, 3)
        if fresh is not None:  # 1. cmdCallback
            f = np.asarray(fresh).astype(bool)
            self.Vb[f] = np.asarray(twist, np.float64).reshape(self.n, 6)[f]
            self.cmd_pending[f] = 1
        # 2. the stand latch (measured height)
        self.standing[(self.standing == 0) & (np.abs(x[:, 2] - self.stand_height) < self.stand_tol)] = 1
        st = self.standing == 1
        was_running = self.gait_running == 1
        run = st & was_running
        applied = run & (self.cmd_pending == 1)
        # 3. standing, not yet running: start the gait (the first schedule() is next tick)
        self.gait_running[st & ~was_running] = 1
        if applied.any():
            i = np.nonzero(applied)[0]
            Rd, xd = integrate_twist_yaw(Rwb[i], x[i], self.Vb[i], self.cmd_dt)
            xd[:, 2] = self.stand_height  # "TODO: height drifts"
            v, w = adjoint_twist(Rwb[i], x[i], self.Vb[i])
            self.Rwb_d[i] = Rd.reshape(-1, 9)
            self.x_d[i] = xd
            self.xdot_d[i] = v
            self.w_d[i] = w
            self.cmd_pending[i] = 0
        return run, applied

    def desired(self):
        return dict(Rwb_d=self.Rwb_d.copy(), x_d=self.x_d.copy(), xdot_d=self.xdot_d.copy(), w_d=self.w_d.copy())

    def flags(self):
        return np.stack([self.standing, self.gait_running, self.cmd_pending], axis=1)
