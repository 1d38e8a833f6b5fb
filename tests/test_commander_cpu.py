"""CPU: the commander-mode restatement on hand-checked cases, and the C ABI of qc_tick_batch (exports, struct sizes,
the initial state) - no GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np

from tests import commander_restatement as CR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _rz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _rx(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def _ry(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def test_pure_yaw_twist():
    x = np.array([1.0, 2.0, 0.26])
    wz, vx, dt = 0.05, 0.2, 0.001
    Rd, xd = CR.integrate_twist_yaw(np.eye(3), x, [vx, 0, 0, 0, 0, wz], dt)
    th = wz * dt
    np.testing.assert_allclose(Rd[0], _rz(th), atol=1e-15)
    # the translation is rotated by Rbb' before it is added
    np.testing.assert_allclose(xd[0], x + np.array([np.cos(th) * vx * dt, np.sin(th) * vx * dt, 0.0]), atol=1e-16)
    # a yawed pose: the increment composes on the right of Rz(yaw)
    Rd2, xd2 = CR.integrate_twist_yaw(_rz(0.7), x, [vx, 0, 0, 0, 0, wz], dt)
    np.testing.assert_allclose(Rd2[0], _rz(0.7 + th), atol=1e-15)
    np.testing.assert_allclose(xd2[0], x + vx * dt * np.array([np.cos(0.7 + th), np.sin(0.7 + th), 0.0]), atol=1e-16)


def test_rotation_threshold_branches():
    x = np.array([0.3, -0.1, 0.25])
    v = np.array([0.2, -0.1, 0.03])
    dt = 0.001
    # theta = 0.9e-12 < 1e-12: Rbb' = I and t = v dt, unrotated
    below = np.concatenate([v, [0.0, 0.0, 0.9e-9]])
    Rd, xd = CR.integrate_twist_yaw(np.eye(3), x, below, dt)
    assert np.array_equal(Rd[0], np.eye(3))
    assert np.array_equal(xd[0], x + v * dt)
    # theta = 1.1e-12: the angle-axis branch, and the translation is rotated by it
    above = np.concatenate([v, [0.0, 0.0, 1.1e-9]])
    Rd, xd = CR.integrate_twist_yaw(np.eye(3), x, above, dt)
    th = 1.1e-12
    assert Rd[0][0, 1] == -np.sin(th) and Rd[0][1, 0] == np.sin(th)
    Rb = _rz(th)
    np.testing.assert_allclose(xd[0], x + Rb @ v * dt, rtol=0, atol=1e-18)
    assert not np.array_equal(xd[0], x + v * dt)
    # a general axis: Rbb' is the rotation by |delta| about delta / |delta|
    w = np.array([0.03, -0.02, 0.05])
    Rd, _ = CR.integrate_twist_yaw(np.eye(3), x, np.concatenate([v, w]), 0.5)
    d = w * 0.5
    th = np.linalg.norm(d)
    a = d / th
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    np.testing.assert_allclose(Rd[0], np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K, atol=1e-15)
    np.testing.assert_allclose(Rd[0] @ Rd[0].T, np.eye(3), atol=1e-15)


def test_tilted_pose_keeps_yaw_only():
    yaw, pitch, roll = 0.9, 0.2, -0.15
    Rwb = _rz(yaw) @ _ry(pitch) @ _rx(roll)
    x = np.array([0.1, 0.2, 0.3])
    Rd, xd = CR.integrate_twist_yaw(Rwb, x, np.zeros(6))
    np.testing.assert_allclose(Rd[0], _rz(yaw), atol=1e-15)  # roll and pitch dropped
    assert np.array_equal(xd[0], x)
    v = np.array([0.2, 0.1, 0.0])
    _, xd = CR.integrate_twist_yaw(Rwb, x, np.concatenate([v, np.zeros(3)]), 0.001)
    np.testing.assert_allclose(xd[0], x + _rz(yaw) @ v * 0.001, atol=1e-17)
    # at gimbal lock the restatement (like the device) takes yaw = 0 and stays finite
    Rgl = _ry(np.pi / 2)
    Rgl[0, 0] = Rgl[1, 0] = 0.0
    Rd, _ = CR.integrate_twist_yaw(Rgl, x, np.zeros(6))
    assert np.array_equal(Rd[0], np.eye(3))


def test_adjoint_quirk():
    Rwb = _rz(0.4) @ _ry(0.1) @ _rx(0.05)
    x = np.array([0.5, -0.3, 0.26])
    Vb = np.array([0.2, 0.1, 0.0, 0.01, -0.02, 0.05])
    v, w = CR.adjoint_twist(Rwb, x, Vb)
    np.testing.assert_allclose(v[0], Rwb.T @ (Vb[:3] - np.cross(x, Vb[3:])), atol=1e-16)
    np.testing.assert_allclose(w[0], Rwb.T @ Vb[3:], atol=1e-16)
    # the 6x6 matrix of rigid3d.cpp:259-271 itself
    px = np.array([[0, -x[2], x[1]], [x[2], 0, -x[0]], [-x[1], x[0], 0]])
    Ad = np.zeros((6, 6))
    Ad[:3, :3] = Rwb.T
    Ad[3:, 3:] = Rwb.T
    Ad[:3, 3:] = -Rwb.T @ px
    np.testing.assert_allclose(np.concatenate([v[0], w[0]]), Ad @ Vb, atol=1e-16)
    # not the physical world-frame twist
    assert np.max(np.abs(v[0] - Rwb @ Vb[:3])) > 1e-3


def test_stand_threshold_is_strict():
    # values exact in binary: |x - h| == tol exactly is NOT standing
    h, tol = 0.25, 2.0 ** -7
    c = CR.Commander(4, x_stand=(0.0, 0.0, h), stand_tol=tol)
    xs = np.array([h + tol, h - tol, np.nextafter(h + tol, 0.0), np.nextafter(h - tol, 1.0)])
    assert np.abs(xs[0] - h) == tol and np.abs(xs[1] - h) == tol
    x = np.stack([np.zeros(4), np.zeros(4), xs], axis=1)
    run, _ = c.step(np.tile(np.eye(3).reshape(9), (4, 1)), x)
    assert c.standing.tolist() == [0, 0, 1, 1] and not run.any()
    # the reference's defaults: 0.26 +- 0.005
    c = CR.Commander(3)
    x = np.array([[0, 0, 0.26 + 0.0049], [0, 0, 0.26 - 0.0051], [0, 0, 0.255]])
    c.step(np.tile(np.eye(3).reshape(9), (3, 1)), x)
    assert c.standing.tolist() == [1, 0, int(abs(0.255 - 0.26) < 0.005)]
    # latched: leaving the band does not reset it
    c.step(np.tile(np.eye(3).reshape(9), (3, 1)), np.zeros((3, 3)))
    assert c.standing[0] == 1


def test_command_held_until_the_gait_runs():
    c = CR.Commander(1)
    R = np.eye(3).reshape(1, 9)
    tw = np.array([[0.2, 0.05, 0.0, 0.01, 0.0, 0.04]])
    low = np.array([[0.0, 0.0, 0.20]])
    stand = np.array([[0.01, 0.02, 0.258]])
    init = c.desired()
    # tick 0: a command arrives while the robot is still rising: held
    run, applied = c.step(R, low, tw, np.array([1]))
    assert not run[0] and not applied[0]
    assert c.flags().tolist() == [[0, 0, 1]] and np.array_equal(c.Vb, tw)
    assert all(np.array_equal(c.desired()[k], init[k]) for k in init)
    # tick 1: the stand height is reached: standing, the gait starts, nothing else
    run, applied = c.step(R, stand)
    assert not run[0] and not applied[0] and c.flags().tolist() == [[1, 1, 1]]
    assert all(np.array_equal(c.desired()[k], init[k]) for k in init)
    # tick 2: the gait runs and the held command becomes the desired state
    run, applied = c.step(R, stand)
    assert run[0] and applied[0] and c.flags().tolist() == [[1, 1, 0]]
    Rd, xd = CR.integrate_twist_yaw(R, stand, tw)
    v, w = CR.adjoint_twist(R, stand, tw)
    np.testing.assert_array_equal(c.Rwb_d, Rd.reshape(1, 9))
    assert c.x_d[0, 2] == 0.26 and np.array_equal(c.x_d[0, :2], xd[0, :2])
    np.testing.assert_array_equal(c.xdot_d, v)
    np.testing.assert_array_equal(c.w_d, w)
    # tick 3: no new command: the desired state stays
    d = c.desired()
    run, applied = c.step(R, stand + 0.001)
    assert run[0] and not applied[0] and all(np.array_equal(c.desired()[k], d[k]) for k in d)


def test_commander_symbols_exported(built):
    from quadruped_control_amd import _lib

    lib = ctypes.CDLL(os.path.join(ROOT, "quadruped_control_amd", "libqc_balance.so"))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qc_balance.h")).read(), flags=re.S)
    for name in ("qc_tick_batch", "qc_default_command", "qc_commander_state_init"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name) and name in _lib.EXPORTS


def test_struct_mirrors_match_the_header(built, tmp_path):
    from quadruped_control_amd import _lib
    from quadruped_control_amd.balance_controller import COMMANDER_STATE_DTYPE

    src = tmp_path / "sizes.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"qc_balance.h\"\n"
                   "int main(void) { printf(\"%zu %zu %zu %zu %zu %zu %zu\\n\", sizeof(qc_commander_state), sizeof(qc_command_in),"
                   " offsetof(qc_commander_state, Vb), offsetof(qc_commander_state, w_d), offsetof(qc_command_in, state),"
                   " offsetof(qc_command_in, stand_height), offsetof(qc_command_in, cmd_dt)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["g++", "-x", "c++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S, Cin = _lib.QcCommanderState, _lib.QcCommandIn
    assert got == [ctypes.sizeof(S), ctypes.sizeof(Cin), S.Vb.offset, S.w_d.offset, Cin.state.offset, Cin.stand_height.offset, Cin.cmd_dt.offset]
    assert got[0] == COMMANDER_STATE_DTYPE.itemsize == 208
    assert COMMANDER_STATE_DTYPE.fields["Vb"][1] == S.Vb.offset and COMMANDER_STATE_DTYPE.fields["w_d"][1] == S.w_d.offset


def test_initial_state_and_default_command(built):
    from quadruped_control_amd import _lib
    from quadruped_control_amd.balance_controller import new_commander_states

    s = new_commander_states(5)
    ref = CR.Commander(5)
    assert np.array_equal(np.stack([s["standing"], s["gait_running"], s["cmd_pending"]], axis=1), ref.flags())
    assert (s["reserved"] == 0).all() and (s["Vb"] == 0).all()
    for k, v in ref.desired().items():
        assert np.array_equal(s[k], v), k
    s = new_commander_states(2, x_stand=(0.1, -0.2, 0.3))
    assert np.array_equal(s["x_d"], [[0.1, -0.2, 0.3]] * 2)
    # NULL x_stand: the reference's (0, 0, 0.26)
    raw = np.zeros(3, dtype=s.dtype)
    _lib.load().qc_commander_state_init(raw.ctypes.data_as(ctypes.c_void_p), 3, None)
    assert np.array_equal(raw["x_d"], [[0.0, 0.0, 0.26]] * 3) and np.array_equal(raw["Rwb_d"], [np.eye(3).reshape(9)] * 3)
    c = _lib.QcCommandIn()
    _lib.load().qc_default_command(ctypes.byref(c))
    assert c.struct_size == ctypes.sizeof(_lib.QcCommandIn)
    assert (c.stand_height, c.stand_tol, c.cmd_dt) == (CR.X_STAND[2], CR.STAND_TOL, CR.CMD_DT)
    assert not c.twist and not c.fresh and not c.state


# ---------------------------------------------------------------- the high-precision commander reference
def _commander_sweep(rng, n, wide):
    """`wide`: the GPU sweep's ranges (|w| dt log-uniform over [1e-14, 50], |x| up to 1e6, roll / pitch up to 1.5 rad); else the
    closed-loop tests' domain (small twists at cmd_dt = 1e-3)."""
    from scipy.spatial.transform import Rotation

    if wide:
        dt = 0.5
        ang = np.exp(rng.uniform(np.log(1e-14), np.log(50.0), n))
        ax = rng.normal(size=(n, 3))
        w = ax / np.linalg.norm(ax, axis=1, keepdims=True) * (ang / dt)[:, None]
        v = rng.normal(size=(n, 3)) * rng.uniform(0, 10.0 / np.sqrt(3), (n, 1))
        x = rng.normal(size=(n, 3)) * np.exp(rng.uniform(np.log(1e-3), np.log(1e6), (n, 1)))
        eul = np.stack([rng.uniform(-np.pi, np.pi, n), rng.uniform(-1.5, 1.5, n), rng.uniform(-1.5, 1.5, n)], 1)
    else:
        dt = 1e-3
        w = rng.uniform(-0.05, 0.05, (n, 3))
        v = rng.uniform(-0.2, 0.2, (n, 3))
        x = rng.normal(size=(n, 3))
        eul = np.stack([rng.uniform(-np.pi, np.pi, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n)], 1)
    Rw = Rotation.from_euler("ZYX", eul).as_matrix().reshape(n, 9)
    return Rw, x, np.concatenate([v, w], 1), dt


def _restated(Rw, x, Vb, dt, h):
    Rd, xd = CR.integrate_twist_yaw(Rw, x, Vb, dt)
    xd[:, 2] = h
    v, w = CR.adjoint_twist(Rw, x, Vb)
    return dict(Rwb_d=Rd.reshape(-1, 9), x_d=xd, xdot_d=v, w_d=w)


def test_commander_reference_against_the_restatement():
    """commander_apply_mp / _ld (tests/device_math_reference.py, written from trajectory.cpp and rigid3d.cpp) against the float64
    restatement, which shares no code with them: to 1e-13 on the restatement's own domain; and over the GPU sweep's ranges the
    restatement - a plain double evaluation of the same formulas - sits inside count * EPS * condition sum entry by entry, which
    is what the GPU test asks of the device (a bar a correct double evaluation could miss would be a wrong bar)."""
    from tests import device_math_reference as R

    rng = np.random.default_rng(21)
    for wide, n in ((False, 4000), (True, 20000)):
        Rw, x, Vb, dt = _commander_sweep(rng, n, wide)
        ref = R.commander_apply_ld(Rw, x, Vb, dt, 0.26)
        got = _restated(Rw, x, Vb, dt, 0.26)
        assert ref["small"].sum() > (100 if wide else -1) and (~ref["small"]).sum() > 100
        for k, (val, cond, cnt) in ((k, ref[k]) for k in got):
            err = np.abs(got[k] - np.asarray(val, np.float64))
            if not wide:
                assert err.max() <= 1e-13, (k, err.max())
            assert np.all(err <= cnt * R.EPS * cond + 5e-324), (k, wide, float(np.max(err / np.maximum(cnt * R.EPS * cond, 5e-324))))
            bound = np.where(ref["small"][:, None], R.COMMANDER_COUNTS_SMALL[k], R.COMMANDER_COUNTS[k])
            assert (cnt <= bound).all() and cnt.max() == R.COMMANDER_COUNTS[k], (k, cnt.max())
        for i in range(0, n, n // 40):
            m = R.commander_apply_mp(Rw[i], x[i], Vb[i], dt, 0.26)
            assert m["small"] == ref["small"][i] and m["yaw_ok"]
            for k in got:
                val, cond, cnt = ref[k]
                assert np.all(np.abs(m[k][0] - np.asarray(val[i], np.float64)) <= 2.0 ** -60 * cnt[i] * cond[i] + 2.0 ** -1074 + R.EPS * np.abs(m[k][0]))
                assert np.array_equal(m[k][2], cnt[i])


def test_commander_reference_branches():
    """The two double decisions: the angle threshold is |angle| < 1e-12 strictly, on the double norm; a pose without a yaw
    (R00 = R10 = 0, |R00|, |R10| < 1.5e-162 whose squares underflow to 0, a non-finite entry) takes yaw 0 as INTEGRATION.md says."""
    from tests import device_math_reference as R

    x, v = np.array([0.0, 0.0, 0.3]), np.array([0.25, -0.5, 0.125])
    for ang, small in ((0.0, True), (-0.0, True), (9.9e-13, True), (np.nextafter(1e-12, 0), True), (1e-12, False), (np.nextafter(1e-12, 1), False), (1e-9, False)):
        m = R.commander_apply_mp(np.eye(3), x, np.concatenate([v, [0.0, 0.0, ang * 1024.0]]), 2.0 ** -10, 0.26)
        assert m["small"] == small, ang
        if small:
            assert np.array_equal(m["Rwb_d"][0], np.eye(3).reshape(9)) and np.array_equal(m["x_d"][0], [v[0] / 1024, v[1] / 1024, 0.26])
        else:
            assert m["Rwb_d"][0][3] == np.sin(ang) and m["x_d"][0][1] != v[1] / 1024
    for r00, r10 in ((0.0, 0.0), (1e-163, -1e-163), (np.nan, 0.5), (np.inf, 0.0), (0.3, -np.inf)):
        Rw = _ry(np.pi / 2)
        Rw[0, 0], Rw[1, 0] = r00, r10
        m = R.commander_apply_mp(Rw, x, np.concatenate([v, [0.0, 0.0, 0.0]]), 1e-3, 0.26)
        assert not m["yaw_ok"] and np.array_equal(m["Rwb_d"][0], np.eye(3).reshape(9))
    # quadrants with exact zeros: yaw = pi/2 -> Rz = [[0, -1], [1, 0]] exactly, pi -> diag(-1, -1)
    m = R.commander_apply_mp(np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1.0]]), x, np.zeros(6), 1e-3, 0.26)
    assert np.array_equal(m["Rwb_d"][0], [0, -1, 0, 1, 0, 0, 0, 0, 1])
    m = R.commander_apply_mp(np.diag([-1.0, -1.0, 1.0]), x, np.zeros(6), 1e-3, 0.26)
    assert np.array_equal(m["Rwb_d"][0], [-1, 0, 0, 0, -1, 0, 0, 0, 1])
