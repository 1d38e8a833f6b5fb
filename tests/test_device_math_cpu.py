"""CPU: the device-math probe cross-compiles for gfx950 and exports every launcher, and the high-precision references of
tests/test_gpu_device_math.py agree with independent answers where one exists (scipy's rotation log, the C oracle's and the
tick restatement's kinematics, the tick restatement's sextic trajectory and angle wraps)."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import device_math_reference as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PROBE = os.path.join(ROOT, "tests", "hip", "device_math_probe.hip")


def test_probe_cross_compiles_and_exports_every_launcher(tmp_path):
    import __graft_entry__ as g
    from tests import device_probe as D

    if not os.path.exists(g.HIPCC) and shutil.which("hipcc") is None:
        pytest.fail(f"hipcc not found at {g.HIPCC}")
    out = str(tmp_path / "libprobe.so")
    subprocess.check_call([g.HIPCC] + g.HIP_FLAGS + [PROBE, "-o", out], cwd=os.path.dirname(PROBE))
    syms = subprocess.run(["nm", "-D", "--defined-only", out], stdout=subprocess.PIPE, text=True, check=True).stdout
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    missing = [f for f in D.LAUNCHERS if f not in names]
    assert not missing, f"launchers not exported: {missing}"


def test_probe_source_is_thin_and_allocation_free():
    """The probe applies the header's functions; it allocates and copies nothing itself (device pointers come from torch)."""
    src = open(PROBE).read()
    assert '#include "../../quadruped_control_amd/csrc/qc_device.hpp"' in src
    for word in ("hipMalloc", "hipMemcpy", "hipFree"):
        assert word not in src, word


def test_eigen_log_map_restatement_against_scipy():
    from scipy.spatial.transform import Rotation

    rng = np.random.default_rng(1)
    for _ in range(300):
        axis = rng.normal(size=3)
        angle = rng.uniform(0.0, 3.0)
        M = R.rotation_mp(axis, angle)
        ref, ang, _ = R.angle_axis_total_mp(M)
        np.testing.assert_allclose(ref, Rotation.from_matrix(M).as_rotvec(), atol=1e-13)
        assert abs(ang - angle) <= 1e-13
    # each of Eigen's four branches is reached
    cases = {R.eigen_case(R.rotation_mp(ax, 3.0)) for ax in ([1, 0.1, 0.1], [0.1, 1, 0.1], [0.1, 0.1, 1])}
    cases.add(R.eigen_case(R.rotation_mp([1, 2, 3], 0.5)))
    assert cases == {-1, 0, 1, 2}
    # ties keep the lower index: m00 = m11 > m22 -> 0; m11 = m22 > m00 -> 1
    assert R.eigen_case(np.diag([0.5, 0.5, -2.0])) == 0 and R.eigen_case(np.diag([-2.0, 0.5, 0.5])) == 1


def test_inverse_kinematics_restatement_against_the_oracle():
    from oracle import c_oracle as O
    from oracle import tick_restatement as T

    O.build()
    rng = np.random.default_rng(2)
    for _ in range(200):
        leg = int(rng.integers(0, 4))
        q = np.array([rng.uniform(-0.6, 0.6), rng.uniform(-0.2, 1.4), rng.uniform(-2.4, -0.3)])
        p = O.leg_fk(leg, q)
        np.testing.assert_allclose(np.asarray(R.leg_fk_ld(leg, q[None])[0], float), p, atol=1e-15)
        qm, _ = R.leg_inverse_kinematics_mp(leg, p)
        qm = np.array([float(v) for v in qm])
        np.testing.assert_allclose(qm, q, atol=1e-12)
        np.testing.assert_allclose(qm, O.leg_ik(leg, p), atol=1e-12)
        np.testing.assert_allclose(qm, T.leg_inverse_kinematics(T.LEGS[leg], p), atol=1e-12)
        np.testing.assert_allclose(np.asarray(R.leg_jacobian_ld(leg, q[None])[0], float), O.leg_jacobian(leg, q), atol=1e-15)


def test_sextic_trajectory_restatement_against_the_tick_restatement():
    from oracle import tick_restatement as T

    B, basis = R.sextic_basis_mp()
    rng = np.random.default_rng(3)
    duty = 0.8 / (0.18 + 0.8)
    for _ in range(100):
        p0, pf = rng.uniform(-0.4, 0.4, 3), rng.uniform(-0.4, 0.4, 3)
        phase = rng.uniform(0.0, 1.2)
        pos, vel, t = R.track_swing_mp(B, phase, p0, pf, 0.08, 0.18, 0.8)
        pc = np.array([0.5 * (p0[0] + pf[0]), 0.5 * (p0[1] + pf[1]), 0.08])
        tp, tv = T.FootTrajectory(p0, pc, pf).track(t)
        np.testing.assert_allclose(pos, tp, atol=1e-14)
        np.testing.assert_allclose(vel, tv, atol=1e-13)
        assert abs(t - min(max((phase - duty) / (1.0 - duty), 0.0), 1.0)) < 1e-14


def test_unfused_wraps_against_the_tick_restatement():
    from oracle import tick_restatement as T

    rng = np.random.default_rng(4)
    x = np.concatenate([rng.uniform(-1e4, 1e4, 5000), np.arange(-20, 21) * 2.0 * R.PI, [R.PI, -R.PI, 0.0, -0.0, 1e15]])
    np.testing.assert_array_equal(R.normalize_angle_2PI_unfused(x), [T.normalize_angle_2PI(float(v)) for v in x])
    np.testing.assert_array_equal(R.normalize_angle_PI_unfused(x), [T.normalize_angle_PI(float(v)) for v in x])


def test_references_of_the_small_primitives():
    """sin / cos, rsqrt and the exact sum against math / fractions where the answer is known exactly."""
    assert R.sincos_mp(0.0) == (0.0, 1.0) and R.sincos_mp(math.pi / 2)[1] == 6.123233995736766e-17
    rs, rc = R.rsqrt_rcp_ld(np.array([4.0, 0.25]))
    assert list(rs) == [0.5, 2.0] and list(rc) == [0.25, 4.0]
    assert R.exact_sum([1e16, 1.0, -1e16]) == 1.0
    M = np.array([[4.0, 1.0], [1.0, 3.0]])
    np.testing.assert_allclose(R.solve_mp(M, [1.0, 2.0]), np.linalg.solve(M, [1.0, 2.0]), rtol=1e-15)
