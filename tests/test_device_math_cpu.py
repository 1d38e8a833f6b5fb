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


# ---------------------------------------------------------------- wrench assembly and foothold references


def test_wrench_reference_against_the_kkt_restatement():
    """wrench_mp / wrench_ld (written from BC.cpp) against tests/kkt_batch.wrench_data (numpy + scipy's rotation log, shares no
    code with them): within the reference's own bar count * EPS * condition sum plus scipy's float64 log map (1e-13 rad through
    kp_w |Ib|).  The `sic` index shows: the variant with (2) += kff5 w_d2 is far outside."""
    from tests import kkt_batch as K

    rng = np.random.default_rng(11)
    P = R._wrench_params(rng)
    assert np.all(np.linalg.eigvalsh(P["Ib"]) > 0) and abs(P["Ib"][0, 1]) > 1e-4 and not np.allclose(P["Ib"], np.diag(np.diag(P["Ib"])))
    n = 3000
    b = R._wrench_states(rng, n)
    A, bv = K.wrench_data(P, b)
    o = R.wrench_ld(P, b, b["feet"])
    val, cond, cnt = o["b"]
    slack = 1e-13 * 5000.0 * np.abs(P["Ib"]).sum()
    assert np.all(np.abs(np.asarray(val, float) - bv) <= cnt * R.EPS * cond + slack)
    assert (cnt[:, :3] <= 6).all() and (cnt[:, 3:] == cnt[0, 3]).all()
    r_ref = np.stack([np.stack([A[:, 5, 3 * i + 1], A[:, 3, 3 * i + 2], A[:, 4, 3 * i]], 1) for i in range(4)], 1)  # x, y, z of r_i from [r_i]x
    rv, rc, rk = o["r"]
    assert np.all(np.abs(np.asarray(rv, float) - r_ref) <= rk * R.EPS * rc) and (rk == 3).all()
    wrong = R.wrench_ld(P, b, b["feet"], sic=False)["b"][0]
    assert np.median(np.abs(np.asarray(wrong, float) - bv)[:, 3:].max(1)) > 1e-3  # the other index is not within any bar
    # a transposed Iw = R^T Ib R is not within the bar either (Ib is not diagonal here)
    Rm = b["Rwb"].reshape(n, 3, 3)
    bT = dict(b, Rwb=np.swapaxes(Rm, 1, 2).reshape(n, 9), Rwb_d=(b["Rwb_d"].reshape(n, 3, 3) @ Rm @ Rm).reshape(n, 9))  # same R_err, Rwb^T in Iw
    assert np.median(np.abs(K.wrench_data(P, bT)[1] - bv)[:, 3:].max(1)) > 1e-3
    # 50 digits against long double on a subsample, and the condition sums / counts of the two agree
    for i in range(0, n, 150):
        m = R.wrench_mp(P, {k: v[i] for k, v in b.items()}, b["feet"][i])
        assert np.all(np.abs(m["b"][0] - np.asarray(val[i], float)) <= 2.0 ** -60 * cond[i] * cnt[i] + 1e-300)
        np.testing.assert_allclose(m["b"][1], cond[i], rtol=1e-6)
        assert np.array_equal(m["b"][2], cnt[i])


def test_wrench_reference_forward_kinematics_variant():
    """`kin`: the feet come from forwardKinematics of the joint angles: r against R.leg_fk_ld (itself held to the C oracle above)."""
    rng = np.random.default_rng(12)
    P = R._wrench_params(rng)
    n = 400
    b = R._wrench_states(rng, n)
    qj = np.stack([rng.uniform(-0.6, 0.6, (n, 4)), rng.uniform(-0.2, 1.4, (n, 4)), rng.uniform(-2.4, -0.3, (n, 4))], 2).reshape(n, 12)
    o = R.wrench_ld(P, b, qj, kin=(R.HIP, R.LINKS))
    feet = np.concatenate([np.asarray(R.leg_fk_ld(i, qj[:, 3 * i:3 * i + 3]), np.float64) for i in range(4)], 1)
    o2 = R.wrench_ld(P, b, feet)
    rv, rc, rk = o["r"]
    assert np.all(np.abs(np.asarray(rv - o2["r"][0], float)) <= 4 * R.EPS * rc)  # (the rounding of `feet` to double)
    assert np.array_equal(np.asarray(o["b"][0], float), np.asarray(o2["b"][0], float))  # b does not read the feet


def test_foothold_reference_against_the_tick_restatement():
    from oracle import tick_restatement as T
    from scipy.spatial.transform import Rotation

    rng = np.random.default_rng(13)
    fp = T.FootPlanner(k=0.07)
    for trial in range(200):
        leg = int(rng.integers(0, 4))
        Rw = Rotation.random(random_state=trial).as_matrix()
        x = np.array([rng.normal(), rng.normal(), rng.uniform(0.05, 0.6)])
        xdot, w, xdd, foot = rng.normal(size=3), rng.normal(size=3), rng.normal(size=3), rng.uniform(-0.4, 0.4, 3)
        want = fp.single_foot(0.31, Rw, x, xdot, w, xdd, foot, T.LEGS[leg])
        v, c, k = R.foothold_mp(T.HIP_MAP[T.LEGS[leg]], 0.07, 0.31, Rw, x, xdot, w, xdd, foot)
        assert v[2] == 0.0 and want[2] == 0.0
        assert np.all(np.abs(v - want) <= k * R.EPS * c), (v, want, k, c)
        vl, cl, kl = R.foothold_ld(T.HIP_MAP[T.LEGS[leg]][None], 0.07, 0.31, Rw.reshape(1, 9), x[None], xdot[None], w[None], xdd[None], (Rw @ foot)[None],
                                   foot_is_lever=True)
        assert np.all(np.abs(np.asarray(vl[0], float) - v) <= 4 * R.EPS * c) and (kl[0] <= k).all()


def test_probe_wraps_the_wrench_and_the_foothold():
    """The two new launchers call the header's functions on a RawState / arrays they only copy; nothing of them is restated."""
    src = open(PROBE).read()
    assert "wrench_from_state<4, KIN>(params(), S, f, 0, W)" in src and "plan_foothold(params(), l, R, x, xdot, w, xdd, pc, o)" in src
    for word in ("angle_axis_total(Re", "9.81", "kff[", "sqrt("):
        assert word not in src.split("extern \"C\"")[0], word


def test_odd_kin_is_off_every_symmetry_of_the_default_model():
    """ODD_KIN against the default model: every link and hip x, y is the default times a factor in [0.8, 1.25], all twelve factors of
    each distinct; the links keep their signs, no two legs share a length and |l2| != |l3| on every leg; hip z is non-zero, of both
    signs, within 0.04; nine distinct gains, no kd equal to 1, kff non-zero with mixed signs and at most 0.5; asymmetric limits; an
    anisotropic leg inertia.  The default model's per-leg band end is the one constant the restatements always used."""
    from tests import leg_plant_restatement as LR

    k, d = R.ODD_KIN, R.DEFAULT_KIN
    f = k.links / d.links
    assert (f >= 0.8).all() and (f <= 1.25).all() and len(set(np.round(f.reshape(-1), 9))) == 12
    assert (np.sign(k.links) == np.sign(d.links)).all()
    for c in range(3):
        assert len(set(np.abs(k.links[:, c]))) == 4
    assert (np.abs(k.links[:, 1]) != np.abs(k.links[:, 2])).all()
    h = k.hip[:, :2] / d.hip[:, :2]
    assert (h >= 0.8).all() and (h <= 1.25).all() and len(set(np.round(h.reshape(-1), 9))) == 8 and len(set(k.hip.reshape(-1))) == 12
    z = k.hip[:, 2]
    assert (z != 0).all() and (z > 0).any() and (z < 0).any() and (np.abs(z) <= 0.04).all()
    gains = k.jc_kp + k.jc_kd + k.jc_kff
    assert len(set(gains)) == 9 and 1.0 not in k.jc_kd and all(v != 0 for v in k.jc_kff) and min(k.jc_kff) < 0 < max(k.jc_kff)
    assert max(abs(v) for v in k.jc_kff) <= 0.5 and k.tau_min != -k.tau_max and k.tau_min < 0 < k.tau_max
    assert len(set(k.leg_inertia)) == 3
    assert all(d.det_lo(leg) == LR.DET_LO for leg in range(4)) and len({k.det_lo(leg) for leg in range(4)}) == 4
