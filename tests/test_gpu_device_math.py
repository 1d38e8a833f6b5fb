"""GPU: the hand-written device math of qc_device.hpp, one primitive at a time (tests/hip/device_math_probe.hip), against
high-precision references (tests/device_math_reference.py).  The end-to-end tests compare through a QP at 1e-6 of max|GRF|;
a wrong coefficient digit, a lost Newton step or a flipped tie rule moves these primitives by 1e-16 ... 1e-9 and would pass
there.  Here the bars are a few epsilon.  Bars are absolute unless said otherwise; EPS = 2^-52."""
import math

import mpmath as mp
import numpy as np
import pytest

from tests import device_math_reference as R

pytestmark = pytest.mark.gpu
EPS = R.EPS


@pytest.fixture(scope="module")
def P():
    """The probe (a missing probe is an error, not a skip) with the default kinematics, gains and gait in its constants."""
    import __graft_entry__ as g

    g.build(force=False)
    g.build_device_probe()
    from tests import device_probe as D

    _, basis = R.sextic_basis_mp()
    D.set_params(R.HIP, R.LINKS, R.JC_KFF, R.JC_KP, R.JC_KD, basis, 0.18, 0.8, 0.08)
    return D


def _set_model(D, kin, t_stance=0.8, gains=None, wrench=None):
    """the probe's constants at the model `kin` (gains: (kff, kp, kd) instead of the model's)"""
    _, basis = R.sextic_basis_mp()
    kff, kp, kd = gains or (kin.jc_kff, kin.jc_kp, kin.jc_kd)
    D.set_params(kin.hip, kin.links, kff, kp, kd, basis, 0.18, t_stance, 0.08, wrench=wrench)


def _ulp_walk(x, k):
    """x and its +-1 ... k ulp neighbours"""
    out = [x]
    up = dn = x
    for _ in range(k):
        up = np.nextafter(up, np.inf); dn = np.nextafter(dn, -np.inf)
        out += [up, dn]
    return out


# ---------------------------------------------------------------- sincos_joint
def test_sincos_joint(P):
    """|err| <= 2 EPS for |x| < 2^30 against 50-digit sin / cos (edge set) and long double (1 M random points); relative
    <= 2 EPS on [-pi/4, pi/4]; sin(-0) = -0; NaN for |x| >= 2^30 and for non-finite x."""
    rng = np.random.default_rng(1)
    with mp.workdps(R.DPS):
        near = []
        for k in list(range(-64, 65)) + list(rng.integers(-2 ** 20, 2 ** 20, 400)) + [2 ** 20, -2 ** 20, 58, -58]:
            near += _ulp_walk(float(mp.mpf(int(k)) * mp.pi / 2), 3)
    tiny = [5e-324, -5e-324, 2.2250738585072014e-308 / 3, -1e-310, 1e-300, 1e-160, 1e-20]
    big = [np.nextafter(2.0 ** 30, 0.0), -np.nextafter(2.0 ** 30, 0.0), 2.0 ** 30 - 2.0 ** -22, -(2.0 ** 30 - 2.0 ** -22), np.pi / 4, -np.pi / 4, np.nextafter(np.pi / 4, 1.0)]
    edge = np.array(near + tiny + big + [0.0], np.float64)
    s, c = P.sincos(edge)
    rs = np.array([R.sincos_mp(x)[0] for x in edge]); rc = np.array([R.sincos_mp(x)[1] for x in edge])
    err = max(np.abs(s - rs).max(), np.abs(c - rc).max())
    assert err <= 2 * EPS, f"sincos_joint edge set: max abs err {err:.3e} ({err / EPS:.2f} eps)"
    small = np.abs(edge) <= np.pi / 4
    rel = np.abs(s[small] - rs[small]) / np.maximum(np.abs(rs[small]), 5e-324)
    assert rel.max() <= 2 * EPS, f"sin relative error on [-pi/4, pi/4]: {rel.max():.3e}"
    assert np.abs(c[small] - rc[small]).max() <= EPS  # cos near 1: within an ulp of 1
    # random sweeps under long double
    x = np.concatenate([rng.uniform(-7, 7, 400_000), rng.uniform(-1e3, 1e3, 300_000), rng.uniform(-1e6, 1e6, 300_000)])
    s, c = P.sincos(x)
    ls, lc = R.sincos_ld(x)
    err = float(max(np.abs(s - ls).max(), np.abs(c - lc).max()))
    assert err <= 2 * EPS, f"sincos_joint random sweep: max abs err {err:.3e}"
    # signed zero, the range limit, non-finite inputs
    s, c = P.sincos(np.array([-0.0, 0.0, 2.0 ** 30, -2.0 ** 30, 1e300, np.nan, np.inf, -np.inf]))
    assert math.copysign(1.0, s[0]) == -1.0 and s[0] == 0.0 and c[0] == 1.0, "sin(-0) must be -0, cos(-0) = 1"
    assert math.copysign(1.0, s[1]) == 1.0 and s[1] == 0.0 and c[1] == 1.0
    assert np.isnan(s[2:]).all() and np.isnan(c[2:]).all(), (s, c)


# ---------------------------------------------------------------- rsqrt_nr / rcp_nr
def test_rsqrt_rcp(P):
    """<= 1 ulp relative over normal inputs (log-uniform over the whole normal range, powers of two, DBL_MAX); the IEEE answer
    for 0, inf and NaN where the call sites select on it.  Subnormal inputs: rsqrt_nr is reached with a subnormal argument by
    angle_axis_total (|q_v|^2 of a rotation below ~1e-154 rad) and must give a finite result within 1 ulp there too;
    rcp_nr's call sites (LDL^T pivots, 3x3 determinants inside [eps, 1 / eps]) never pass one."""
    rng = np.random.default_rng(2)
    pw = [2.0 ** k for k in range(-1022, 1024, 7)] + [1.0, 4.0, 2.0, 0.5, 2.0 ** -1022, 2.0 ** 1023, np.finfo(np.float64).max]
    x = np.concatenate([np.exp2(rng.uniform(-1021.9, 1023.9, 400_000)), np.array(pw)])
    rs, rc = P.rsqrt_rcp(x)
    lrs, lrc = R.rsqrt_rcp_ld(x)
    ers = float((np.abs(rs - lrs) / lrs).max()); erc = float((np.abs(rc - lrc) / np.abs(lrc)).max())
    assert np.isfinite(rs).all() and ers <= EPS, f"rsqrt_nr: max rel err {ers:.3e} ({ers / EPS:.2f} eps)"
    # 1 / x for x near DBL_MAX is subnormal: there an ulp is 2^-1074 absolute, not relative
    normal = lrc >= 2.0 ** -1022
    assert (np.abs(rc - lrc) / np.abs(lrc))[normal].max() <= EPS, f"rcp_nr: max rel err {erc:.3e}"
    assert np.abs(rc - lrc)[~normal].max() <= 2.0 ** -1074
    # powers of two: exact
    p2 = np.array([2.0 ** k for k in range(-1020, 1021, 2)])
    rs, rc = P.rsqrt_rcp(p2)
    assert np.array_equal(rs, 1.0 / np.sqrt(p2)) and np.array_equal(rc, 1.0 / p2)
    # subnormal inputs of rsqrt_nr
    sub = np.array([5e-324, 1e-323, 2.5e-321, 1e-310, 2.0 ** -1023, np.nextafter(2.0 ** -1022, 0.0)])
    rs, _ = P.rsqrt_rcp(sub)
    lrs, _ = R.rsqrt_rcp_ld(sub)
    err = np.abs(rs - lrs) / lrs
    assert np.isfinite(rs).all() and err.max() <= EPS, f"rsqrt_nr of subnormals: {rs} (rel err {err})"
    # 0, inf, NaN: the seeds are inf / 0 there and the Newton steps make 0 * inf = NaN.  The call sites rely on exactly that and
    # select it away: angle_axis_total at |q_v|^2 = 0 (test_angle_axis_total: the identity), leg_swing_torque routes an overflowing
    # square (inf) to its reference-shaped path, rcp_nr never sees 0 or inf (positive pivots, |det| inside [eps, 1 / eps])
    rs, rc = P.rsqrt_rcp(np.array([0.0, np.inf, np.nan]))
    assert np.isnan(rs).all() and np.isnan(rc).all(), (rs, rc)


# ---------------------------------------------------------------- angle_axis_total
def _aa_inputs():
    rng = np.random.default_rng(3)
    angles = [0.0, 1e-300, 1e-160, 1e-20, 1e-12, 1e-8, 0.5, np.pi / 2, 3.0, np.pi - 1e-7, np.pi - 1e-12]
    axes = [np.eye(3)[k] for k in range(3)] + [np.array([1.0, 2.0, 3.0]), np.array([-0.3, 0.8, 0.1]), np.array([1.0, 1.0, 1.0])]
    axes += [rng.normal(size=3) for _ in range(6)]
    mats = []
    for a in angles:
        for ax in axes:
            for sgn in (1.0, -1.0):
                mats.append(R.rotation_mp(sgn * ax, a))
    # exact pi about every axis: 2 a a^T - I (rounded), and exactly about the coordinate axes
    for ax in axes:
        mats.append(R.rotation_mp(ax, mp.pi))
    for k in range(3):
        e = np.eye(3)[k]
        mats.append(2.0 * np.outer(e, e) - np.eye(3))
    # diagonal ties: m00 = m11 (about z-perpendicular axes with |ax| = |ay|), m11 = m22, all three equal
    for ax in ([1.0, 1.0, 0.3], [1.0, -1.0, 0.0], [0.2, 1.0, 1.0], [0.0, 1.0, -1.0], [1.0, 1.0, 1.0]):
        for a in (np.pi, np.pi - 1e-7, 2.5, 2.0 * np.pi / 3):
            mats.append(R.rotation_mp(ax, a))
    for _ in range(200):
        mats.append(R.rotation_mp(rng.normal(size=3), rng.uniform(0, np.pi)))
    return np.array(mats)


def test_angle_axis_total(P):
    """Same Eigen case as the 50-digit restatement of Eigen's selection; error <= 8 EPS max(1, angle) away from pi and
    <= 8 EPS / (pi - angle) near it; exact at pi about a coordinate axis; finite everywhere (a subnormal |q_v|^2 at
    ~1e-160 rad included)."""
    M = _aa_inputs()
    out = P.angle_axis(M)
    assert np.isfinite(out).all(), f"non-finite rotation log for {M[~np.isfinite(out).all(1)][:2]}"
    for m, o in zip(M, out):
        ref, angle, case = R.angle_axis_total_mp(m)
        gap = np.pi - angle
        # (an angle that rounds to pi: the gap is floored at ulp(pi), so those inputs are still held to a bar)
        bar = 8 * EPS * max(1.0, angle) if gap > 1e-3 else max(8 * EPS * np.pi, 8 * EPS / max(gap, np.spacing(np.pi)))
        err = float(np.abs(o - ref).max())
        assert err <= bar, f"angle_axis_total: err {err:.3e} > bar {bar:.3e} at angle {angle!r} (Eigen case {case})\n{m}"
    for k in range(3):
        e = np.eye(3)[k]
        o = P.angle_axis((2.0 * np.outer(e, e) - np.eye(3))[None])[0]
        assert np.array_equal(o, np.pi * e), (k, o)
    # half turns about z and x: the pivot is the one positive diagonal entry (z: m00 = m11 tie below it, decided by m22 > m00;
    # x: no tie).  Exact answers; the tie rule itself is test_angle_axis_tie_rule's
    half = np.array([[-1.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 1.0], [1.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, -1.0]])
    o = P.angle_axis(half)
    assert np.array_equal(o[0], [0.0, 0.0, np.pi]) and np.array_equal(o[1], [np.pi, 0.0, 0.0]), o
    # the identity: |q_v|^2 = 0, where rsqrt_nr(0) is not a number and angle_axis_total selects it away
    assert np.array_equal(P.angle_axis(np.eye(3)[None])[0], [0.0, 0.0, 0.0])


def test_angle_axis_tie_rule(P):
    """Eigen keeps the lower index on a diagonal tie (its tests are strict >).  On an exact tie of a non-rotation input the two
    candidate pivots give different vectors, so the device must take Eigen's: m00 = m11 > m22 with off-diagonal terms that
    make the two quaternions differ."""
    rng = np.random.default_rng(4)
    mats = []
    for _ in range(300):
        m = rng.uniform(-1, 1, (3, 3))
        d = rng.uniform(0.05, 0.9)
        i = rng.integers(0, 3); j = (i + rng.integers(1, 3)) % 3
        m[i, i] = m[j, j] = d
        k = 3 - i - j
        m[k, k] = -2.5 - rng.uniform(0, 1)  # trace < 0, the tie is the largest diagonal entry
        mats.append(m)
    mats = np.array(mats)
    out = P.angle_axis(mats.reshape(-1, 9))
    for m, o in zip(mats, out):
        ref, angle, case = R.angle_axis_total_mp(m)
        assert np.abs(o - ref).max() <= 64 * EPS * max(1.0, np.abs(ref).max()), (case, m, o, ref)


# ---------------------------------------------------------------- wraps
def test_wraps(P):
    """wrap_2PI / wrap_PI (multiplication form) and normalize_angle_2PI / PI (the reference-shaped form) land in [0, 2 pi] and
    [-pi, pi]; each within 2 ulp(2 pi) of numerics.cpp's unfused float64 arithmetic reproduced in numpy; the reference-shaped
    form is bit-identical to it (it is kept out of FMA contraction, as the reference's x86-64 build does not fuse)."""
    rng = np.random.default_rng(5)
    two_pi = 2.0 * R.PI
    edge = []
    for k in list(range(-40, 41)) + [1000, -1000, 123457, -98765]:
        edge += _ulp_walk(k * two_pi, 3)
        edge += _ulp_walk(k * two_pi + R.PI, 3)
    edge += [R.PI, -R.PI, np.nextafter(R.PI, 4), np.nextafter(-R.PI, -4), 1e15, -1e15, 0.0, -0.0]
    x = np.concatenate([np.array(edge), rng.uniform(-1e4, 1e4, 200_000), rng.uniform(-10, 10, 100_000)])
    out = P.wraps(x)
    r2, rp = R.normalize_angle_2PI_unfused(x), R.normalize_angle_PI_unfused(x)
    assert ((out[:, 0] >= 0) & (out[:, 0] <= two_pi) & (out[:, 2] >= 0) & (out[:, 2] <= two_pi)).all()
    assert ((out[:, 1] >= -R.PI) & (out[:, 1] <= R.PI) & (out[:, 3] >= -R.PI) & (out[:, 3] <= R.PI)).all()
    # The multiplication forms subtract q 2 pi with ONE rounding (an FMA); the reference rounds q 2 pi first, half an ulp of
    # |x| that the fused form does not make.  So the band is 2 ulp(2 pi) plus ulp(|x|) (1.8e-12 at 1e4, 0.125 at 1e15).
    band = 2 * np.spacing(two_pi) + np.spacing(np.abs(x))

    def circ(a, b, period):  # distance on the circle: the two ends of [0, 2 pi] are the same angle
        d = np.abs(a - b)
        return np.minimum(d, np.abs(d - period))

    for col, ref in ((0, r2), (1, rp)):
        err = circ(out[:, col], ref, two_pi)
        assert (err <= band).all(), f"wrap form {col}: {err.max():.3e} from the unfused reference at {x[np.argmax(err - band)]!r}"
    np.testing.assert_array_equal(out[:, 2], r2, err_msg="normalize_angle_2PI differs from the unfused reference arithmetic")
    np.testing.assert_array_equal(out[:, 3], rp, err_msg="normalize_angle_PI differs from the unfused reference arithmetic")
    nan = P.wraps(np.array([np.nan, np.inf, -np.inf]))
    assert np.isnan(nan).all()


def test_swing_pd_error_fast_vs_reference(P):
    """_swing_pd_error_fast_vs_reference at the default model"""
    _swing_pd_error_fast_vs_reference(P, "default")


def test_swing_pd_error_fast_vs_reference_at_the_odd_model(P):
    """_swing_pd_error_fast_vs_reference with ODD_KIN's hip and links"""
    _swing_pd_error_fast_vs_reference(P, "odd")


def _swing_pd_error_fast_vs_reference(P, model):
    """The PD error e of swing_pd<FAST> (multiplication-form wraps, Newton reciprocal) and swing_pd<false> (numerics.cpp's
    wraps, a division) agree to 2 ulp(2 pi), or both lie within 1e-14 of +-pi (a +pi / -pi flip is a torque jump of 2 pi kp:
    only allowed where the inputs sit on the branch).  kp = 1, kd = kff = 0 in the constants so the torque is e itself; hip and
    links are the model's."""
    D = P
    _set_model(D, R.KINS[model], gains=((0, 0, 0), (1, 1, 1), (0, 0, 0)))
    try:
        rng = np.random.default_rng(6)
        n = 60_000
        qr = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.2, 1.2, n), rng.uniform(-2.4, -0.4, n)], 1)
        q = qr + rng.uniform(-1e4, 1e4, (n, 3))
        q[::7] = qr[::7] + np.pi * rng.choice([-1, 1, 3, -3], (len(q[::7]), 3))  # errors near the branch
        q[::11] = qr[::11] + 2 * np.pi * rng.integers(-50, 50, (len(q[::11]), 3))
        legs = rng.integers(0, 4, n)
        tf, tr = D.swing_pd(legs, qr, q)
        assert np.isfinite(tf).all() and np.isfinite(tr).all()
        # each form carries the rounding of its wraps: 2 ulp(2 pi) and, for the reference-shaped one, half an ulp of |q| (see
        # test_wraps) on each of its three wraps
        close = np.abs(tf - tr) <= 4 * np.spacing(2 * np.pi) + 2 * np.spacing(np.maximum(np.abs(q), np.abs(qr)))
        branch = (np.abs(np.abs(tf) - np.pi) <= 1e-14) & (np.abs(np.abs(tr) - np.pi) <= 1e-14)
        assert (close | branch).all(), f"{(~(close | branch)).sum()} PD errors differ: {tf[~(close | branch)][:4]} vs {tr[~(close | branch)][:4]}"
    finally:
        _set_model(D, R.DEFAULT_KIN)


# ---------------------------------------------------------------- leg kinematics
def test_leg_fk_and_jt_force(P):
    """_leg_fk_and_jt_force_at at the default model"""
    _leg_fk_and_jt_force_at(P, "default")


def test_leg_fk_and_jt_force_at_the_odd_model(P):
    """_leg_fk_and_jt_force_at at ODD_KIN"""
    _leg_fk_and_jt_force_at(P, "odd")


def _leg_fk_and_jt_force_at(P, model):
    """leg_trig + leg_fk <= 8 EPS sum|l|; leg_jt_force (both overloads) <= 16 EPS sum|l| |f| against long double, random q in
    [-pi, pi]^3 and +-50 rad, all four legs; J^T f of the two overloads bit-identical.  At ODD_KIN every leg has its own links and
    a hip with z != 0; the bars are the same expressions of the model's links."""
    kin = R.KINS[model]
    _set_model(P, kin)
    try:
        _leg_fk_and_jt_force(P, kin)
    finally:
        _set_model(P, R.DEFAULT_KIN)


def _leg_fk_and_jt_force(P, kin):
    rng = np.random.default_rng(8)
    n = 200_000
    q = np.concatenate([rng.uniform(-np.pi, np.pi, (n // 2, 3)), rng.uniform(-50, 50, (n // 2, 3))])
    f = rng.normal(size=(n, 3)) * rng.choice([1.0, 100.0, 1e-3], (n, 1))
    legs = rng.integers(0, 4, n)
    _, p, tc, tg = P.leg(legs, q, f)
    np.testing.assert_array_equal(tc, tg)
    lsum = np.abs(kin.links).sum(1)
    for leg in range(4):
        sel = legs == leg
        pr = R.leg_fk_ld(leg, q[sel], kin)
        err = float(np.abs(p[sel] - pr).max())
        assert err <= 8 * EPS * lsum[leg], f"FK leg {leg}: {err:.3e}"
        J = R.leg_jacobian_ld(leg, q[sel], kin)
        tr = np.einsum("nij,ni->nj", J, f[sel].astype(np.longdouble))
        terr = np.abs(tc[sel] - tr).max(1) / np.abs(f[sel]).sum(1)
        assert terr.max() <= 16 * EPS * lsum[leg], f"J^T f leg {leg}: {float(terr.max()):.3e} per |f|"


def test_leg_kinematics_against_reference_notebook(P):
    """The notebook's printed numbers on the HIP path: FK of RL / RR and every leg's Jacobian, its row k as
    J^T e_k, to 6e-9 (8 printed digits)."""
    import json
    import os

    with open(os.path.join(os.path.dirname(__file__), "golden", "kinematics_notebook.json")) as fh:
        g = json.load(fh)
    q = np.array(g["q"])
    legs = np.repeat(np.arange(4), 3)
    f = np.tile(np.eye(3), (4, 1))
    _, p, tc, _ = P.leg(legs, np.tile(q, (12, 1)), f)
    for leg, name in enumerate(R.LEG_NAMES):
        if name in g["fk"]:
            np.testing.assert_allclose(p[3 * leg], g["fk"][name], atol=6e-9)
        J = tc[3 * leg:3 * leg + 3]  # row k of J = (J^T e_k)^T
        np.testing.assert_allclose(J, np.array(g["jacobian"][name]), atol=6e-9)


# ---------------------------------------------------------------- track_swing
def test_track_swing(P):
    """pos and vel against the 50-digit sextic, with t clamped exactly as std::clamp; a NaN phase stays NaN.  Bar: 4 EPS times
    the condition of evaluating the monomial form, sum_k |p_k| sum_j |basis_jk| t^j (for vel sum_j j |basis_jk| t^(j-1)).  A flat
    4 EPS max|p| does not hold for a correct evaluation: near t = 1 the monomial terms (coefficients up to 192) cancel to
    ~1e-15 at |p| ~ 0.4.  A wrong basis digit or power moves the result by orders of magnitude more than this bar."""
    B, basis = R.sextic_basis_mp()
    bas = np.abs(basis.reshape(7, 3))
    duty = 0.8 / (0.18 + 0.8)
    rng = np.random.default_rng(10)
    ph = [0.0, -0.0, np.nextafter(duty, 0), duty, np.nextafter(duty, 1), np.nextafter(1.0, 0), 1.0, np.nextafter(1.0, 2), 0.5, 1.5, -3.0]
    phase = np.concatenate([np.array(ph * 4), rng.uniform(duty, 1.0, 1500), rng.uniform(0, 1, 300)])
    n = len(phase)
    p0 = rng.uniform(-0.4, 0.4, (n, 3)); pf = rng.uniform(-0.4, 0.4, (n, 3))
    pos, vel = P.track_swing(phase, p0, pf)
    for i in range(n):
        rp, rv, t = R.track_swing_mp(B, phase[i], p0[i], pf[i], 0.08, 0.18, 0.8)
        pk = np.stack([np.abs(p0[i]), np.abs(pf[i]), np.abs([0.5 * (p0[i][0] + pf[i][0]), 0.5 * (p0[i][1] + pf[i][1]), 0.08])])  # [k, r]
        # t itself: the device fuses slope phase + y_int into one FMA, the reference rounds twice (2 EPS of the terms); the
        # condition sums grow with t, so they are taken at t + dt
        dt = 2 * EPS * (abs(phase[i]) / (1 - duty) + abs(1 - 1 / (1 - duty)))
        tu = min(t + dt, 1.0) if t < 1.0 else 1.0
        cpos = (np.array([tu ** j for j in range(7)]) @ bas) @ pk
        cvel = (np.array([j * tu ** (j - 1) if j else 0.0 for j in range(7)]) @ bas) @ pk
        cacc = (np.array([j * (j - 1) * tu ** (j - 2) if j > 1 else 0.0 for j in range(7)]) @ bas) @ pk
        assert (np.abs(pos[i] - rp) <= 4 * EPS * cpos + cvel * dt).all(), (phase[i], pos[i], rp, cpos)
        assert (np.abs(vel[i] - rv) <= 4 * EPS * cvel + cacc * dt).all(), (phase[i], vel[i], rv, cvel)
    pos, vel = P.track_swing(np.array([np.nan]), p0[:1], pf[:1])
    assert np.isnan(pos).all() and np.isnan(vel).all()


# ---------------------------------------------------------------- ldlt_solve
def _spd(rng, N, kappa):
    Q, _ = np.linalg.qr(rng.normal(size=(N, N)))
    ev = np.exp(np.linspace(0, -np.log(kappa), N))
    return (Q * ev) @ Q.T * rng.uniform(0.1, 10)


@pytest.mark.parametrize("N", [6, 12])
def test_ldlt_solve(P, N):
    """Backward error |M x - b| <= 4 N EPS |M| |x| (inf norms); forward error <= 4 N EPS kappa relative against a 50-digit
    solve; ok == false for an indefinite matrix; random SPD with kappa 1 ... 1e12."""
    rng = np.random.default_rng(11 + N)
    Ms, bs, kap = [], [], []
    for kappa in (1.0, 10.0, 1e3, 1e6, 1e9, 1e12):
        for _ in range(20):
            M = _spd(rng, N, kappa)
            M = 0.5 * (M + M.T)
            Ms.append(M); bs.append(rng.normal(size=N)); kap.append(np.linalg.cond(M))
    x, ok = P.ldlt(np.array([R.pack_lower(M) for M in Ms]), np.array(bs))
    assert ok.all()
    for M, b, k, xi in zip(Ms, bs, kap, x):
        res = float(R.residual_ld(M, xi, b).max())
        assert res <= 4 * N * EPS * np.abs(M).sum(1).max() * np.abs(xi).max(), (k, res)
        xr = R.solve_mp(M, b)
        fwd = np.abs(xi - xr).max() / np.abs(xr).max()
        assert fwd <= 4 * N * EPS * k, (k, fwd)
    # one negative eigenvalue; an exactly singular (semidefinite) matrix: not positive definite
    Q, _ = np.linalg.qr(rng.normal(size=(N, N)))
    ind = (Q * np.r_[np.ones(N - 1), -0.5]) @ Q.T
    semi = np.zeros((N, N)); semi[: N - 1, : N - 1] = np.eye(N - 1)
    _, ok = P.ldlt(np.array([R.pack_lower(0.5 * (ind + ind.T)), R.pack_lower(semi)]), np.ones((2, N)))
    assert not ok[0] and not ok[1]


# ---------------------------------------------------------------- tags and step candidates
def test_tag_and_step_cand(P):
    """tag_code(tag(v, c)) == c; the tagged value keeps its sign and lies within 31 ulp; step_cand is ~1e300 when the face cannot
    block and within 2^-22 relative of slack / nd otherwise; a negative slack ranks below every positive one; a min over tagged
    candidates that differ by more than 2^-20 relative returns the true arg-min's code."""
    vals = [5e-324, -5e-324, 1e-310, -1e-310, 1.0, -1.0, 1e300, -1e300, 3.7, -2.2e-5]
    codes = np.arange(32)
    v = np.repeat(np.array(vals), 32); c = np.tile(codes, len(vals))
    n = len(v)
    tagged, back, _ = P.tags(v, c, np.zeros(n), np.zeros(n), np.ones(n))
    np.testing.assert_array_equal(back, c)
    assert (np.signbit(tagged) == np.signbit(v)).all()
    ulps = np.abs(tagged.view(np.int64) - v.view(np.int64))
    assert ulps.max() <= 31
    rng = np.random.default_rng(12)
    m = 20_000
    slack = rng.uniform(-1, 10, m) * np.exp2(rng.uniform(-20, 20, m))
    nd = np.exp2(rng.uniform(-40, 20, m))
    ff = rng.integers(0, 2, m)
    nd[::13] = 1e-15  # below the threshold: cannot block
    code = rng.integers(0, 32, m)
    _, back, cand = P.tags(np.ones(m), code, ff, slack, nd)
    can = (ff != 0) & (nd > 1e-14) & (slack < nd)
    assert (np.abs(cand[~can] - 1e300) <= 1e300 * 2.0 ** -20).all()  # the high word of 1e300; the low word carries the code
    ratio = slack[can] / nd[can]
    assert (np.abs(cand[can] - ratio) <= np.abs(ratio) * 2.0 ** -22 + 2.0 ** -1022).all()
    assert (cand.view(np.int64) & 31 == code).all()
    neg = cand[can & (slack < 0)]
    pos = cand[can & (slack > 0)]
    if len(neg) and len(pos):
        assert neg.max() < pos.min()
    # arg-min over sets of 16 well-separated candidates, as the device's v_min trees see them
    sets = np.exp2(rng.uniform(-10, 10, (500, 16))) * np.where(rng.random((500, 16)) < 0.1, -1, 1)
    ok_sets = [s for s in sets if np.all(np.abs(np.diff(np.sort(s))) > 2.0 ** -20 * np.abs(np.sort(s))[1:])]
    sets = np.array(ok_sets)
    codes = np.tile(np.arange(16), len(sets))
    tagged, _, _ = P.tags(sets.ravel(), codes, np.zeros(codes.size), np.zeros(codes.size), np.ones(codes.size))
    tagged = tagged.reshape(sets.shape)
    assert ((tagged.min(1).view(np.int64) & 31) == sets.argmin(1)).all()


# ---------------------------------------------------------------- lane-group reductions
@pytest.mark.parametrize("G,S", [(2, False), (4, True)])
def test_group_reductions(P, G, S):
    """One value per lane over whole waves: sum within (G - 1) EPS sum|v| of the exact sum, min / max / or exact, and every
    member of a group holding the bit-identical result (commander_step and the lane-group kernels rely on that)."""
    rng = np.random.default_rng(13 + G + S)
    waves = 64
    n = 64 * waves
    v = rng.normal(size=n) * np.exp2(rng.integers(-60, 60, n))
    v[::17] = 0.0; v[5::17] = -0.0
    v[: 64] = rng.normal(size=64)  # one plain wave
    add = np.repeat(rng.normal(size=n // 4), 4) if not S else rng.normal(size=n)
    bits = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32) & rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    lane = np.arange(n) % 64
    wave = np.arange(n) // 64
    gid = wave * 64 + ((lane & 15) if S else (lane // G))
    if S:  # the addend of group_sum_add is group-uniform
        add = add[wave * 64 + (lane & 15)]
    else:
        add = add[wave * 64 + (lane // G) * G]
    s, sa, mn, mx, orr = P.group(G, S, v, add, bits)
    for g in np.unique(gid):
        idx = np.nonzero(gid == g)[0]
        assert len(idx) == G
        for arr in (s, sa, mn, mx):
            assert len(set(arr[idx].view(np.int64).tolist())) == 1, f"group {g}: members disagree {arr[idx]}"
        assert len(set(orr[idx].tolist())) == 1
        ex = R.exact_sum(v[idx])
        bar = (G - 1) * EPS * np.abs(v[idx]).sum()
        assert abs(s[idx[0]] - ex) <= bar, (v[idx], s[idx[0]], ex)
        exa = R.exact_sum(list(v[idx]) + [add[idx[0]]])
        assert abs(sa[idx[0]] - exa) <= G * EPS * (np.abs(v[idx]).sum() + abs(add[idx[0]])), (v[idx], add[idx[0]], sa[idx[0]])
        assert mn[idx[0]] == v[idx].min() and mx[idx[0]] == v[idx].max()
        assert orr[idx[0]] == np.bitwise_or.reduce(bits[idx])


# ---------------------------------------------------------------- pinv3_apply
def _pinv_cases(rng):
    Js, ranks = [], []
    for _ in range(100):  # a stretched knee (q3 = 0): the knee column parallel to the hip-pitch column, rank 2
        leg = int(rng.integers(0, 4))
        q = np.array([[rng.uniform(-0.6, 0.6), rng.uniform(-1.0, 1.4), 0.0]])
        Js.append(np.asarray(R.leg_jacobian_ld(leg, q)[0], np.float64)); ranks.append(2)
    for _ in range(60):  # rank 1: an outer product (the lateral clamp acting as well leaves one direction)
        u, v = rng.normal(size=3), rng.normal(size=3)
        Js.append(np.outer(u, v)); ranks.append(1)
    for _ in range(40):  # second pivot at 1e-9 of the first, x (1 +- 1e-3): exact pivots (a signed permutation of a diagonal)
        for f, rk in ((1.001, 2), (0.999, 1)):
            s = 10.0 ** rng.uniform(-2, 2)
            D = np.diag([s, s * 1e-9 * f, 0.0])
            Pm = np.eye(3)[rng.permutation(3)] * rng.choice([-1, 1], 3)
            Qm = np.eye(3)[rng.permutation(3)] * rng.choice([-1, 1], 3)
            Js.append(Pm @ D @ Qm); ranks.append(rk)
    return np.array(Js), np.array(ranks)


def test_pinv3_apply(P):
    """pinv3_apply = the pseudo-inverse truncated to the rank its complete-pivoting rule chooses (at most 2; a second pivot
    only above 1e-9 of the first) to 1e-13 relative against the 50-digit SVD pseudo-inverse of that rank."""
    rng = np.random.default_rng(14)
    J, ranks = _pinv_cases(rng)
    v = rng.normal(size=(len(J), 3))
    x = P.pinv3(J, v)
    for Ji, vi, xi, rk in zip(J, v, x, ranks):
        with mp.workdps(R.DPS):
            Pm = R.pinv_mp(Ji, rk)
            ref = np.array([float(sum(Pm[r, c] * R.mpf(vi[c]) for c in range(3))) for r in range(3)])
            other = R.pinv_mp(Ji, 3 - rk)
            alt = np.array([float(sum(other[r, c] * R.mpf(vi[c]) for c in range(3))) for r in range(3)])
        assert np.abs(xi - ref).max() <= 1e-13 * np.abs(ref).max(), (rk, Ji, xi, ref)
        assert np.abs(xi - alt).max() > 1e-6 * np.abs(ref).max(), ("the other rank gives the same answer: not a rank test", rk, Ji)


# ---------------------------------------------------------------- leg_swing_torque
def _swing_cases(rng, kin=R.DEFAULT_KIN):
    legs, pb = [], []
    for _ in range(300):  # inside the workspace: FK of a knee-bent posture
        leg = int(rng.integers(0, 4))
        q = np.array([[rng.uniform(-0.6, 0.6), rng.uniform(-0.2, 1.4), rng.uniform(-2.4, -0.3)]])
        legs.append(leg); pb.append(np.asarray(R.leg_fk_ld(leg, q, kin)[0], np.float64))
    for leg in range(4):  # near full stretch: the knee cosine d = 1 - k 2^-53 (to the rounding of the target), k <= 8
        for k in range(1, 9):
            q3 = -math.sqrt(2.0 * k * 2.0 ** -53)
            q = np.array([[rng.uniform(-0.3, 0.3), rng.uniform(0.0, 0.8), q3]])
            legs.append(leg); pb.append(np.asarray(R.leg_fk_ld(leg, q, kin)[0], np.float64))
    for leg in range(4):  # the foot near the hip's x axis (rho^2 -> 0, rt -> 0 after the lateral clamp)
        for r in (1e-3, 1e-6):
            hip = kin.hip[leg]
            legs.append(leg); pb.append(hip + np.array([0.2, r, -r]))
    for _ in range(12):  # out of reach: d clamped to 1, q3 = 0, J of rank 2 (the pseudo-inverse inside swing_pd)
        leg = int(rng.integers(0, 4))
        u = rng.normal(size=3); u /= np.linalg.norm(u)
        legs.append(leg); pb.append(kin.hip[leg] + u * rng.uniform(0.6, 2.0))
    for leg in range(4):  # fully folded: d = -1 exactly (u = 0, q3 = pi), again the pseudo-inverse
        p = _folded_target(leg, rng, kin)
        legs.append(leg); pb.append(p)
    return np.array(legs), np.array(pb)


def _folded_target(leg, rng, kin=R.DEFAULT_KIN):
    """A target whose float64 knee cosine is exactly -1: |p - hip|^2 = l1^2 + (l2 - l3)^2, walked by ulps until it rounds there"""
    l1, l2, l3 = np.abs(kin.links[leg])
    rad = math.sqrt(l1 * l1 + (l2 - l3) ** 2)
    phi = rng.uniform(-2.5, -0.6)  # x = 0 relative to the hip, (y, z) on a circle outside the lateral offset l1
    p = kin.hip[leg] + rad * np.array([0.0, math.cos(phi), math.sin(phi)])
    for _ in range(4000):
        d = R.knee_cosine_double(leg, p, kin)
        if d == -1.0:
            return p
        outward = np.sign(p[2] - kin.hip[leg][2])  # |z - hip_z| grows with z moved this way
        p = p.copy(); p[2] = np.nextafter(p[2], outward * np.inf if d < -1.0 else -outward * np.inf)
    raise AssertionError("no target with d = -1 found")


def test_leg_swing_torque(P):
    """_leg_swing_torque_at at the default model"""
    _leg_swing_torque_at(P, "default")


def test_leg_swing_torque_at_the_odd_model(P):
    """_leg_swing_torque_at at ODD_KIN"""
    _leg_swing_torque_at(P, "odd")


def _leg_swing_torque_at(P, model):
    """The trig-free swing-leg torque against a 50-digit legInverseKinematics -> legJacobian^-1 -> joint PD.  Bar:
    c EPS cond(J) (|kp| pi + |kd| (|J^-1 vb| + |qdot|)) with c = 64: the IK angles carry a few ulps of the target (~8 roundings
    of lengths of order sum|l|), the inverse amplifies them by cond(J), and the rest is a dozen rounded products; 64 leaves ~4x
    over the accumulation of ~16 rounding steps, far below the 1e-9 ... 1e-6 a wrong formula gives.  For a singular J (out of
    reach, folded) the inverse is the rank-2 pseudo-inverse and cond is sigma_1 / sigma_2.
    The knee cosine d is the one input whose conditioning cond(J) does not cover: near full stretch q3 ~ -sqrt(2 (1 - d)), so one
    ulp of d moves q3, and J^-1 vb with it, by a fraction 1 / k of itself at d = 1 - k 2^-53.  The reference rounds d in float64,
    every operation on its own, and the device computes it the same way (ik_knee_num, a true division), so the reference is
    evaluated at that double d and the device must agree with it there, with no allowance for another d.
    At ODD_KIN the cases - the knee-cosine boundary ones among them - are rebuilt from the model's hip and links, and the gains
    in the bar are the model's (kff adds one exact term)."""
    kin = R.KINS[model]
    _set_model(P, kin)
    try:
        _leg_swing_torque(P, kin)
    finally:
        _set_model(P, R.DEFAULT_KIN)


def _leg_swing_torque(P, kin):
    rng = np.random.default_rng(15)
    legs, pb = _swing_cases(rng, kin)
    n = len(legs)
    vb = rng.normal(size=(n, 3)) * 0.5
    q = rng.uniform(-np.pi, np.pi, (n, 3))
    qdot = rng.normal(size=(n, 3))
    tau = P.swing_torque(legs, pb, vb, q, qdot)
    saw = dict(pinv=0, folded=0)
    for i in range(n):
        d0 = min(R.knee_cosine_double(int(legs[i]), pb[i], kin), 1.0)
        ref, cond, _, qdn = R.swing_torque_mp(int(legs[i]), pb[i], vb[i], q[i], qdot[i], d=d0, kin=kin)
        saw["pinv"] += d0 == 1.0
        saw["folded"] += d0 == -1.0
        bar = 64 * EPS * cond * (max(kin.jc_kp) * np.pi + max(kin.jc_kd) * (qdn + np.abs(qdot[i]).max()))
        err = float(np.abs(tau[i] - ref).max())
        assert err <= bar, f"leg {legs[i]} target {pb[i]!r}: err {err:.3e} > {bar:.3e} (cond {cond:.3e})"
    assert saw["pinv"] >= 12 and saw["folded"] == 4, saw


# ---------------------------------------------------------------- wrench_from_state, plan_foothold
def _wrench_setup(P, seed, kin=R.DEFAULT_KIN):
    """The probe's constants with every quirk of the wrench law visible (device_math_reference._wrench_params: kff[3..5] all
    different and non-zero, a full non-diagonal Ib, non-uniform gains) and a planner; returns (params dict, restore())."""

    rng = np.random.default_rng(seed)
    W = R._wrench_params(rng)
    W["planner_hip"] = (R.HIP + rng.uniform(-0.01, 0.01, (4, 3))).reshape(12)
    W["planner_k"] = 0.07
    _, basis = R.sextic_basis_mp()
    P.set_params(kin.hip, kin.links, kin.jc_kff, kin.jc_kp, kin.jc_kd, basis, 0.18, 0.31, 0.08, wrench=W)
    return W, lambda: P.set_params(R.HIP, R.LINKS, R.JC_KFF, R.JC_KP, R.JC_KD, basis, 0.18, 0.8, 0.08)


def _check_wrench(P, W, b, fp, kin, sample, tag, model=R.DEFAULT_KIN):
    """b and r of the probe against wrench_ld on every state and wrench_mp on `sample`; returns the worst error / bar"""
    bd, rd, fin = P.wrench(b, fp, kin)
    assert np.array_equal(fin, np.zeros_like(fin)), (tag, fin[fin != 0][:4])
    ref = R.wrench_ld(W, b, fp, kin=(model.hip, model.links) if kin else None)
    worst = 0.0
    for got, (val, cond, cnt) in ((bd, ref["b"]), (rd, ref["r"])):
        ratio = np.abs(got.astype(np.longdouble) - val) / (cnt * EPS * cond)
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, (tag, kin, float(ratio.max()), np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    for i in sample:
        m = R.wrench_mp(W, {k: v[i] for k, v in b.items()}, fp[i], kin=(model.hip, model.links) if kin else None)
        for got, (val, cond, cnt) in ((bd[i], m["b"]), (rd[i], m["r"])):
            ratio = np.abs(got - val) / (cnt * EPS * cond)
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (tag, kin, int(i), float(ratio.max()))
    return worst


def test_wrench_from_state(P):
    """b [6] and r [4][3] of wrench_from_state<4, false> and <4, true> against BC.cpp:126-139, 244-269 at 50 digits (edge set and a
    2 000-state sample) and in long double (100 000 random states), entry by entry within count * EPS * condition sum
    (device_math_reference.Tr: the count is the number of roundings on the entry's longest chain - 5 or 6 for the linear part, 3 for
    r, 22 for the angular part, where the rotation log enters with its own pinned 8 EPS max(1, angle) plus the sensitivity of the log
    map to the <= 3 roundings of each entry of Re = Rwb_d Rwb^T, measured by perturbing Re in the reference's precision).  The
    parameters make the `sic` index (kff5 w_d2 on row 1), a transposed Iw and swapped gains visible (test_device_math_cpu shows each
    of them far outside these bars).  Rotation errors stay below pi - 1e-3; beyond it test_angle_axis_total's domain applies."""

    W, restore = _wrench_setup(P, 31)
    try:
        rng = np.random.default_rng(32)
        n = 100_000
        b = R._wrench_states(rng, n, max_angle=np.pi - 1e-3)
        feet = b.pop("feet")
        qj = np.stack([rng.uniform(-0.6, 0.6, (n, 4)), rng.uniform(-0.2, 1.4, (n, 4)), rng.uniform(-2.4, -0.3, (n, 4))], 2).reshape(n, 12)
        sample = rng.choice(n, 2000, replace=False)
        w0 = _check_wrench(P, W, b, feet, False, sample, "random")
        w1 = _check_wrench(P, W, b, qj, True, sample, "random")
        # edge set: rotation errors 0, 1e-9, pi/2, pi - 1e-3 about coordinate and general axes; x_d - x = 1e-12 next to |x| = 1e3
        from scipy.spatial.transform import Rotation

        rows = []
        for ang in (0.0, 1e-9, np.pi / 2, 3.0, np.pi - 1e-3):
            for ax in (np.eye(3)[0], np.eye(3)[1], np.eye(3)[2], np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0), np.array([-0.3, 0.8, 0.1])):
                for base in (np.eye(3), Rotation.from_euler("ZYX", [0.7, -0.4, 1.1]).as_matrix()):
                    rows.append((base, R.rotation_mp(ax, ang) @ base if ang else base.copy()))
        m = len(rows)
        e = {k: v[:m].copy() for k, v in b.items()}
        e["Rwb"] = np.array([r[0].reshape(9) for r in rows])
        e["Rwb_d"] = np.array([r[1].reshape(9) for r in rows])
        e["x"][: m // 2] = np.array([1e3, -1e3, 1e3]) * rng.uniform(0.5, 1.0, (m // 2, 3))
        e["x_d"][: m // 2] = e["x"][: m // 2] + 1e-12
        w2 = _check_wrench(P, W, e, feet[:m], False, range(m), "edge")
        w3 = _check_wrench(P, W, e, qj[:m], True, range(m), "edge")
        # a zero rotation error (Rwb_d == Rwb == I: Re = I exactly): e = 0 exactly, so b[3:] must not move when kp_w does
        same = [i for i in range(m) if np.array_equal(e["Rwb"][i], np.eye(3).reshape(9)) and np.array_equal(e["Rwb_d"][i], np.eye(3).reshape(9))]
        assert len(same) == 5
        bd, _, _ = P.wrench(e, feet[:m], False)
        W2 = dict(W, kp_w=np.zeros(3))
        _, basis = R.sextic_basis_mp()
        P.set_params(R.HIP, R.LINKS, R.JC_KFF, R.JC_KP, R.JC_KD, basis, 0.18, 0.31, 0.08, wrench=W2)
        bd0, _, _ = P.wrench(e, feet[:m], False)
        assert np.array_equal(bd[same], bd0[same]) and not np.array_equal(bd[:, 3:], bd0[:, 3:])
        print(f"wrench_from_state: worst error / bar: random {w0:.3f} (feet) {w1:.3f} (joint angles), edge set {w2:.3f} {w3:.3f}")
    finally:
        restore()


def test_wrench_from_state_with_joint_angles_at_the_odd_model(P):
    """The KIN = true wrench (the feet through forwardKinematics) with ODD_KIN's hip and links in the probe's constants: 20 000 random
    states in long double, 200 of them and the rotation edge set at 50 digits, the same count * EPS * condition-sum bars; the
    defaults are restored afterwards."""
    kin = R.ODD_KIN
    W, restore = _wrench_setup(P, 31, kin)
    try:
        rng = np.random.default_rng(33)
        n = 20_000
        b = R._wrench_states(rng, n, max_angle=np.pi - 1e-3)
        b.pop("feet")
        qj = np.stack([rng.uniform(-0.6, 0.6, (n, 4)), rng.uniform(-0.2, 1.4, (n, 4)), rng.uniform(-2.4, -0.3, (n, 4))], 2).reshape(n, 12)
        w1 = _check_wrench(P, W, b, qj, True, rng.choice(n, 200, replace=False), "random, odd model", kin)
        from scipy.spatial.transform import Rotation

        rows = [(base, R.rotation_mp(ax, ang) @ base if ang else base.copy()) for ang in (0.0, 1e-9, np.pi / 2, np.pi - 1e-3)
                for ax in (np.eye(3)[2], np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)) for base in (np.eye(3), Rotation.from_euler("ZYX", [0.7, -0.4, 1.1]).as_matrix())]
        m = len(rows)
        e = {k: v[:m].copy() for k, v in b.items()}
        e["Rwb"], e["Rwb_d"] = np.array([r[0].reshape(9) for r in rows]), np.array([r[1].reshape(9) for r in rows])
        w3 = _check_wrench(P, W, e, qj[:m], True, range(m), "edge, odd model", kin)
        # the model matters: the default geometry's lever arms on the same angles are centimetres away
        _, rd, _ = P.wrench(b, qj, True)
        assert np.abs(rd.reshape(n, -1) - np.asarray(R.wrench_ld(W, b, qj, kin=(R.HIP, R.LINKS))["r"][0], np.float64).reshape(n, -1)).max() > 0.01
        print(f"wrench_from_state at the odd model: worst error / bar: random {w1:.3f}, edge set {w3:.3f}")
    finally:
        restore()


def test_wrench_finiteness_value(P):
    """The value wrench_from_state returns is exactly 0.0 for finite inputs - up to 1e150 in every input at once - and non-zero (or
    NaN) as soon as ONE entry of an input that reaches b, r or R is NaN or Inf: each of Rwb, Rwb_d, x, x_d, xdot, xdot_d, w, w_d and the
    feet / joint angles in turn, both variants."""

    W, restore = _wrench_setup(P, 33)
    try:
        rng = np.random.default_rng(34)
        names = ("Rwb", "Rwb_d", "x", "x_d", "xdot", "xdot_d", "w", "w_d", "fp")
        rows = [(name, k, bad) for name in names for k in ((0, 4, 8) if name.startswith("Rwb") else (0, 2, 7, 11) if name == "fp" else (0, 1, 2)) for bad in (np.nan, np.inf, -np.inf)]
        m = len(rows)
        b = R._wrench_states(rng, m, max_angle=2.0)
        feet = b.pop("feet")
        qj = np.stack([rng.uniform(-0.6, 0.6, (m, 4)), rng.uniform(-0.2, 1.4, (m, 4)), rng.uniform(-2.4, -0.3, (m, 4))], 2).reshape(m, 12)
        for kin, fp in ((False, feet), (True, qj)):
            _, _, fin = P.wrench(b, fp, kin)
            assert np.array_equal(fin, np.zeros(m)) and not np.signbit(fin).any()
            bb = {k: v.copy() for k, v in b.items()}
            ff = fp.copy()
            for i, (name, k, bad) in enumerate(rows):
                (ff if name == "fp" else bb[name])[i, k] = bad
            _, _, fin = P.wrench(bb, ff, kin)
            assert (fin != 0.0).all(), [rows[i] for i in np.nonzero(fin == 0.0)[0]]
        big = {k: (v if k.startswith("Rwb") else np.sign(v) * 1e150) for k, v in b.items()}
        bd, rd, fin = P.wrench(big, np.sign(feet) * 1e150, False)
        assert np.array_equal(fin, np.zeros(m)) and np.isfinite(bd).all() and np.isfinite(rd).all()
        for name in names[2:-1]:
            one = dict(b, **{name: big[name]})
            for kin, fp in ((False, feet), (True, qj)):
                assert np.array_equal(P.wrench(one, fp, kin)[2], np.zeros(m)), (name, kin)
    finally:
        restore()


def test_plan_foothold(P):
    """plan_foothold against foot_planner.cpp:76-104 at 50 digits (a 1 000-case sample) and in long double (100 000 cases): x and y
    within count * EPS * sum |terms| (count 7 as Tr counts it: the thigh position 4, then the three sums of the four-term sum), z == 0 exactly.
    A height of 0 or -0 drops the pendulum term and nothing else; a negative height is NaN in x and y like the reference's
    std::sqrt, z still 0."""
    from scipy.spatial.transform import Rotation

    W, restore = _wrench_setup(P, 35)
    try:
        rng = np.random.default_rng(36)
        n = 100_000
        legs = rng.integers(0, 4, n)
        Rw = Rotation.random(n, random_state=5).as_matrix().reshape(n, 9)
        x = np.stack([rng.normal(size=n) * 10, rng.normal(size=n) * 10, rng.uniform(0.02, 0.8, n)], 1)
        xdot, w, xdd, pc = rng.normal(size=(n, 3)) * 2, rng.normal(size=(n, 3)) * 3, rng.normal(size=(n, 3)) * 2, rng.uniform(-0.5, 0.5, (n, 3))
        fh = P.foothold(legs, Rw, x, xdot, w, xdd, pc)
        hips = W["planner_hip"].reshape(4, 3)[legs]
        val, cond, cnt = R.foothold_ld(hips, W["planner_k"], 0.31, Rw, x, xdot, w, xdd, pc, foot_is_lever=True)
        assert (fh[:, 2] == 0.0).all() and not np.signbit(fh[:, 2]).any()
        ratio = np.abs(fh[:, :2].astype(np.longdouble) - val[:, :2]) / (cnt[:, :2] * EPS * cond[:, :2])
        assert cnt[:, :2].max() == 7 and ratio.max() <= 1.0, (float(ratio.max()), int(cnt.max()))
        worst = float(ratio.max())
        for i in rng.choice(n, 1000, replace=False):
            v, c, k = R.foothold_mp(hips[i], W["planner_k"], 0.31, Rw[i], x[i], xdot[i], w[i], xdd[i], pc[i], foot_is_lever=True)
            r = np.abs(fh[i, :2] - v[:2]) / (k[:2] * EPS * c[:2])
            worst = max(worst, float(r.max()))
            assert r.max() <= 1.0, (int(i), float(r.max()))
        print(f"plan_foothold: worst error / bar {worst:.3f}")
        # heights 0, -0, negative
        m = 12
        xe = x[:m].copy()
        xe[:4, 2], xe[4:8, 2], xe[8:, 2] = 0.0, -0.0, -rng.uniform(0.01, 1.0, 4)
        fe = P.foothold(legs[:m], Rw[:m], xe, xdot[:m], w[:m], xdd[:m], pc[:m])
        assert (fe[:, 2] == 0.0).all() and np.isnan(fe[8:, :2]).all() and np.isfinite(fe[:8, :2]).all()
        for i in range(8):  # sqrt(+-0 / g) = +-0: the pendulum term is +-0 xdot
            xi = xe[i].copy()
            xi[2] = 1e-300  # (the reference takes a positive height: 0.5 sqrt(1e-300 / g) |xdot| = 1e-150, far below the bar)
            v, c, k = R.foothold_mp(hips[i], W["planner_k"], 0.31, Rw[i], xi, xdot[i], w[i], xdd[i], pc[i], foot_is_lever=True)
            assert np.all(np.abs(fe[i, :2] - v[:2]) <= k[:2] * EPS * c[:2])
    finally:
        restore()
