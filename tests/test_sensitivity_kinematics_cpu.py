"""CPU: the joint-angle cotangents' restatement (tests/sensitivity_kinematics_restatement.py) against central differences of its own
forward kinematics and of the clamped torque map at 50 digits and beyond, its float64 evaluation against its 50-digit one, the oracle's
tick under the finite-difference keep rule of the GPU test, and the C ABI of qc_sensitivity_kin_batch as far as it goes without a device.

Measured (committed seeds): test_restatement_against_50_digits prints the float64 restatement's worst error / (EPS terms) over the
40-robot case of both mask sources: grf_bar 0.72, joint_q_bar 1.00.  The GPU test's bar against 50 digits is derived from the
figure that test measures in the same session (4 x, floor 64 EPS of the output's scale)."""
import ctypes
import os
import subprocess

import mpmath as mp
import numpy as np
import pytest

import quadruped_control_amd as q
from tests import device_math_reference as DMR
from tests import sensitivity_kinematics_restatement as KN
from tests.fd_support import FD_H, N_FD

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EPS = 2.0 ** -52
ANGLES = ([0.0, 0.8, -1.6], [0.21, 0.63, -1.41], [-0.25, 1.05, -1.85], [1.3, -2.1, 0.4], [-2.9, 0.05, 3.0])


def test_jacobian_and_hessian_against_differences_of_the_forward_kinematics():
    """J and H of the restatement - made by differentiating the monomials of its forward kinematics - against first and second
    central differences of that forward kinematics itself, every leg (the left and right link signs differ) at five angle triples,
    at 80 digits with h = 1e-20: truncation h^2 = 1e-40 of the third / fourth derivatives (link lengths: < 1), rounding 1e-80 / h^2
    = 1e-40.  Bar 1e-30, far below the ~1e-20 that would settle it.  This is also the check of the issue's table of H: the kernel's
    G = sum_r g_r H_r is compared with this H through the restatement on the GPU."""
    with mp.workdps(80):
        h = mp.mpf(10) ** -20
        for leg in range(4):
            for a in ANGLES:
                q0 = [KN.lift(v) for v in a]
                p = lambda d: KN.geometry_mp(leg, [q0[k] + d[k] for k in range(3)])[0]
                _, J, H = KN.geometry_mp(leg, q0)
                e = lambda c, k=None, sc=1, sk=1: [(sc * h if j == c else 0) + (sk * h if j == k else 0) for j in range(3)]
                for c in range(3):
                    pp, pm = p(e(c)), p(e(c, sc=-1))
                    for r in range(3):
                        assert abs((pp[r] - pm[r]) / (2 * h) - J[r][c]) < mp.mpf(10) ** -30, (leg, a, r, c)
                    for k in range(3):
                        f = [p(e(c, k, sc, sk)) for sc, sk in ((1, 1), (1, -1), (-1, 1), (-1, -1))]
                        for r in range(3):
                            fd = (f[0][r] - f[1][r] - f[2][r] + f[3][r]) / (4 * h * h)
                            assert abs(fd - H[r][c][k]) < mp.mpf(10) ** -30, (leg, a, r, c, k)
                            assert H[r][c][k] == H[r][k][c]


def test_issue_table_of_the_second_derivatives():
    """The table of H the kernel's header states (a = l2 c2 + l3 c23, b = l2 s2 + l3 s23, d = l3 c23, e = l3 s23) against the H
    differentiated from the monomials, in float64 to 8 EPS of the entry's magnitude."""
    for leg in range(4):
        l1, l2, l3 = DMR.LINKS[leg]
        for ang in ANGLES:
            geo = KN.geometry(np.tile(np.asarray(ang), 4))
            H, aH = geo["H"][0, leg], geo["aH"][0, leg]
            s1, c1, s2, c2 = np.sin(ang[0]), np.cos(ang[0]), np.sin(ang[1]), np.cos(ang[1])
            s23, c23 = np.sin(ang[1] + ang[2]), np.cos(ang[1] + ang[2])
            a, b, d, e = l2 * c2 + l3 * c23, l2 * s2 + l3 * s23, l3 * c23, l3 * s23
            table = {(0, 0): (0.0, s1 * a - l1 * c1, -l1 * s1 - c1 * a), (0, 1): (0.0, c1 * b, s1 * b), (0, 2): (0.0, c1 * e, s1 * e),
                     (1, 1): (-b, s1 * a, -c1 * a), (1, 2): (-e, s1 * d, -c1 * d), (2, 2): (-e, s1 * d, -c1 * d)}
            for (c, k), col in table.items():
                for r in range(3):
                    assert abs(H[r, c, k] - col[r]) <= 8 * EPS * aH[r, c, k] and H[r, c, k] == H[r, k, c], (leg, ang, r, c, k)


@pytest.fixture(scope="module")
def legs():
    """The legs of the 40-robot case (stance bytes): every contact pattern, failed robots, the tight limits."""
    b, grf, status, cot = KN.case(40, "stance")
    ref = KN.kin_cotangents(b, grf, status, KN.TAU_MIN, KN.TAU_MAX, **cot)
    return dict(b=b, grf=grf, status=status, cot=cot, ref=ref)


def test_restatement_against_differences_of_the_clamped_torque_map(legs):
    """The full restatement at 50 digits, <joint_q_bar, v> and <grf_bar, u>, against central differences (h = 1e-20: truncation 1e-40,
    rounding 1e-30) of L(q, g) = <joint_tau_bar, clamp(J(q)^T g)> + <feet_bar, FK(q)> + <grf_bar_in, g> + <joint_q_bar_in, q>
    at 50 digits along committed directions, over all four legs of the first 32 robots of the 40-robot case: both clamp branches,
    pass-through, swing legs and failed robots are among them (asserted), and the pass-through mask of the float64 restatement is the
    50-digit one at every point (no torque within 1e-20 of a limit).  Bar 1e-25 of the terms."""
    c = legs
    n = 40
    ref = c["ref"]
    raw, emit = ref["tau_raw"], ref["emit"]
    assert (raw[emit] < KN.TAU_MIN).any() and (raw[emit] > KN.TAU_MAX).any() and ref["mask"].any() and (~emit).any()
    assert (c["status"] != 0).any() and all((emit[:32, l]).any() for l in range(4))
    arr = lambda k: np.asarray(c["cot"][k]).reshape(n, 4, 3)
    qq, gg = c["b"]["joint_q"].reshape(n, 4, 3), c["grf"].reshape(n, 4, 3)
    rng = np.random.default_rng(31)
    with mp.workdps(DMR.DPS):
        h = mp.mpf(10) ** -20
        lo, hi = KN.lift(KN.TAU_MIN), KN.lift(KN.TAU_MAX)
        for i in range(32):
            for l in range(4):
                v, u = rng.normal(size=3), rng.normal(size=3)
                q0, g0 = [KN.lift(x) for x in qq[i, l]], [KN.lift(x) for x in gg[i, l]]
                cots = [[KN.lift(x) for x in arr(k)[i, l]] for k in ("joint_tau_bar", "feet_bar", "grf_bar_in", "joint_q_bar_in")]
                at = lambda t: KN.loss_mp(l, [q0[k] + t * KN.lift(v[k]) for k in range(3)], [g0[k] + t * KN.lift(u[k]) for k in range(3)],
                                          bool(emit[i, l]), lo, hi, *cots)
                (lp, mp_), (lm, mm), (_, m0) = at(h), at(-h), at(0)
                assert mp_ == mm == m0 == ref["mask"][i, l].tolist(), (i, l)
                grf_bar, q_bar = KN.kin_cotangents_mp(l, qq[i, l], gg[i, l], m0, *(arr(k)[i, l] for k in ("joint_tau_bar", "feet_bar", "grf_bar_in", "joint_q_bar_in")))
                an = sum(q_bar[k] * KN.lift(v[k]) + grf_bar[k] * KN.lift(u[k]) for k in range(3))
                scale = float((ref["terms"]["joint_q_bar"][i, l] * np.abs(v)).sum() + (ref["terms"]["grf_bar"][i, l] * np.abs(u)).sum())
                assert abs((lp - lm) / (2 * h) - an) <= 1e-25 * max(scale, 1e-300), (i, l)


def test_restatement_against_50_digits(legs):
    """The float64 restatement's own distance from its 50-digit evaluation over every leg of the 40-robot case, both mask sources:
    the worst error / (EPS terms) is printed - measured 0.72 (grf_bar) and 1.00 (joint_q_bar) - and held to 16: per monomial two
    sines or cosines at 1 EPS each, the rounding of q1 + q2 inside them (<= |q1 + q2| |cot| <= 4.5 EPS of the monomial at these
    angles), three products at 1/2 EPS, and the sums of up to 27 products behind them."""
    worst = {k: 0.0 for k in KN.OUTPUTS}
    for source in ("stance", "phase"):
        b, grf, status, cot = KN.case(40, source)
        ref = KN.kin_cotangents(b, grf, status, KN.TAU_MIN, KN.TAU_MAX, **cot)
        per_terms, _ = KN.worst_against_50_digits(b, grf, ref, ref, **cot)
        worst = {k: max(worst[k], per_terms[k]) for k in KN.OUTPUTS}
    print("restatement against 50 digits, worst error / (EPS terms):", worst)
    assert all(v <= 16.0 for v in worst.values()), worst


def test_restatement_against_50_digits_at_the_odd_model():
    """The same measurement at ODD_KIN (hip, links) with the limits (ODD_TAU_MIN, ODD_TAU_MAX), both mask sources: error / (EPS terms)
    held to the same 16, and the distance relative to the leg's largest entry recorded as KN.C_KIN_ODD.  The pool's conditions, on the
    restatement alone: at every size the GPU test uses from 15 on, every joint is clamped at tau_min, clamped at tau_max and passes at
    least once, no torque lies within 1e-9 of a limit, and the clamped share stays between 10 % and 90 % from n = 16 on."""
    K = DMR.ODD_KIN
    lo, hi = KN.ODD_TAU_MIN, KN.ODD_TAU_MAX
    assert lo != -hi
    for n in (15, 16, 17, 40):
        b, grf, status, cot = KN.case(n, "stance")
        ref = KN.kin_cotangents(b, grf, status, lo, hi, kin=K, **cot)
        raw, emit = ref["tau_raw"], ref["emit"]
        for c in range(3):
            r = raw[..., c][emit]
            assert (r < lo).any() and (r > hi).any() and ref["mask"][..., c].any(), (n, c)
        assert np.abs(raw - lo).min() > 1e-9 and np.abs(raw - hi).min() > 1e-9
        assert n < 16 or 0.1 <= 1.0 - ref["mask"][emit].mean() <= 0.9
    worst, mag = {k: 0.0 for k in KN.OUTPUTS}, {k: 0.0 for k in KN.OUTPUTS}
    for source in ("stance", "phase"):
        b, grf, status, cot = KN.case(40, source)
        ref = KN.kin_cotangents(b, grf, status, lo, hi, kin=K, **cot)
        per_terms, per_mag = KN.worst_against_50_digits(b, grf, ref, ref, kin=K, **cot)
        worst = {k: max(worst[k], per_terms[k]) for k in KN.OUTPUTS}
        mag = {k: max(mag[k], per_mag[k] / EPS) for k in KN.OUTPUTS}
    print("odd model, restatement against 50 digits: error / (EPS terms)", worst, "EPS of the largest entry", mag)
    assert all(v <= 16.0 for v in worst.values()), worst
    assert all(mag[k] <= KN.C_KIN_ODD[k] for k in KN.OUTPUTS), mag
    # the model matters: the default geometry on the same inputs is far from the odd one
    dflt = KN.kin_cotangents(b, grf, status, lo, hi, **cot)
    assert np.abs(dflt["joint_q_bar"] - ref["joint_q_bar"]).max() > 1e-3


def test_masks_and_exact_zeros(legs):
    """Contact pattern 0 and failed robots: grf_bar - grf_bar_in and the torque part of joint_q_bar are exactly 0; the kinematics term
    is unmasked (their joint_q_bar still moves with feet_bar); equality with a limit passes through; a NaN torque passes and
    propagates; a missing optional input counts as zero; both mask sources resolve alike."""
    c = legs
    b, grf, status, cot, ref = c["b"], c["grf"], c["status"], c["cot"], c["ref"]
    dead = ~ref["emit"]
    assert dead[0].all() and dead[16].all() and dead[5].all() and status[5] != 0 and b["stance"][5].any()
    assert np.array_equal(ref["grf_bar"][dead], cot["grf_bar_in"].reshape(40, 4, 3)[dead]) and not ref["torque_part"][dead].any()
    only_fk = KN.kin_cotangents(b, grf, status, KN.TAU_MIN, KN.TAU_MAX, feet_bar=cot["feet_bar"])
    assert np.abs(only_fk["joint_q_bar"][dead]).min() > 0 and not only_fk["grf_bar"].any()
    one = {k: v[15:16] for k, v in b.items()}
    raw = KN.kin_cotangents(one, grf[15:16], None, -1e9, 1e9, joint_tau_bar=np.ones((1, 12)))["tau_raw"]
    t = float(raw[0, 0, 1])
    for lo, hi, expect in ((t, 1e9, True), (-1e9, t, True), (np.nextafter(t, np.inf), 1e9, False), (-1e9, np.nextafter(t, -np.inf), False)):
        assert bool(KN.kin_cotangents(one, grf[15:16], None, lo, hi, joint_tau_bar=np.ones((1, 12)))["mask"][0, 0, 1]) is expect
    bad = dict(one, joint_q=one["joint_q"].copy())
    bad["joint_q"][0, 0] = np.nan
    r = KN.kin_cotangents(bad, grf[15:16], None, KN.TAU_MIN, KN.TAU_MAX, joint_tau_bar=np.ones((1, 12)))
    assert r["mask"][0, 0].all() and np.isnan(r["grf_bar"][0, 0]).any() and np.isfinite(r["grf_bar"][0, 1:]).all()
    bp, grfp, statusp, cotp = KN.case(40, "phase")
    refp = KN.kin_cotangents(bp, grfp, statusp, KN.TAU_MIN, KN.TAU_MAX, **cotp)
    assert np.array_equal(refp["emit"], ref["emit"]) and np.array_equal(refp["joint_q_bar"], ref["joint_q_bar"])


def test_clamped_share_of_the_committed_limits():
    """TAU_MIN / TAU_MAX clamp between 10 % and 90 % of the stance torque components of every batch size the GPU test uses from 16
    robots on (smaller ones do not hold every contact pattern), both ends among them."""
    for n in (16, 17, 40):
        b, grf, status, cot = KN.case(n, "stance")
        r = KN.kin_cotangents(b, grf, status, KN.TAU_MIN, KN.TAU_MAX, **cot)
        share = 1.0 - r["mask"][r["emit"]].mean()
        print(n, "clamped share", share)
        assert 0.1 <= share <= 0.9 and (r["tau_raw"][r["emit"]] < KN.TAU_MIN).any() and (r["tau_raw"][r["emit"]] > KN.TAU_MAX).any()


# ------------------------------------------------------------------ the oracle under the GPU test's keep rule
def test_oracle_meets_the_keep_rule_at_the_committed_step(built):
    """The end-to-end GPU test differentiates control_batch(want_torques=True) along joint_q + k h dq, x + k h dx at k = +-1, +-2 and
    keeps a robot that is solved with its working set and its clamp mask unchanged at all five points.  Here the oracle alone -
    the C oracle's tick (forward kinematics, solve, clamped torques), the certificate's working set of its forces, the restatement's
    clamp mask - meets that rule at h = FD_H on fd_case: kept 0.971 (>= 0.75 asked) with all 15 contact patterns among the kept.
    The sweep (committed seed; t = |FD(h) - FD(2h)| of the loss <c_tau, joint_tau> + <c_g, grf_body> on the oracle's tick, relative
    to |FD(h)|, over the kept robots):
      h      kept   face alone  worst t    median t
      1e-3   0.815  0.885       1.2e-03    2.7e-06
      1e-4   0.971  0.985       2.8e-05    2.8e-08
      1e-5   0.998  0.998       2.3e-06    3.0e-10
      1e-6   1.000  1.000       6.1e-06    2.7e-11      (the worst robot is rounding: force error / h)
    The truncation falls as h^2 down to 1e-5 and is rounding from there on, as for the feet and the rotations, whose h = FD_H = 1e-4
    the GPU test uses too: the device's forces carry ~1e-8 N, ten times the oracle's, which moves the turning point up by as much."""
    from oracle import c_oracle
    from tests import kkt_certificate_restatement as KR

    P = q.cheetah_params(mu=0.6)
    b, d = KN.fd_case(N_FD)
    kin = c_oracle.default_kinematics()
    kin.tau_min, kin.tau_max = KN.FD_TAU_MIN, KN.FD_TAU_MAX

    def at(k, h):
        bb = dict(b, joint_q=np.ascontiguousarray(b["joint_q"] + k * h * d["dq"]), x=np.ascontiguousarray(b["x"] + k * h * d["dx"]))
        t = c_oracle.tick_batch(P, bb, kin=kin)
        F, st = t["grf_body"], t["status"]
        cert = KR.certificate(P, dict(bb, feet=t["feet"]), F)
        r = KN.kin_cotangents(bb, F, st, KN.FD_TAU_MIN, KN.FD_TAU_MAX, joint_tau_bar=np.ones_like(F))
        clamped = np.where(r["emit"][..., None], np.clip(r["tau_raw"], KN.FD_TAU_MIN, KN.FD_TAU_MAX), 0.0).reshape(-1, 12)
        assert np.abs(clamped - t["joint_tau"]).max() < 1e-12  # the oracle's tick and the restatement clamp the same torques
        return st, cert["active"], r["mask"]

    st0, a0, m0 = at(0, FD_H)
    keep = st0 == 0
    for k in (-2, -1, 1, 2):
        st, a, m = at(k, FD_H)
        keep &= (st == 0) & (a == a0).all(axis=1) & (m == m0).all(axis=(1, 2))
    print("kept", keep.mean())
    assert keep.mean() >= 0.75, keep.mean()
    pats = set((b["stance"][keep].astype(int) * [1, 2, 4, 8]).sum(axis=1).tolist())
    assert pats == set(range(1, 16)), sorted(pats)
    emit = (b["stance"] != 0) & (st0 == 0)[:, None]
    assert (~m0[emit]).mean() > 0.05 and m0[emit].mean() > 0.05  # the limits do clamp, and do pass


# ------------------------------------------------------------------ the C ABI without a device
IO_POINTERS = ("grf_body", "status", "joint_tau_bar", "feet_bar", "grf_bar_in", "joint_q_bar_in", "grf_bar", "joint_q_bar")


def test_symbols_are_exported_and_the_abi_stays(built):
    from quadruped_control_amd import _lib

    lib = ctypes.CDLL(os.path.join(ROOT, "quadruped_control_amd", "libqc_balance.so"))
    for name in ("qc_default_sensitivity_kin", "qc_sensitivity_kin_batch"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert _lib.load().qc_abi_version() == 6 and _lib.ABI_VERSION == 6  # new entry points, no change to what existed
    assert ctypes.sizeof(_lib.QcSensitivityIo) == 112 and ctypes.sizeof(_lib.QcSensitivityRotIo) == 72


def test_mirror_matches_the_header(built, tmp_path):
    """sizeof and the member offsets of qc_sensitivity_kin_io as the C compiler lays the header's struct out, against the ctypes
    mirror; qc_default_sensitivity_kin fills the io as documented and needs no device."""
    from quadruped_control_amd import _lib

    fields = [f for f, _ in _lib.QcSensitivityKinIo._fields_]
    assert fields == ["struct_size"] + list(IO_POINTERS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qc_balance.h"\nint main(void) {\n  printf("%zu", sizeof(qc_sensitivity_kin_io));\n'
                   + "".join(f'  printf(" %zu", offsetof(qc_sensitivity_kin_io, {f}));\n' for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_lib.QcSensitivityKinIo) == 72
    assert got[1:] == [getattr(_lib.QcSensitivityKinIo, f).offset for f in fields]
    io = _lib.QcSensitivityKinIo()
    io.grf_body, io.joint_q_bar, io.struct_size = 123, 456, 7
    _lib.load().qc_default_sensitivity_kin(ctypes.byref(io))
    assert io.struct_size == 72
    assert all(getattr(io, f) is None for f in IO_POINTERS)


def test_argument_check_needs_no_device(built):
    """qc_sensitivity_kin_batch refuses a bad call before it touches the device - the handle is null, so every call below ends in the
    argument check."""
    from quadruped_control_amd import _lib

    lib = _lib.load()
    io = _lib.QcSensitivityKinIo()
    lib.qc_default_sensitivity_kin(ctypes.byref(io))
    bi = _lib.QcBatchIn()
    for args in ((None, 1, ctypes.byref(bi), ctypes.byref(io), None), (None, 0, ctypes.byref(bi), None, None), (None, 1, None, ctypes.byref(io), None)):
        assert lib.qc_sensitivity_kin_batch(*args) == -1 and _lib.last_error() == "qc_sensitivity_kin_batch: null argument"


def test_host_logic_without_a_device():
    """check_sensitivity_kin_args through every refusal - a null handle, `in` or `io`, a wrong struct_size, no output, no cotangent,
    joint_tau_bar without grf_body or status, grf_bar without joint_tau_bar, a missing joint_q, n beyond one launch - and the accepted
    combinations, a batch without any state array among them, with its message (csrc/qc_host.hpp), in a stand-alone program built
    with the address and undefined-behaviour sanitizers (tests/cpp/sensitivity_kin_host_test.cpp)."""
    import __graft_entry__ as g

    assert "sensitivity_kin_host_test" in g.HOST_TESTS
    exe = g.build_host_test("sensitivity_kin_host_test")
    assert exe is not None and os.path.exists(exe)
    libs = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "amdhip64" not in libs and "qc_balance" not in libs, libs
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "sensitivity kinematics host logic ok" in r.stdout, r.stdout[-3000:]
