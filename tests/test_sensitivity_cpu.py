"""CPU: the adjoint's numpy restatement (tests/sensitivity_restatement.py) against central differences of the C oracle and
against its own 50-digit variant, and the C ABI of qc_sensitivity_batch as far as it goes without a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import quadruped_control_amd as q
from quadruped_control_amd import workloads
from tests import device_math_reference as DMR
from tests import kkt_certificate_restatement as KR
from tests import sensitivity_restatement as SR
from tests.fd_support import N_FD, _check_kept, _kept, fd_batch, pinned_cases

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EPS = 2.0 ** -52
B_KEYS = ("x", "xdot", "w", "x_d", "xdot_d", "w_d")


@pytest.fixture(scope="module")
def solved(built):
    from oracle import c_oracle

    P = q.cheetah_params(mu=0.6)
    b = fd_batch()
    rng = np.random.default_rng(5)
    gbar = rng.normal(0.0, 1.0, (N_FD, 12))
    F0, st0, _ = c_oracle.control_batch(P, b)
    s = SR.sensitivity(P, b, F0, gbar)
    return dict(P=P, b=b, rng=rng, gbar=gbar, F0=F0, st0=st0, s=s)


def _oracle_at(P, b, d, h):
    from oracle import c_oracle

    bb = dict(b)
    for k, v in d.items():
        bb[k] = b[k] + h * v
    F, st, _ = c_oracle.control_batch(P, bb)
    return F, st, KR.certificate(P, bb, F)["active"]


def test_b_type_cotangents_against_oracle_differences(solved):
    """<theta_bar, d> against <grf_bar, (F(theta + h d) - F(theta - h d)) / 2h> of the C oracle for a random direction d in
    (x, xdot, w, x_d, xdot_d, w_d), 480 robots, every non-empty contact pattern 32 times.  On a fixed face f is exactly linear in
    b and b is linear in these inputs at fixed Rwb, Rwb_d: no truncation, so h = 1e-3 (metres, m/s, rad/s).  Kept share of the
    committed seed: 0.91 (the working set must be the same at -h, 0, +h; all 15 patterns are among the kept).
    Bar: the difference quotient carries the oracle's own force error dF / h.  The oracle recomputes each accepted point in long
    double, dF <~ 1e-12 x 120 N ~ 1e-10 N, so dF / h ~ 1e-7 on derivatives of size |theta_bar| |d| ~ 5e3: ~2e-11 relative.  The
    restatement's own error against its 50-digit variant is 1e-11 relative (test_restatement_against_50_digits).  The bar is
    1e-8 |theta_bar| |d|: a factor 500 over either."""
    c = solved
    P, b, n = c["P"], c["b"], N_FD
    rng = np.random.default_rng(6)
    d = {k: rng.normal(0.0, 1.0, (n, 3)) for k in B_KEYS}
    h = 1e-3
    Fp, Fm = _oracle_at(P, b, d, h), _oracle_at(P, b, d, -h)
    keep = _kept(c, (Fp, Fm))
    print("kept", keep.mean())
    _check_kept(c, keep)
    fd = (c["gbar"] * (Fp[0] - Fm[0])).sum(axis=1) / (2 * h)
    an = sum((c["s"][k + "_bar"] * d[k]).sum(axis=1) for k in B_KEYS)
    scale = np.sqrt(sum((c["s"][k + "_bar"] ** 2).sum(axis=1) for k in B_KEYS)) * np.sqrt(sum((d[k] ** 2).sum(axis=1) for k in B_KEYS))
    err = np.abs(fd - an)
    print("worst relative error", float((err[keep] / np.maximum(scale[keep], 1e-300)).max()))
    assert (scale[keep] > 0).mean() > 0.9  # (the check is not vacuous: almost every kept robot has a face that moves)
    assert np.all(err[keep] <= 1e-8 * scale[keep]), float((err[keep] / np.maximum(scale[keep], 1e-300)).max())


def test_feet_cotangent_against_oracle_differences(solved):
    """The same for a random direction in `feet` (body-frame foot positions).  A enters the Hessian, so the difference quotient has
    O(h^2) truncation.  A sweep on the oracle (h = 1e-3 ... 1e-7) shows the quotient's error falling as h^2 down to h = 1e-4 and
    rounding (oracle force error / h, worst on robots whose reduced Hessian is carried by W alone) taking over below 1e-5: h = 1e-4.
    The truncation is estimated per robot from the oracle alone: t = |FD(h) - FD(2h)| is three times the h^2 term of FD(h).  Bar:
    t + 1e-7 |feet_bar| |d| - the rounding term of the b-type test scaled by its 1 / h.  Kept share of the committed seed: 0.96
    (the working set must be the same at 0, +-h and +-2h)."""
    c = solved
    P, b, n = c["P"], c["b"], N_FD
    rng = np.random.default_rng(7)
    d = {"feet": rng.normal(0.0, 1.0, (n, 12))}
    h = 1e-4
    pts = {k: _oracle_at(P, b, d, k * h) for k in (-2, -1, 1, 2)}
    keep = _kept(c, pts.values())
    print("kept", keep.mean())
    _check_kept(c, keep)
    fd1 = (c["gbar"] * (pts[1][0] - pts[-1][0])).sum(axis=1) / (2 * h)
    fd2 = (c["gbar"] * (pts[2][0] - pts[-2][0])).sum(axis=1) / (4 * h)
    fbar = c["s"]["feet_bar"].reshape(n, 12)
    an = (fbar * d["feet"]).sum(axis=1)
    scale = np.linalg.norm(fbar, axis=1) * np.linalg.norm(d["feet"], axis=1)
    err, t = np.abs(fd1 - an), np.abs(fd1 - fd2)
    print("worst relative error", float((err[keep] / np.maximum(scale[keep], 1e-300)).max()), "worst t", float((t[keep] / np.maximum(scale[keep], 1e-300)).max()))
    assert (scale[keep] > 0).mean() > 0.9
    assert np.median(t[keep] / np.maximum(scale[keep], 1e-300)) < 1e-6  # (the bar is tight: the estimate itself is small)
    assert np.all(err[keep] <= t[keep] + 1e-7 * scale[keep])


# ------------------------------------------------------------------ 50 digits


def test_restatement_against_50_digits():
    """The float64 restatement against sensitivity_mp on the hand-picked robots: a tied axis, fz pinned at fzmax with a pinned fy, an
    interior foot, a swing leg or fz = fzmin; uniform weights, and a general SPD S with a dense W.  Bar per robot and output:
    16 eps cond(Z^T H Z) max|output| - a Cholesky solve is backward stable, its forward error is c n eps cond with n = 12 and c
    of order one.  The last case takes its feet from joint_q (the `kin` branch of sensitivity_mp)."""
    rng = np.random.default_rng(3)
    for name, P, b, grf, codes in pinned_cases():
        gbar = rng.normal(0.0, 1.0, (1, 12))
        s = SR.sensitivity(P, b, grf, gbar, act_tol=1e-9)
        assert s["active"][0].tolist() == codes, (name, s["active"][0])
        assert s["flags"][0] == 0
        ref = SR.sensitivity_mp(P, b, grf, gbar, 0, s["active"][0], kin=(DMR.HIP.reshape(-1), DMR.LINKS.reshape(-1)) if "joint_q" in b else None)
        cond = SR.reduced_condition(P, b, s["active"], 0)
        assert np.abs(s["adjoint"][0]).max() > 0
        assert s["adjoint"][0][[5, 9, 10, 11] if codes[3] == KR.SWING else [5, 11]].tolist() == [0.0] * (4 if codes[3] == KR.SWING else 2)  # pinned
        assert s["adjoint"][0][0] == P["mu"] * s["adjoint"][0][2] and s["adjoint"][0][4] == 0.0  # tied / pinned with its fz
        for k in SR.OUTPUTS + ("r_bar",):
            dist = SR.distance(s[k][0], ref[k])
            bar = 16 * EPS * cond * SR.magnitude(ref[k])
            print(name, k, "error / bar", float(dist.max() / bar), "cond", cond)
            assert np.all(dist <= bar), (name, k, dist.max(), bar)


def test_flagged_and_empty_faces():
    """All swing: every output 0, flags 0.  All-zero forces (a failed robot): every stance foot on both friction rows - adjoint 0,
    bit 0.  fzmin = fzmax: both fz rows - bit 0."""
    P = q.cheetah_params(mu=0.6)
    b = workloads.slice_batch(workloads.config3(n=8), 0, 3)
    gbar = np.ones((3, 12))
    b["stance"] = np.zeros((3, 4), np.uint8)
    s = SR.sensitivity(P, b, np.zeros((3, 12)), gbar)
    assert not s["flags"].any() and all(not s[k].any() for k in SR.OUTPUTS)
    b["stance"] = np.ones((3, 4), np.uint8)
    s = SR.sensitivity(P, b, np.zeros((3, 12)), gbar)
    assert (s["flags"] == 1).all() and not s["adjoint"].any()
    P2 = dict(P, fzmin=35.0, fzmax=35.0)
    grf = -np.einsum("nji,nkj->nki", b["Rwb"].reshape(3, 3, 3), np.tile([1.0, -2.0, 35.0], (3, 4, 1))).reshape(3, 12)
    s = SR.sensitivity(P2, b, grf, gbar)
    assert (s["flags"] == 1).all() and not s["adjoint"].any()


# ------------------------------------------------------------------ the C ABI without a device
IO_POINTERS = ("grf_body", "grf_bar", "adjoint", "b_bar", "feet_bar", "x_bar", "xdot_bar", "w_bar", "x_d_bar", "xdot_d_bar", "w_d_bar", "flags")


def test_sensitivity_symbols_are_exported(built):
    from quadruped_control_amd import _lib

    lib = ctypes.CDLL(os.path.join(ROOT, "quadruped_control_amd", "libqc_balance.so"))
    for name in ("qc_default_sensitivity", "qc_sensitivity_batch"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert _lib.load().qc_abi_version() == 6  # new entry points, no change to what existed


def test_sensitivity_mirror_matches_the_header(built, tmp_path):
    """sizeof and the member offsets of qc_sensitivity_io as the C compiler lays the header's struct out, against the ctypes
    mirror; qc_default_sensitivity fills the io as documented and needs no device."""
    from quadruped_control_amd import _lib

    fields = [f for f, _ in _lib.QcSensitivityIo._fields_]
    assert fields == ["struct_size", "grf_body", "grf_bar", "act_tol"] + list(IO_POINTERS[2:])
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qc_balance.h"\nint main(void) {\n  printf("%zu", sizeof(qc_sensitivity_io));\n'
                   + "".join(f'  printf(" %zu", offsetof(qc_sensitivity_io, {f}));\n' for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_lib.QcSensitivityIo) == 112
    assert got[1:] == [getattr(_lib.QcSensitivityIo, f).offset for f in fields]
    io = _lib.QcSensitivityIo()
    io.grf_body, io.adjoint, io.act_tol, io.struct_size = 123, 456, -1.0, 7
    _lib.load().qc_default_sensitivity(ctypes.byref(io))
    assert io.struct_size == 112 and io.act_tol == 1e-7
    assert all(getattr(io, f) is None for f in IO_POINTERS)


def test_sensitivity_argument_check_needs_no_device(built):
    """qc_sensitivity_batch refuses a bad call before it touches the device: the message is its own."""
    from quadruped_control_amd import _lib

    lib = _lib.load()
    io = _lib.QcSensitivityIo()
    lib.qc_default_sensitivity(ctypes.byref(io))
    bi = _lib.QcBatchIn()
    assert lib.qc_sensitivity_batch(None, 1, ctypes.byref(bi), ctypes.byref(io), None) == -1
    assert _lib.last_error() == "qc_sensitivity_batch: null argument"
    assert lib.qc_sensitivity_batch(None, 0, ctypes.byref(bi), None, None) == -1 and _lib.last_error() == "qc_sensitivity_batch: null argument"


def test_sensitivity_host_logic_without_a_device():
    """check_sensitivity_args through every refusal, and the launch grid (csrc/qc_host.hpp), in a stand-alone program built with
    the address and undefined-behaviour sanitizers (tests/cpp/sensitivity_host_test.cpp)."""
    import __graft_entry__ as g

    assert "sensitivity_host_test" in g.HOST_TESTS
    exe = g.build_host_test("sensitivity_host_test")
    assert exe is not None and os.path.exists(exe)
    libs = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "amdhip64" not in libs and "qc_balance" not in libs, libs
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "sensitivity host logic ok" in r.stdout, r.stdout[-3000:]
