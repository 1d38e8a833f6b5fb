"""CPU: the forward mode's numpy restatement (tests/tangent_restatement.py) against the adjoint restatements through the dot-product
identity, and the C ABI of qc_tangent_batch as far as it goes without a device."""
import ctypes
import os
import subprocess

import numpy as np

import quadruped_control_amd as q
from tests import sensitivity_restatement as SR
from tests import sensitivity_rotation_restatement as RR
from tests import tangent_restatement as TR
from tests.solved_batch_support import EPS, inputs
from tests.tangent_restatement import C_DOT, C_TAN, dot_gap

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_restatement_against_50_digits():
    """The float64 restatement against tangent_mp on every eighth robot of the 130-robot placed-force batch, two directions each: from
    `feet` with every tangent but joint_q_tan, and from joint_q with every tangent.  The distance of every entry of grf_tan and b_tan
    is measured in EPS x its condition sum (tests/tangent_restatement.py); an entry whose condition sum is 0 is exact.  The worst is
    the module's C_TAN (measured: grf_tan 0.52 / 0.66, b_tan 1.06); the device's bar is 4 x it.  This is the worst of a SAMPLE -
    robots 0, 8, ... 128: over all 130 robots b_tan reaches 3.06, the module's C_TAN_ALL, which
    tests/test_odd_law_cpu.py::test_tangent_restatement_against_50_digits_on_every_robot asserts."""
    from tests.kkt_certificate_restatement import distance

    P = q.cheetah_params(mu=0.6)
    worst = {}
    for source in ("feet", "joint_q"):
        b, grf = inputs(130, source)
        tans = TR.random_tangents(130, 2, 50, joint_q=source != "feet")
        t = TR.tangent(P, b, grf, tans)
        assert (t["flags"] == 0).all()
        for i in range(0, 130, 8):
            for k in range(2):
                ref = TR.tangent_mp(P, b, grf, tans, i, k, t["active"][i])
                for name, sums in (("grf_tan", "grf_sum"), ("b_tan", "b_sum")):
                    d, c = distance(t[name][k, i], ref[name]), t[sums][k, i].reshape(-1)
                    assert np.all(d[c == 0] == 0), (source, i, k, name)
                    if (c > 0).any():
                        worst[source, name] = max(worst.get((source, name), 0.0), float((d[c > 0] / (EPS * c[c > 0])).max()))
    print("C_TAN measured", worst)
    assert np.abs(t["grf_tan"]).max() > 0 and max(worst.values()) <= C_TAN, worst
def test_dot_product_identity_in_numpy():
    """<v, tangent(u)> = sum <theta_bar, theta_tan> over the outputs of sensitivity_restatement (x_bar ... w_d_bar, feet_bar) and of
    sensitivity_rotation_restatement (Rwb_rot_bar, Rwb_d_rot_bar), on the 130-robot placed-force batch, for two random directions u in
    every input at once and a random cotangent v.  The two sides share no formula beyond the face and the reduced matrix: the forward
    side differentiates the wrench law and the log in forward mode, the reverse side pulls back through them.  The gap is measured in
    EPS x (sum of the magnitudes of all terms on both sides) x the reduced condition number; the measured worst is C_DOT."""
    P = q.cheetah_params(mu=0.6)
    n, K = 130, 2
    b, grf = inputs(n, "feet")
    tans = TR.random_tangents(n, K, 1)
    gbar = np.random.default_rng(2).normal(0.0, 1.0, (n, 12))
    t = TR.tangent(P, b, grf, tans)
    s = SR.sensitivity(P, b, grf, gbar)
    r = RR.rotation_cotangents(P, b, grf, gbar, s["b_bar"], s["feet_bar"])
    assert np.array_equal(t["flags"], s["flags"])
    ok = t["flags"] == 0
    assert ok.mean() > 0.9
    worst = 0.0
    for k in range(K):
        gap, lhs = dot_gap(gbar, t["grf_tan"], s, r, tans, k, t["cond"])
        assert (np.abs(lhs[ok]) > 0).mean() > 0.9  # (not vacuous: almost every robot has a face that moves)
        worst = max(worst, float(gap[ok].max()))
    print("C_DOT measured", worst)
    assert worst <= C_DOT, worst


def test_each_input_alone_in_numpy():
    """The identity for one input at a time: a sign or a factor wrong in one input's line cannot hide behind the others."""
    P = q.cheetah_params(mu=0.6)
    n = 130
    b, grf = inputs(n, "feet")
    gbar = np.random.default_rng(3).normal(0.0, 1.0, (n, 12))
    s = SR.sensitivity(P, b, grf, gbar)
    r = RR.rotation_cotangents(P, b, grf, gbar, s["b_bar"], s["feet_bar"])
    worst = {}
    for name in TR.TANGENTS:
        if name == "joint_q_tan":
            continue
        tans = TR.random_tangents(n, 1, 4, names=(name,))
        t = TR.tangent(P, b, grf, tans)
        ok = t["flags"] == 0
        gap, lhs = dot_gap(gbar, t["grf_tan"], s, r, tans, 0, t["cond"])
        print(name, float(gap[ok].max()))
        # (one robot in sixteen has no stance foot, and a face whose only free coordinates are orthogonal to one input's gradient
        # tangent does not move: three quarters is what "not vacuous" asks of a single input)
        assert (np.abs(lhs[ok]) > 0).mean() > 0.75, name
        worst[name] = float(gap[ok].max())
    print("worst gap per input", worst)
    assert max(worst.values()) <= C_DOT, worst


def test_joint_q_tangent_is_the_feet_tangent_through_the_leg_jacobian():
    """joint_q_tan = dq on a batch with joint_q gives what feet_tan = J(q) dq gives on the same batch with its feet written out."""
    from tests import kkt_certificate_restatement as KR
    from tests.leg_plant_restatement import jacobian

    P = q.cheetah_params(mu=0.6)
    n = 33
    b, grf = inputs(n, "joint_q")
    dq = TR.random_tangents(n, 1, 5, joint_q=True, names=("joint_q_tan",))
    qa = b["joint_q"].reshape(n, 4, 3)
    feet_tan = np.array([[jacobian(l, qa[i, l]) @ dq["joint_q_tan"][0, i].reshape(4, 3)[l] for l in range(4)] for i in range(n)]).reshape(1, n, 12)
    a = TR.tangent(P, b, grf, dq)
    c = TR.tangent(P, KR.with_feet(b), grf, {"feet_tan": feet_tan})
    assert np.abs(a["grf_tan"]).max() > 0
    assert np.allclose(a["grf_tan"], c["grf_tan"], rtol=0, atol=64 * EPS * np.abs(c["grf_tan"]).max())


def test_flagged_and_empty_faces():
    """All swing: grf_tan 0 exactly, flags 0, b_tan = db all the same.  All-zero forces under four stance feet (a failed robot):
    grf_tan 0, bit 0."""
    from quadruped_control_amd import workloads

    P = q.cheetah_params(mu=0.6)
    b = workloads.slice_batch(workloads.config3(n=8), 0, 3)
    tans = TR.random_tangents(3, 2, 6)
    b["stance"] = np.zeros((3, 4), np.uint8)
    t = TR.tangent(P, b, np.zeros((3, 12)), tans)
    assert not t["flags"].any() and not t["grf_tan"].any() and np.abs(t["b_tan"]).min() > 0
    b["stance"] = np.ones((3, 4), np.uint8)
    t = TR.tangent(P, b, np.zeros((3, 12)), tans)
    assert (t["flags"] == 1).all() and not t["grf_tan"].any()


# ------------------------------------------------------------------ the C ABI without a device
def test_tangent_exists(built):
    """The two symbols are in the built library, the header parses on its own and declares them, the package exposes the module -
    and none of it went into the pinned surfaces: _lib.EXPORTS, the ABI revision."""
    from quadruped_control_amd import _lib

    lib = ctypes.CDLL(os.path.join(ROOT, "quadruped_control_amd", "libqc_balance.so"))
    for name in ("qc_default_tangent", "qc_tangent_batch"):
        assert hasattr(lib, name) and name not in _lib.EXPORTS, name
    assert _lib.load().qc_abi_version() == 6
    assert callable(q.tangent.tangent_batch) and callable(q.tangent.jacobian_batch) and q.tangent.tangent_batch.__doc__ and q.tangent.jacobian_batch.__doc__
    header = open(os.path.join(ROOT, "include", "qc_tangent.h")).read()
    assert '#include "qc_balance.h"' in header and "qc_default_tangent(" in header and "qc_tangent_batch(" in header


def test_tangent_mirror_matches_the_header(built, tmp_path):
    """sizeof and the member offsets of qc_tangent_io as the C compiler lays the header's struct out, against the ctypes mirror;
    qc_default_tangent fills the io as documented and needs no device."""
    T = q.tangent
    T._library()
    fields = [f for f, _ in T.QcTangentIo._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qc_tangent.h"\nint main(void) {\n  printf("%zu", sizeof(qc_tangent_io));\n'
                   + "".join(f'  printf(" %zu", offsetof(qc_tangent_io, {f}));\n' for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(T.QcTangentIo) == 136
    assert got[1:] == [getattr(T.QcTangentIo, f).offset for f in fields]
    io = T.QcTangentIo()
    io.grf_body, io.grf_tan, io.act_tol, io.struct_size, io.n_dir = 123, 456, -1.0, 7, 9
    T._library().qc_default_tangent(ctypes.byref(io))
    assert io.struct_size == 136 and io.act_tol == 1e-7 and io.n_dir == 1
    assert all(getattr(io, f) is None for f in fields if f not in ("struct_size", "act_tol", "n_dir"))


def test_tangent_argument_check_needs_no_device(built):
    """qc_tangent_batch refuses a bad call before it touches the device: the message is its own."""
    from quadruped_control_amd import _lib

    T = q.tangent
    lib = T._library()
    io = T.QcTangentIo()
    lib.qc_default_tangent(ctypes.byref(io))
    bi = _lib.QcBatchIn()
    assert lib.qc_tangent_batch(None, 1, ctypes.byref(bi), ctypes.byref(io), None) == -1
    assert _lib.last_error() == "qc_tangent_batch: null argument"
    assert lib.qc_tangent_batch(None, 0, ctypes.byref(bi), None, None) == -1 and _lib.last_error() == "qc_tangent_batch: null argument"


def test_tangent_host_logic_without_a_device():
    """check_tangent_args through every refusal and their order, tangent_constants, the launch grid past its cap and the [K][n]
    offsets (csrc/qc_host.hpp, csrc/qc_tangent.hpp), in a stand-alone program built with the address and undefined-behaviour
    sanitizers (tests/cpp/tangent_host_test.cpp)."""
    import __graft_entry__ as g

    assert "tangent_host_test" in g.HOST_TESTS
    exe = g.build_host_test("tangent_host_test")
    assert exe is not None and os.path.exists(exe)
    libs = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "amdhip64" not in libs and "qc_balance" not in libs, libs
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "tangent host logic ok" in r.stdout, r.stdout[-3000:]


# ------------------------------------------------------------------ central differences of the forces
def test_central_differences_of_the_forces(built):
    """<grf_bar, grf_tan> of the float64 restatement against central differences of the C oracle's forces on fd_support's 480-robot
    batch (every non-empty contact pattern 32 times), with its keep rule (_kept: solved, flags 0, the certificate's working set of
    the oracle's forces unchanged at every point) and _check_kept (kept share >= 0.75, all 15 patterns among the kept).  Two
    directions, each with the step and the bar of the existing test of the adjoint on the same batch (tests/test_sensitivity_cpu.py):
    the b-type inputs at h = 1e-3, bar 1e-8 |theta_bar| |d| (exactly linear on a fixed face); the feet at h = 1e-4, bar
    |FD(h) - FD(2h)| + 1e-7 |feet_bar| |d|.  The scales are those tests': the norms of sensitivity_restatement's cotangents."""
    from oracle import c_oracle
    from tests import kkt_certificate_restatement as KR
    from tests.fd_support import N_FD, _check_kept, _kept, fd_batch

    P = q.cheetah_params(mu=0.6)
    b, n = fd_batch(), N_FD
    gbar = np.random.default_rng(5).normal(0.0, 1.0, (n, 12))
    F0, st0, _ = c_oracle.control_batch(P, b)
    s = SR.sensitivity(P, b, F0, gbar)
    c = dict(b=b, st0=st0, s=s)

    def at(d, h):
        bb = dict(b)
        for k, v in d.items():
            bb[k] = b[k] + h * v
        F, st, _ = c_oracle.control_batch(P, bb)
        return F, st, KR.certificate(P, bb, F)["active"]

    keys = ("x", "xdot", "w", "x_d", "xdot_d", "w_d")
    rng = np.random.default_rng(61)
    d = {k: rng.normal(0.0, 1.0, (n, 3)) for k in keys}
    t = TR.tangent(P, b, F0, {k + "_tan": v[None] for k, v in d.items()})
    assert np.array_equal(t["flags"], s["flags"])
    h = 1e-3
    Fp, Fm = at(d, h), at(d, -h)
    keep = _kept(c, (Fp, Fm))
    _check_kept(c, keep)
    fd = (gbar * (Fp[0] - Fm[0])).sum(axis=1) / (2 * h)
    an = (gbar * t["grf_tan"][0].reshape(n, 12)).sum(axis=1)
    scale = np.sqrt(sum((s[k + "_bar"] ** 2).sum(axis=1) for k in keys)) * np.sqrt(sum((d[k] ** 2).sum(axis=1) for k in keys))
    err = np.abs(fd - an)
    print("b-type: kept", keep.mean(), "worst relative error", float((err[keep] / np.maximum(scale[keep], 1e-300)).max()))
    assert (scale[keep] > 0).mean() > 0.9 and np.all(err[keep] <= 1e-8 * scale[keep])

    df = np.random.default_rng(62).normal(0.0, 1.0, (n, 12))
    t = TR.tangent(P, b, F0, {"feet_tan": df[None]})
    h = 1e-4
    pts = {k: at({"feet": df}, k * h) for k in (-2, -1, 1, 2)}
    keep = _kept(c, pts.values())
    _check_kept(c, keep)
    fd1 = (gbar * (pts[1][0] - pts[-1][0])).sum(axis=1) / (2 * h)
    fd2 = (gbar * (pts[2][0] - pts[-2][0])).sum(axis=1) / (4 * h)
    an = (gbar * t["grf_tan"][0].reshape(n, 12)).sum(axis=1)
    scale = np.linalg.norm(s["feet_bar"].reshape(n, 12), axis=1) * np.linalg.norm(df, axis=1)
    err, tr = np.abs(fd1 - an), np.abs(fd1 - fd2)
    print("feet: kept", keep.mean(), "worst error beyond t", float((np.maximum(err - tr, 0.0)[keep] / np.maximum(scale[keep], 1e-300)).max()))
    assert (scale[keep] > 0).mean() > 0.9 and np.all(err[keep] <= tr[keep] + 1e-7 * scale[keep])
