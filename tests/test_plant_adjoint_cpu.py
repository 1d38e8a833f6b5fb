"""CPU: the plant step's reverse pass restated in numpy (tests/plant_adjoint_restatement.py) against central differences of
plant_step_np and against its own 50-digit variant, the A1 / B1 crossover against 50 digits, and the C ABI of
qc_plant_step_adjoint_batch as far as it goes without a device.

c_np, the worst |numpy - 50 digits| / (EPS x condition sum) per output over the three pools (dt = 1e-4, 1/300, 1e-2; 257 robots each),
measured here and asserted not to exceed what tests/plant_adjoint_restatement.py records as C_NP (the measurement rounded up):
    measured   Rwb_bar 1.35   x_bar 1.52   xdot_bar 0.97   w_bar 0.99   grf_bar 2.00   foot_world_bar 2.17
    C_NP       Rwb_bar 1.4    x_bar 1.6    xdot_bar 1.0    w_bar 1.0    grf_bar 2.1    foot_world_bar 2.2
tests/test_gpu_plant_adjoint.py holds the device to K = 4 C_NP of the same scale."""
import ctypes
import os
import subprocess

import mpmath as mp
import numpy as np
import pytest

import quadruped_control_amd as q
from tests import plant_adjoint_restatement as AR
from tests import plant_restatement as PR
from tests.fd_support import BAR_OF, fd_bar

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EPS = AR.EPS
C_NP = AR.C_NP
FD_DT = 1.0 / 300.0


@pytest.fixture(scope="module")
def P(built):
    return q.cheetah_params()


def test_adjoint_against_central_differences_of_the_step(P):
    """<x_bar, v> of the numpy adjoint against central differences of plant_step_np's loss <c, y> along the committed directions v in
    all six inputs at once (entrywise for Rwb: the step is evaluated on nine numbers that are no rotation), on the first 65 robots of
    the pool (identity, nearly pi, w = 0, +-1e-12, ordinary; dt = 1/300).  The step is smooth: every robot is kept.  Bar: fd_bar.
    The sweep (worst over the robots, relative to |x_bar| |v|):
      h      worst error  worst t    median error
      1e-2   2.7e-04      8.2e-04    1.5e-05
      1e-3   2.7e-06      8.2e-06    1.5e-07
      1e-4   2.7e-08      8.2e-08    1.5e-09
      1e-5   2.7e-10      8.2e-10    1.5e-11
      1e-6   1.4e-11      1.5e-11    2.5e-12
      1e-7   1.3e-10      1.4e-10    2.3e-11
      1e-8   2.7e-09      3.2e-09    2.4e-10
    The error falls as h^2 down to 1e-5 and is rounding from 1e-6 on (it grows as 1 / h below): h = 1e-5, the last step at which the
    truncation estimate still is one."""
    dt, h, n = FD_DT, AR.FD_H, AR.FD_N
    s, bars = ({k: a[:n] for k, a in d.items()} for d in AR.pool(dt))
    v = AR.fd_directions()
    an = AR.plant_adjoint_np(P["mass"], P["Ib"], *(s[k] for k in AR.INPUTS), dt, bars)
    cond = {k: c[:n] for k, (_, c) in AR.pool_reference(dt).items()}
    step = lambda d: PR.plant_step_np(P["mass"], P["Ib"], *(d[k] for k in AR.INPUTS), dt)
    fd1, fd2 = AR.fd_of(step, s, bars, v, h)
    dd = sum((an[BAR_OF[k]] * v[k]).sum(axis=1) for k in AR.INPUTS)
    bar = fd_bar(P, s, bars, v, cond, fd1, fd2, h, dt)
    err = np.abs(fd1 - dd)
    scale = np.sqrt(sum((an[BAR_OF[k]] ** 2).sum(axis=1) for k in AR.INPUTS)) * np.sqrt(sum((v[k] ** 2).sum(axis=1) for k in AR.INPUTS))
    print("worst relative error", float((err / scale).max()), "worst bar", float((bar / scale).max()), "worst error / bar", float((err / bar).max()))
    assert (scale > 0).all() and np.median(bar / scale) < 1e-8  # (the bar is tight: nine digits of the derivative)
    assert np.all(err <= bar), float((err / bar).max())


def test_each_input_cotangent_is_seen(P):
    """A guard on the test above: along a direction in ONE input, the analytic derivative is far beyond that test's bar on most
    robots - so a missing or wrong output would show - and it agrees with the difference quotient input by input."""
    dt, h, n = FD_DT, AR.FD_H, AR.FD_N
    s, bars = ({k: a[:n] for k, a in d.items()} for d in AR.pool(dt))
    an = AR.plant_adjoint_np(P["mass"], P["Ib"], *(s[k] for k in AR.INPUTS), dt, bars)
    step = lambda d: PR.plant_step_np(P["mass"], P["Ib"], *(d[k] for k in AR.INPUTS), dt)
    for name in AR.INPUTS:
        v = {k: (a if k == name else np.zeros_like(a)) for k, a in AR.fd_directions().items()}
        fd1, fd2 = AR.fd_of(step, s, bars, v, h)
        dd = (an[BAR_OF[name]] * v[name]).sum(axis=1)
        assert np.mean(np.abs(dd) > 1e-4 * np.abs(an[BAR_OF[name]]).max(axis=1)) > 0.5, name
        assert np.all(np.abs(fd1 - dd) <= np.abs(fd1 - fd2) + 1e-9 * (1.0 + np.abs(dd))), name


def test_restatement_against_50_digits_on_the_pool(P):
    """The numpy adjoint against plant_adjoint_mp on the GPU test's pools, every output entry, in units of EPS x condition sum: c_np
    (module docstring).  The pools' step angles are asserted to cover 0 exactly, 1e-12 ... 3 and both sides of the series threshold."""
    worst = {k: 0.0 for k in AR.OUTPUTS}
    for dt in AR.DTS:
        s, bars = AR.pool(dt)
        theta = AR.step_angle(P, s, dt)
        assert (theta == 0).sum() >= 8 and ((theta > 0) & (theta < 3e-12)).any() and theta.max() >= 2.99
        assert ((theta > 0.98) & (theta * theta < AR.SERIES_BELOW)).sum() >= 2 and ((theta * theta >= AR.SERIES_BELOW) & (theta < 1.02)).sum() >= 2
        assert np.allclose(theta[-AR.SWEEP:], AR.SWEEP_THETA, rtol=1e-6, atol=0)
        ref = AR.pool_reference(dt)
        an = AR.plant_adjoint_np(P["mass"], P["Ib"], *(s[k] for k in AR.INPUTS), dt, bars)
        for k in AR.OUTPUTS:
            val, cond = ref[k]
            assert (cond > 0).all()
            worst[k] = max(worst[k], float((np.abs(an[k] - val) / (EPS * cond)).max()))
    print("c_np", worst)
    for k in AR.OUTPUTS:
        assert worst[k] <= C_NP[k], (k, worst[k])


def test_exp_slopes_crossover_against_50_digits():
    """A1 = (cos t - A) / t^2 and B1 = (A - 2 B) / t^2 over t = 1e-12 ... 3 (400 points, logarithmic, and the two doubles next to the
    threshold t^2 = 1 on either side) against 50 digits.  Bars: below the threshold the series' nine terms leave 20 / 21! = 4e-19 and
    20 / 22! = 2e-20 of sums of at least 0.30 and 0.078, and Horner's nine steps round 2 EPS each of partial sums no larger than the
    first coefficient: 8 EPS of 1/3 and of 1/12.  From the threshold on the minuends carry the roundings - sin and cos of t / 2 to an
    ulp, A = (s / h) c four, cos t = 1 - 2 s^2 three of at most 3, 2 B six - which the division by t^2 passes on:
    8 EPS (|cos t| + |A|) / t^2 and 8 EPS (|A| + 2 |B|) / t^2, plus 2 EPS of the quotient itself.  At t = 0 exactly: the limits."""
    t = np.concatenate([np.logspace(-12, np.log10(3.0), 400), [np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0)]])
    th2 = t * t
    A1, B1 = AR.exp_slopes_np(th2)
    assert (th2 < AR.SERIES_BELOW).sum() > 100 and (th2 >= AR.SERIES_BELOW).sum() > 10
    worst = [0.0, 0.0, 0.0, 0.0]
    with mp.workdps(AR.DPS):
        for i, z in enumerate(th2):
            zm = AR.mpf(z)
            a1, b1 = AR.exp_slopes_mp(zm)
            tm = mp.sqrt(zm)
            A, B, ct = mp.sin(tm) / tm, (1 - mp.cos(tm)) / zm, mp.cos(tm)
            if z < AR.SERIES_BELOW:
                bar_a, bar_b, side = 8 * EPS / 3, 8 * EPS / 12, 0
            else:
                bar_a = float(8 * EPS * (abs(ct) + abs(A)) / zm + 2 * EPS * abs(a1))
                bar_b = float(8 * EPS * (abs(A) + 2 * abs(B)) / zm + 2 * EPS * abs(b1))
                side = 2
            ea, eb = abs(float(A1[i] - a1)), abs(float(B1[i] - b1))
            worst[side], worst[side + 1] = max(worst[side], ea / bar_a), max(worst[side + 1], eb / bar_b)
            assert ea <= bar_a and eb <= bar_b, (t[i], ea / bar_a, eb / bar_b)
    print("worst error / bar: series A1 %.3f B1 %.3f, quotients A1 %.3f B1 %.3f" % tuple(worst))
    z0 = AR.exp_slopes_np(np.array([0.0, 1e-300]))
    assert z0[0][0] == -1.0 / 3.0 and z0[1][0] == -1.0 / 12.0 and z0[0][1] == -1.0 / 3.0 and z0[1][1] == -1.0 / 12.0
    assert all(np.isnan(v[0]) for v in AR.exp_slopes_np(np.array([np.nan])))


def test_zero_cotangents_and_the_smooth_limit_at_zero_angle(P):
    """All cotangents zero: every output exactly zero.  A robot whose step angle is 0 exactly (w = 0, no force): the forward step
    selects A = 1 there, the reverse pass differentiates the smooth limit - w_bar carries dt times the axial part of Rwb'_bar Rwb^T,
    not zero."""
    dt = FD_DT
    s, bars = AR.pool(dt)
    zero = AR.plant_adjoint_np(P["mass"], P["Ib"], *(s[k] for k in AR.INPUTS), dt, {k: np.zeros_like(v) for k, v in bars.items()})
    assert all(not zero[k].any() for k in AR.OUTPUTS)
    assert not s["w"][0].any() and not s["grf_body"][0].any() and AR.step_angle(P, s, dt)[0] == 0.0
    only_R = AR.plant_adjoint_np(P["mass"], P["Ib"], *(s[k][:1] for k in AR.INPUTS), dt, {"Rwb": bars["Rwb"][:1]})
    M = bars["Rwb"][0].reshape(3, 3) @ s["Rwb"][0].reshape(3, 3).T
    axial = np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    assert np.abs(axial).min() > 1e-3 and np.allclose(only_R["w_bar"][0], dt * axial, rtol=1e-12, atol=0)


# ------------------------------------------------------------------ the C ABI without a device
IO_FIELDS = ["struct_size", "Rwb", "x", "xdot", "w", "grf_body", "foot_world", "Rwb_next_bar", "x_next_bar", "xdot_next_bar", "w_next_bar",
             "feet_next_bar", "Rwb_bar", "x_bar", "xdot_bar", "w_bar", "grf_bar", "foot_world_bar", "dt"]


def test_symbols_are_exported_and_the_abi_stays(built):
    from quadruped_control_amd import _lib

    lib = ctypes.CDLL(os.path.join(ROOT, "quadruped_control_amd", "libqc_balance.so"))
    for name in ("qc_default_plant_adjoint", "qc_plant_step_adjoint_batch"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert _lib.load().qc_abi_version() == 6 and _lib.ABI_VERSION == 6  # new entry points, no change to what existed
    assert ctypes.sizeof(_lib.QcPlantIo) == 72
    for name in ("plant_step_autograd", "rollout_autograd", "control_batch_autograd"):
        assert callable(getattr(q, name)) and callable(getattr(q.BalanceController, name)), name
    assert callable(q.BalanceController.plant_step_adjoint) and callable(q.BalanceController.plan_plant_adjoint)


def test_mirror_matches_the_header(built, tmp_path):
    """sizeof and the member offsets of qc_plant_adjoint_io as the C compiler lays the header's struct out, against the ctypes
    mirror; qc_default_plant_adjoint fills the io as documented and needs no device."""
    from quadruped_control_amd import _lib

    fields = [f for f, _ in _lib.QcPlantAdjointIo._fields_]
    assert fields == IO_FIELDS
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qc_balance.h"\nint main(void) {\n  printf("%zu", sizeof(qc_plant_adjoint_io));\n'
                   + "".join(f'  printf(" %zu", offsetof(qc_plant_adjoint_io, {f}));\n' for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_lib.QcPlantAdjointIo) == 152
    assert got[1:] == [getattr(_lib.QcPlantAdjointIo, f).offset for f in fields]
    io = _lib.QcPlantAdjointIo()
    io.Rwb, io.x_bar, io.struct_size, io.dt = 123, 456, 7, -1.0
    _lib.load().qc_default_plant_adjoint(ctypes.byref(io))
    assert io.struct_size == 152 and io.dt == 1.0 / 300.0
    assert all(getattr(io, f) is None for f in fields[1:-1])


def test_argument_check_needs_no_device(built):
    """qc_plant_step_adjoint_batch refuses a bad call before it touches the device - the handle is null, so every call below ends in
    the argument check - and the message is its own."""
    from quadruped_control_amd import _lib

    lib = _lib.load()
    io = _lib.QcPlantAdjointIo()
    lib.qc_default_plant_adjoint(ctypes.byref(io))
    assert lib.qc_plant_step_adjoint_batch(None, 1, ctypes.byref(io), None) == -1
    assert _lib.last_error() == "qc_plant_step_adjoint_batch: null argument"
    assert lib.qc_plant_step_adjoint_batch(None, 0, None, None) == -1 and _lib.last_error() == "qc_plant_step_adjoint_batch: null argument"


def test_host_logic_without_a_device():
    """check_plant_adjoint_args through every refusal - a null handle or io, a wrong struct_size, a bad dt, no cotangent, no output,
    each missing input, n beyond one launch - with its message, and plant_adjoint_constants (csrc/qc_host.hpp), in a stand-alone
    program built with the address and undefined-behaviour sanitizers (tests/cpp/plant_adjoint_host_test.cpp)."""
    import __graft_entry__ as g

    assert "plant_adjoint_host_test" in g.HOST_TESTS
    exe = g.build_host_test("plant_adjoint_host_test")
    assert exe is not None and os.path.exists(exe)
    libs = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "amdhip64" not in libs and "qc_balance" not in libs, libs
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "plant adjoint host logic ok" in r.stdout, r.stdout[-3000:]
