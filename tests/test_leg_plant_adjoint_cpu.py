"""CPU: the legged plant step's reverse pass restated (tests/leg_plant_adjoint_restatement.py) against central differences of
leg_plant_restatement's forward step, the float64 pass against the 50-digit pass in units of EPS x condition sum (measured here,
recorded as C_NP there; tests/test_gpu_leg_plant_adjoint.py holds the device to 4 C_NP of the same scale), the identity
dIK / dp = J(qn)^-1 the kernel relies on, the flagged robots' bits, and the C ABI of qc_leg_plant_step_adjoint_batch as far as it goes
without a device."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import quadruped_control_amd as q
from quadruped_control_amd import _lib
from tests import leg_plant_adjoint_restatement as LA
from tests import leg_plant_restatement as LR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EPS = LA.EPS


@pytest.fixture(scope="module")
def P(built):
    return q.cheetah_params()


def _np(P, s, mask, bars, **kw):  # (kin=: the model, default the library's)
    return LA.leg_plant_adjoint_np(P["mass"], P["Ib"], *(s[k] for k in LA.INPUTS), mask, LA.INERTIA, LA.DT, bars, **kw)


def test_pool_covers_what_it_says(P):
    """The unflagged pool: all 16 contact masks, the identity and a rotation by nearly pi, a step angle of exactly 0, a leg on which
    wrapPI acts, torques at the clamp values; the margins of leg_plant_restatement's pools; no robot flagged by either pass."""
    s, mask, bars = LA.pool()
    assert set((mask * [1, 2, 4, 8]).sum(axis=1).tolist()) == set(range(16)) and mask[0].all() and not mask[15].any()
    R = s["Rwb"].reshape(-1, 3, 3)
    assert np.array_equal(R[0], np.eye(3)) and np.trace(R[1]) < -1 + 1e-8
    step = LR.leg_plant_step_np(P["mass"], P["Ib"], *(s[k] for k in LA.INPUTS), mask, LA.INERTIA, LA.DT)
    assert not step["flags"].any()
    assert not step["w"][15].any() and np.array_equal(step["Rwb"][15], s["Rwb"][15])  # a step angle of exactly 0
    raw = step["joint_q"].reshape(-1, 4, 3)[2, 0] - s["joint_q"].reshape(-1, 4, 3)[2, 0]
    assert mask[2, 0] and np.all(np.abs(raw + LA.TWO_PI) < 0.1) and np.all(np.abs(step["joint_qdot"].reshape(-1, 4, 3)[2, 0]) < 0.1 / LA.DT)
    lo, hi = LA.tau_limits()
    assert np.isfinite([lo, hi]).all() and mask[3, 2:].all() and set(s["joint_tau"].reshape(-1, 4, 3)[3, 2:].ravel().tolist()) == {lo, hi}
    dmax, detmin = LR.pool_margins(s["joint_q"], mask)
    assert dmax <= 0.9 and detmin > 1e4
    dmax, detmin = LR.pool_margins(step["joint_q"], mask)
    assert dmax <= 0.9 and detmin > 1e4
    _, flags = LA.pool_reference()
    assert not flags.any() and not _np(P, s, mask, bars)["flags"].any()


def test_restatement_against_50_digits_on_the_pool(P):
    """The float64 pass against leg_plant_adjoint_mp on the pool, every output entry, in units of EPS x condition sum: c_np"""
    _restatement_against_50_digits(P, "default")


def test_restatement_against_50_digits_on_the_pool_at_the_odd_model(P):
    """The same at ODD_KIN, against C_NP_ODD; and the odd pool's conditions on the reference alone: all 16 masks, no robot flagged by
    the forward step or by either pass, the pools' margins (|d| <= 0.9, det J far inside the leg's own band) before and after the
    step, torques inside the model's limits with two legs at the clamp values."""
    from tests.device_math_reference import ODD_KIN

    s, mask, bars = LA.pool(ODD_KIN)
    assert set((mask * [1, 2, 4, 8]).sum(axis=1).tolist()) == set(range(16))
    step = LR.leg_plant_step_np(P["mass"], P["Ib"], *(s[k] for k in LA.INPUTS), mask, LA.INERTIA, LA.DT, kin=ODD_KIN)
    assert not step["flags"].any()
    for jq in (s["joint_q"], step["joint_q"]):
        dmax, detmin = LR.pool_margins(jq, mask, ODD_KIN)
        assert dmax <= 0.9 and detmin > 1e4
    lo, hi = LA.tau_limits(ODD_KIN)
    assert (lo, hi) == (ODD_KIN.tau_min, ODD_KIN.tau_max) and s["joint_tau"].min() == lo and s["joint_tau"].max() == hi
    _restatement_against_50_digits(P, "odd")


def _restatement_against_50_digits(P, model):
    from tests.device_math_reference import KINS

    kin = KINS[model]
    s, mask, bars = LA.pool(kin)
    ref, flags = LA.pool_reference(kin)
    an = _np(P, s, mask, bars, kin=kin)
    assert not flags.any() and not an["flags"].any()
    worst = {}
    for k in LA.OUTPUTS:
        val, cond = ref[k]
        live = cond > 0  # (a stance leg's joint_qdot_bar is an exact 0 with condition sum 0)
        assert np.array_equal(an[k][~live], val[~live])
        worst[k] = float((np.abs(an[k] - val)[live] / (EPS * cond[live])).max())
    print("c_np", model, worst)
    for k in LA.OUTPUTS:
        assert worst[k] <= LA.C_NP_OF[model][k], (k, worst[k])


def test_ik_derivative_is_the_inverse_jacobian_at_50_digits(P):
    """dIK / dp = J(qn)^-1 on the unflagged pool: the 50-digit pass with the IK end reversed operation by operation (the atan2 / sqrt
    chain as written) against the same pass with p'_bar = J(qn)^-T qn_bar, every output entry, to 1e-40 of the condition sum - the
    two are the same derivative of a leg in reach on the q3 <= 0 branch, so only the 50-digit rounding separates them."""
    s, mask, bars = LA.pool()
    ref, _ = LA.pool_reference()
    worst = 0.0
    for i in range(0, LA.POOL, 4):
        if not mask[i].any():
            continue
        jac, flags = LA.leg_plant_adjoint_mp(P["mass"], P["Ib"], *(s[k][i] for k in LA.INPUTS), mask[i], LA.INERTIA, LA.DT,
                                             {k: v[i] for k, v in bars.items()}, ik="jacobian")
        assert flags == 0
        for k in LA.OUTPUTS:
            val, cond = ref[k][0][i], ref[k][1][i]
            live = cond > 0
            worst = max(worst, float((np.abs(jac[k][0] - val)[live] / cond[live]).max(initial=0.0)))
    print("worst |chain - jacobian| / condition sum, after rounding to double:", worst)
    assert worst <= 2 * EPS  # both are rounded to double on return: one rounding each of values no larger than their condition sums


def test_ik_derivative_identity_unrounded():
    """The same identity on the IK alone, without the rounding to double: (dIK / dp)^T w by the reversed chain against J(qn)^-T w at 50
    digits, on the stance legs of the pool's feet - relative 1e-40."""
    import mpmath as mp

    s, mask, _ = LA.pool()
    rng = np.random.default_rng(5)
    worst = 0.0
    with mp.workdps(LA.DPS):
        for i in range(0, LA.POOL, 8):
            for l in range(4):
                if not mask[i, l]:
                    continue
                pb = [LA.Cs(LA.mpf(v)) for v in LR.fk(l, s["joint_q"].reshape(-1, 4, 3)[i, l])]
                qn, d, tape = LA._ik(LA._Mp, l, pb)
                w = [LA.Cs(LA.mpf(v)) for v in rng.normal(size=3)]
                a = LA._ik_reverse(LA._Mp, tape, w)
                b = LA._Leg(LA._Mp, l, qn).solve_t(w)
                scale = max(abs(t.v) for t in b)
                worst = max(worst, float(max(abs(x.v - y.v) for x, y in zip(a, b)) / scale))
    print("worst relative |chain - J^-T|:", worst)
    assert worst < 1e-40


def test_flagged_rows_carry_exactly_the_expected_bits_at_the_odd_model(P):
    """The flagged pool rebuilt from ODD_KIN's hip and links: exactly FLAGGED's bits in the forward step and in both passes."""
    from tests.device_math_reference import ODD_KIN

    _flagged_bits(P, ODD_KIN)


def _flagged_bits(P, kin):
    s, mask, bars, expected = LA.flagged_pool(kin)
    step = LR.leg_plant_step_np(P["mass"], P["Ib"], *(s[k] for k in LA.INPUTS), mask, LA.INERTIA, LA.DT, kin=kin)
    assert np.array_equal(step["flags"], expected)
    an = _np(P, s, mask, bars, kin=kin)
    assert np.array_equal(an["flags"], expected) and all(np.isnan(an[k]).all() for k in LA.OUTPUTS)
    for i in range(len(expected)):
        ref, flags = LA.leg_plant_adjoint_mp(P["mass"], P["Ib"], *(s[k][i] for k in LA.INPUTS), mask[i], LA.INERTIA, LA.DT,
                                             {k: v[i] for k, v in bars.items()}, kin=kin)
        assert flags == expected[i] and all(np.isnan(ref[k][0]).all() for k in LA.OUTPUTS)
    return s, step


def test_flagged_rows_carry_exactly_the_expected_bits(P):
    """The small flagged pool: the stretched leg, the leg with d < -1 and the singular J(q) carry exactly FLAGGED's bits in both
    passes and in the forward step itself, and every output row is NaN."""
    from tests.device_math_reference import DEFAULT_KIN

    s, step = _flagged_bits(P, DEFAULT_KIN)
    # the margins that make the bits unambiguous: the knee cosines after the step, and the determinants before it
    d0 = LR.knee_cosine(0, np.eye(3) @ (LR.fk(0, s["joint_q"].reshape(-1, 4, 3)[0, 0]) + s["x"][0] - step["x"][0]))
    d1 = LR.knee_cosine(1, np.eye(3) @ (LR.fk(1, s["joint_q"].reshape(-1, 4, 3)[1, 1]) + s["x"][1] - step["x"][1]))
    assert d0 > 1 + 1e-3 and d1 < -1 - 1e-3
    assert abs(LR.det3(LR.jacobian(2, s["joint_q"].reshape(-1, 4, 3)[2, 2]))) < 1e-3 * LR.DET_LO
    assert abs(LR.det3(LR.jacobian(2, step["joint_q"].reshape(-1, 4, 3)[2, 2]))) > 1e6 * LR.DET_LO


def test_50_digit_pass_against_central_differences_of_the_step(P):
    """<x_bar, v> of the 50-digit pass against central differences of leg_plant_step_np's loss <c, y> along the committed directions v
    in all seven inputs at once, on the first 65 robots of the pool (unflagged: test_pool_covers_what_it_says).  The step is smooth
    off the flagged legs: every robot is kept.  Bar: fd_bar.  The sweep (LEG_ADJOINT_SWEEP=1 prints it; worst over the robots, relative
    to |x_bar| |v|):
      h      worst error  worst t    median error
      1e-3   2.6e-04      7.8e-04    1.2e-06
      1e-4   2.6e-06      7.7e-06    1.2e-08
      1e-5   2.6e-08      7.7e-08    1.1e-10
      1e-6   2.6e-10      7.6e-10    8.0e-12
      1e-7   1.9e-10      2.2e-10    5.7e-11
      1e-8   2.1e-09      2.4e-09    5.6e-10
    The error falls as h^2 down to 1e-6 and is rounding below: h = 1e-6, the last step at which the truncation estimate still is one."""
    n = LA.FD_N
    s, mask, bars = ({k: a[:n] for k, a in d.items()} if isinstance(d, dict) else d[:n] for d in LA.pool())
    v = LA.fd_directions()
    ref, _ = LA.pool_reference()
    an = {k: val[:n] for k, (val, _) in ref.items()}
    cond = {k: c[:n] for k, (_, c) in ref.items()}
    step = lambda d: LR.leg_plant_step_np(P["mass"], P["Ib"], *(d[k] for k in LA.INPUTS), mask, LA.INERTIA, LA.DT)
    dd = sum((an[LA.BAR_OF[k]] * v[k]).sum(axis=1) for k in LA.INPUTS)
    scale = np.sqrt(sum((an[LA.BAR_OF[k]] ** 2).sum(axis=1) for k in LA.INPUTS)) * np.sqrt(sum((v[k] ** 2).sum(axis=1) for k in LA.INPUTS))
    if os.environ.get("LEG_ADJOINT_SWEEP"):
        for h in (1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8):
            fd1, fd2 = LA.fd_of(step, s, bars, v, h)
            print("h %g worst error %.1e worst t %.1e median error %.1e" % (h, (np.abs(fd1 - dd) / scale).max(), (np.abs(fd1 - fd2) / scale).max(),
                                                                          np.median(np.abs(fd1 - dd) / scale)))
    h = LA.FD_H
    fd1, fd2 = LA.fd_of(step, s, bars, v, h)
    bar = LA.fd_bar(P, s, mask, bars, v, cond, fd1, fd2, h)
    err = np.abs(fd1 - dd)
    print("worst relative error", float((err / scale).max()), "worst bar", float((bar / scale).max()), "worst error / bar", float((err / bar).max()))
    assert (scale > 0).all() and np.median(bar / scale) < 1e-5
    assert np.all(err <= bar), float((err / bar).max())


def test_each_input_cotangent_is_seen(P):
    """A guard on the test above: along a direction in ONE input the float64 pass agrees with the difference quotient input by input,
    and the derivative is not negligible on most robots (joint_qdot: on the robots with a swing leg)."""
    n, h = LA.FD_N, LA.FD_H
    s, mask, bars = ({k: a[:n] for k, a in d.items()} if isinstance(d, dict) else d[:n] for d in LA.pool())
    an = _np(P, s, mask, bars)
    step = lambda d: LR.leg_plant_step_np(P["mass"], P["Ib"], *(d[k] for k in LA.INPUTS), mask, LA.INERTIA, LA.DT)
    for name in LA.INPUTS:
        v = {k: (a if k == name else np.zeros_like(a)) for k, a in LA.fd_directions().items()}
        fd1, fd2 = LA.fd_of(step, s, bars, v, h)
        dd = (an[LA.BAR_OF[name]] * v[name]).sum(axis=1)
        assert np.mean(np.abs(dd) > 1e-4 * np.abs(an[LA.BAR_OF[name]]).max(axis=1)) > 0.5, name
        assert np.all(np.abs(fd1 - dd) <= np.abs(fd1 - fd2) + 1e-6 * (1.0 + np.abs(dd))), (name, float(np.abs(fd1 - dd).max()))


def test_zero_cotangents_give_zeros(P):
    s, mask, bars = LA.pool()
    zero = _np(P, {k: v[:32] for k, v in s.items()}, mask[:32], {k: np.zeros_like(v[:32]) for k, v in bars.items()})
    assert all(not zero[k].any() for k in LA.OUTPUTS)


def test_cpu_loop_meets_the_rollout_tests_keep_rule(P):
    """The GPU test of rollout_tick_autograd keeps a robot that is solved and unflagged at every step of every point, with the working
    set and the torques' clamp mask of every step unchanged at +-h, +-2h (h = 1e-4) along the state directions and along the gains'
    direction, and asks for at least 0.5 of the robots.  Here the CPU loop alone - the C oracle's tick, the certificate's working set
    of its forces, leg_plant_step_np - under that rule on the same start and directions (leg_plant_adjoint_restatement.rollout_case):
    kept 0.815 (53 of 65).  The same start with all four feet exactly on the home rectangle keeps 0.09: the balance QP is degenerate
    there, and the joint_q direction alone changes the working set of four robots in five at step 0 (stand_start's docstring)."""
    keep = LA.cpu_rollout_kept(P)
    print("kept", keep.mean())
    assert keep.mean() >= 0.5, keep.mean()


# ------------------------------------------------------------------ the C ABI without a device
IO_FIELDS = [f for f, _ in _lib.QcLegPlantAdjointIo._fields_]


def test_symbols_are_exported_and_the_abi_stays(built):
    lib = _lib.load()
    for name in ("qc_default_leg_plant_adjoint", "qc_leg_plant_step_adjoint_batch"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert lib.qc_abi_version() == 6 == _lib.ABI_VERSION
    for name in ("plan_leg_plant_adjoint", "leg_plant_step_adjoint", "leg_plant_step_autograd", "rollout_tick_autograd"):
        assert callable(getattr(q.BalanceController, name))


def test_io_layout_matches_the_header(built, tmp_path):
    """sizeof and the member offsets of qc_leg_plant_adjoint_io as the C compiler lays the header's struct out, against the ctypes
    mirror; qc_default_leg_plant_adjoint fills the io as documented and needs no device."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qc_balance.h"\nint main(void) {\n  printf("%zu", sizeof(qc_leg_plant_adjoint_io));\n'
                   + "".join(f'  printf(" %zu", offsetof(qc_leg_plant_adjoint_io, {f}));\n' for f in IO_FIELDS) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(t) for t in subprocess.check_output([str(exe)]).split()]
    assert got[0] == ctypes.sizeof(_lib.QcLegPlantAdjointIo) == (1 + 25 + 3 + 1) * 8
    assert got[1:] == [getattr(_lib.QcLegPlantAdjointIo, f).offset for f in IO_FIELDS]
    io = _lib.QcLegPlantAdjointIo()
    ctypes.memset(ctypes.byref(io), 0xFF, ctypes.sizeof(io))
    _lib.load().qc_default_leg_plant_adjoint(ctypes.byref(io))
    assert io.struct_size == ctypes.sizeof(io) and io.dt == 1.0 / 300.0 and list(io.leg_inertia) == [0.0] * 3
    assert all(getattr(io, f) is None for f in IO_FIELDS[1:-2])
    _lib.load().qc_default_leg_plant_adjoint(None)  # a null record is left alone


def test_refusals_before_the_device(built):
    """qc_leg_plant_step_adjoint_batch refuses a bad call before it touches the device - the handle is null, so every call below ends
    in the argument check."""
    lib = _lib.load()
    io = _lib.QcLegPlantAdjointIo()
    lib.qc_default_leg_plant_adjoint(ctypes.byref(io))
    for args in ((None, 1, ctypes.byref(io), None), (None, 0, ctypes.byref(io), None), (None, 1, None, None)):
        assert lib.qc_leg_plant_step_adjoint_batch(*args) == -1 and _lib.last_error() == "qc_leg_plant_step_adjoint_batch: null argument"


def test_host_logic_under_sanitizers(built):
    """check_leg_plant_adjoint_args through every refusal with its message, and leg_plant_adjoint_constants (csrc/qc_host.hpp), in a
    stand-alone program built with the address and undefined-behaviour sanitizers (tests/cpp/leg_plant_adjoint_host_test.cpp)."""
    import __graft_entry__ as g

    assert "leg_plant_adjoint_host_test" in g.HOST_TESTS
    exe = g.build_host_test("leg_plant_adjoint_host_test")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "leg plant adjoint host logic ok" in r.stdout, r.stdout
