"""CPU: the swing-leg torque adjoint's restatement (tests/sensitivity_swing_restatement.py) - its float64 evaluation against its
50-digit one, the identity dIK / dp = J(q_ref)^-1 against the 50-digit derivative of the atan2 chain as written, central differences
of oracle/tick_restatement.py's swing torque, the flag bits on constructed legs - and the C ABI of qc_sensitivity_swing_batch as far
as it goes without a device.

Measured (committed seeds): test_float64_against_50_digits prints the float64 restatement's worst distance from the 50-digit pass per
output, in EPS x condition sum; SW.C_SWING holds those figures rounded up, and the GPU test's bar is 4 x C_SWING."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import sensitivity_swing_restatement as SW
from tests.device_math_reference import KINS, ODD_KIN

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EPS = 2.0 ** -52
N_CPU = 65  # the first robots of the pool: every pattern of SW.masks() thirteen times over


def _case(kin):
    b = {k: v[:N_CPU] for k, v in SW.model_pool(kin).items()}
    swing = SW.masks(N_CPU) == 0
    tb, ins = SW.cotangent(N_CPU), {k: v[:N_CPU] for k, v in SW.accumulators(N_CPU).items()}
    ref, cond, flags, raw = SW.swing_adjoint_mp(b, swing, tb, kin=kin, **ins)
    return dict(b=b, swing=swing, tb=tb, ins=ins, ref=ref, cond=cond, flags=flags, raw=raw, kin=kin)


@pytest.fixture(scope="module")
def case():
    return _case(KINS["default"])


@pytest.fixture(scope="module")
def cases(case):
    """the default model's case (the one every default-only test uses) and ODD_KIN's"""
    class Lazy(dict):  # (ODD_KIN's pass is built when an odd-model test first asks for it)
        def __missing__(self, model):
            self[model] = _case(KINS[model])
            return self[model]

    return Lazy(default=case)


def test_the_pool_is_in_reach_and_unclamped(case):
    """Every swing leg of the pool is unflagged, every torque strictly inside the limits, |q_ref - q| < 0.2 rad (no wrap is crossed),
    and every contact pattern of the issue is there."""
    c = case
    assert not c["flags"].any()
    raw = c["raw"][c["swing"]]
    assert np.isfinite(raw).all() and (np.abs(raw) < 19.0).all(), np.abs(raw).max()
    pats = {tuple(r) for r in (~c["swing"]).astype(int).tolist()}
    assert set(SW.PATTERNS) <= pats and len(pats) > len(SW.PATTERNS)
    kp = np.asarray(SW.KP)
    for i in range(N_CPU):
        for leg in range(4):
            out, bad, _ = SW._swing_leg(SW._Float, leg, c["b"]["Rwb"][i], c["b"]["x"][i], c["b"]["swing_pos"][i, 3 * leg:3 * leg + 3],
                                        c["b"]["swing_vel"][i, 3 * leg:3 * leg + 3], c["b"]["joint_q"][i, 3 * leg:3 * leg + 3],
                                        c["b"]["joint_qdot"][i, 3 * leg:3 * leg + 3], kp / kp, "jacobian")
            assert not bad and (np.abs(out["gain_bar"][:3]) < 0.2).all()  # s = 1: gain_bar's first three are e


def test_the_odd_pool_is_in_reach_and_clamped_on_both_sides(cases):
    """ODD_KIN's pool, on the 50-digit reference alone: no swing leg is flagged; in every joint at least one torque is clamped at
    tau_min, one at tau_max and one passes; some torques sit within |kff| of a limit on either side of it (dropping kff flips their
    mask); every contact pattern is there."""
    c, kin = cases["odd"], ODD_KIN
    assert not c["flags"].any()
    assert kin.tau_min != -kin.tau_max and all(v != 1.0 for v in kin.jc_kd) and all(v != 0.0 for v in kin.jc_kff)
    for j in range(3):
        raw = c["raw"][:, :, j][c["swing"]]
        assert np.isfinite(raw).all()
        low, high = raw < kin.tau_min, raw > kin.tau_max
        assert low.any() and high.any() and (~low & ~high).any(), j
        without = raw - kin.jc_kff[j]
        flips = ((without < kin.tau_min) != low) | ((without > kin.tau_max) != high)
        print(f"joint {j}: {int(low.sum())} at tau_min, {int(high.sum())} at tau_max, {int((~low & ~high).sum())} pass, {int(flips.sum())} masks flip without kff")
        assert flips.any(), j
    pats = {tuple(r) for r in (~c["swing"]).astype(int).tolist()}
    assert set(SW.PATTERNS) <= pats and len(pats) > len(SW.PATTERNS)


def test_float64_against_50_digits(cases):
    """_float64_against_50_digits at the default model: C_SWING"""
    _float64_against_50_digits(cases, "default")


def test_float64_against_50_digits_at_the_odd_model(cases):
    """_float64_against_50_digits at ODD_KIN: C_SWING_ODD"""
    _float64_against_50_digits(cases, "odd")


def _float64_against_50_digits(cases, model):
    """C_SWING, C_SWING_ODD: the float64 restatement (the kernel's identity at the IK end) against the 50-digit pass (the atan2 chain
    reversed as written), per output in EPS x condition sum - asserted and recorded - at the default model and at ODD_KIN."""
    c = cases[model]
    kin, C = c["kin"], SW.C_SWING_OF[model]
    val, flags, raw = SW.swing_adjoint_np(c["b"], c["swing"], c["tb"], kin=kin, **c["ins"])
    assert (flags == c["flags"]).all()
    assert ((raw < kin.tau_min) == (c["raw"] < kin.tau_min)).all() and ((raw > kin.tau_max) == (c["raw"] > kin.tau_max)).all()
    for k in SW.OUTPUTS:
        live = c["cond"][k] > 0
        assert (val[k][~live] == c["ref"][k][~live]).all(), k  # stance rows: zeros, or the accumulator, exactly
        worst = float(np.max(np.abs(val[k] - c["ref"][k])[live] / (EPS * c["cond"][k][live])))
        print(f"C_SWING[{model}] {k}: {worst:.4f} (recorded {C[k]})")
        assert worst <= C[k], (k, worst)


def test_ik_derivative_is_the_inverse_jacobian(case):
    """dIK / dp = J(q_ref)^-1: the 50-digit pass with the atan2 chain reversed operation by operation against the 50-digit pass with
    J(q_ref)^-T, on the outputs behind the IK.  Both are exact to ~1e-50 of their condition sums; bar 1e-40."""
    c = case
    jac, cond, _, _ = SW.swing_adjoint_mp(c["b"], c["swing"], c["tb"], ik="jacobian", **c["ins"])
    import mpmath as mp
    with mp.workdps(SW.DPS):
        for i in range(0, N_CPU, 4):
            for leg in range(4):
                args = (leg, c["b"]["Rwb"][i], c["b"]["x"][i], c["b"]["swing_pos"][i, 3 * leg:3 * leg + 3], c["b"]["swing_vel"][i, 3 * leg:3 * leg + 3],
                        c["b"]["joint_q"][i, 3 * leg:3 * leg + 3], c["b"]["joint_qdot"][i, 3 * leg:3 * leg + 3], c["tb"][i, 3 * leg:3 * leg + 3])
                a, _, _ = SW._swing_leg(SW._Mp, *args, "chain")
                j, _, _ = SW._swing_leg(SW._Mp, *args, "jacobian")
                for k in ("swing_pos_bar", "Rwb_bar", "x_bar"):
                    for u, v in zip(a[k], j[k]):
                        assert abs(u.v - v.v) <= mp.mpf(10) ** -40 * mp.mpf(max(u.c, v.c, 1e-300)), (i, leg, k)
    for k in SW.OUTPUTS:  # and rounded to double the two passes are one
        assert np.allclose(jac[k], c["ref"][k], rtol=1e-13, atol=0.0, equal_nan=True), k


DIRECTIONS = ("swing_pos", "swing_vel", "x", "Rwb", "joint_q", "joint_qdot")
FD_H = 1e-6


def test_central_differences_of_the_oracle_swing_torque(case):
    """<gradient, v> of L = <joint_tau_bar, tau_raw> against central differences of oracle/tick_restatement.py's own swing torque, one
    committed direction per input.  h = 1e-6: truncation h^2 L''' / 6 ~ 1e-12 x 1e4 (kp / link^3 scale of the IK's third derivative)
    = 1e-8 of the direction's size, rounding EPS |L| / h ~ 2e-16 x 300 / 1e-6 = 7e-8.  Bar: 1e-6 of sum |gradient_i v_i| + 1e-6.
    No case is excluded: every torque of the pool is strictly inside the limits at every point (asserted)."""
    c = case
    b, swing, tb = c["b"], c["swing"], c["tb"].reshape(N_CPU, 4, 3)
    val, _, _ = SW.swing_adjoint_np(b, swing, c["tb"])
    rng = np.random.default_rng(41)
    sizes = {"swing_pos": 12, "swing_vel": 12, "x": 3, "Rwb": 9, "joint_q": 12, "joint_qdot": 12}

    def loss(bb):
        tot = np.zeros(N_CPU)
        for i in range(N_CPU):
            for leg in range(4):
                if swing[i, leg]:
                    sl = slice(3 * leg, 3 * leg + 3)
                    tau = SW.swing_torque(leg, bb["Rwb"][i], bb["x"][i], bb["swing_pos"][i, sl], bb["swing_vel"][i, sl], bb["joint_q"][i, sl], bb["joint_qdot"][i, sl])
                    assert (np.abs(tau) < 19.5).all()
                    tot[i] += float(tb[i, leg] @ tau)
        return tot

    excluded = 0
    for name in DIRECTIONS:
        v = rng.uniform(-1.0, 1.0, (N_CPU, sizes[name]))
        fd = (loss(dict(b, **{name: b[name] + FD_H * v})) - loss(dict(b, **{name: b[name] - FD_H * v}))) / (2 * FD_H)
        grad = val[name + "_bar"].reshape(N_CPU, -1)
        an, scale = (grad * v).sum(axis=1), (np.abs(grad) * np.abs(v)).sum(axis=1)
        err = np.abs(fd - an)
        print(f"FD {name}: worst error {err.max():.3e}, worst error / bar {np.max(err / (1e-6 * scale + 1e-6)):.3f}")
        assert (err <= 1e-6 * scale + 1e-6).all(), (name, float(err.max()))
    assert excluded == 0


def test_flag_bits_on_constructed_legs():
    """_flag_bits_on_constructed_legs at the default model"""
    _flag_bits_on_constructed_legs("default")


def test_flag_bits_on_constructed_legs_at_the_odd_model():
    """_flag_bits_on_constructed_legs at ODD_KIN"""
    _flag_bits_on_constructed_legs("odd")


def _flag_bits_on_constructed_legs(model):
    """Stretched (d > 1), inside the hip roll's cylinder, a non-finite target and inside the inner reach limit (d < -1): the expected bit,
    NaN in that leg's rows and in the robot's Rwb_bar and x_bar, finite numbers everywhere else - in both arithmetics, at both models
    (the targets are placed from the model's own hip and links)."""
    kin = KINS[model]
    b, expect = SW.flagged_pool(kin)
    swing = np.ones((4, 4), bool)
    tb = SW.cotangent(4)
    for val, flags in (SW.swing_adjoint_np(b, swing, tb, kin=kin)[:2], (lambda r: (r[0], r[2]))(SW.swing_adjoint_mp(b, swing, tb, kin=kin))):
        assert (flags == expect).all(), flags
        for i in range(4):
            for k in SW.PER_LEG:
                bad = np.isnan(val[k][i]).all(axis=1)
                assert bad.tolist() == [leg == i for leg in range(4)] and np.isfinite(val[k][i][~bad]).all(), (i, k)
            for k in SW.PER_ROBOT:
                assert np.isnan(val[k][i]).all()


# ------------------------------------------------------------------ the C ABI without a device
IO_POINTERS = ("joint_tau_bar", "joint_q_bar_in", "Rwb_bar_in", "x_bar_in", "swing_pos_bar", "swing_vel_bar", "joint_q_bar", "joint_qdot_bar",
               "gain_bar", "Rwb_bar", "x_bar", "flags")


def test_symbols_are_exported_and_the_abi_stays(built):
    from quadruped_control_amd import _lib

    lib = ctypes.CDLL(os.path.join(ROOT, "quadruped_control_amd", "libqc_balance.so"))
    for name in ("qc_default_sensitivity_swing", "qc_sensitivity_swing_batch"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert _lib.load().qc_abi_version() == 6 and _lib.ABI_VERSION == 6  # new entry points, no change to what existed
    assert ctypes.sizeof(_lib.QcSensitivityKinIo) == 72 and ctypes.sizeof(_lib.QcLegPlantAdjointIo) == 240


def test_mirror_matches_the_header(built, tmp_path):
    """sizeof and the member offsets of qc_sensitivity_swing_io as the C compiler lays the header's struct out, against the ctypes
    mirror; qc_default_sensitivity_swing fills the io as documented and needs no device."""
    from quadruped_control_amd import _lib

    fields = [f for f, _ in _lib.QcSensitivitySwingIo._fields_]
    assert fields == ["struct_size"] + list(IO_POINTERS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qc_balance.h"\nint main(void) {\n  printf("%zu", sizeof(qc_sensitivity_swing_io));\n'
                   + "".join(f'  printf(" %zu", offsetof(qc_sensitivity_swing_io, {f}));\n' for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_lib.QcSensitivitySwingIo) == 104
    assert got[1:] == [getattr(_lib.QcSensitivitySwingIo, f).offset for f in fields]
    io = _lib.QcSensitivitySwingIo()
    io.joint_tau_bar, io.flags, io.struct_size = 123, 456, 7
    _lib.load().qc_default_sensitivity_swing(ctypes.byref(io))
    assert io.struct_size == 104
    assert all(getattr(io, f) is None for f in IO_POINTERS)


def test_argument_check_needs_no_device(built):
    """qc_sensitivity_swing_batch refuses a bad call before it touches the device - the handle is null, so every call below ends in the
    argument check."""
    from quadruped_control_amd import _lib

    lib = _lib.load()
    io = _lib.QcSensitivitySwingIo()
    lib.qc_default_sensitivity_swing(ctypes.byref(io))
    bi = _lib.QcBatchIn()
    for args in ((None, 1, ctypes.byref(bi), ctypes.byref(io), None), (None, 0, ctypes.byref(bi), None, None), (None, 1, None, ctypes.byref(io), None)):
        assert lib.qc_sensitivity_swing_batch(*args) == -1 and _lib.last_error() == "qc_sensitivity_swing_batch: null argument"


def test_host_logic_without_a_device():
    """check_sensitivity_swing_args through every refusal - a null handle, `in` or `io`, a wrong struct_size, swing_state, gait_dt, no
    output, no joint_tau_bar, each of the six arrays missing, n beyond one launch - and the accepted combinations, every output alone
    among them, with its message (csrc/qc_host.hpp), in a stand-alone program built with the address and undefined-behaviour
    sanitizers (tests/cpp/sensitivity_swing_host_test.cpp)."""
    import __graft_entry__ as g

    assert "sensitivity_swing_host_test" in g.HOST_TESTS
    exe = g.build_host_test("sensitivity_swing_host_test")
    assert exe is not None and os.path.exists(exe)
    libs = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "amdhip64" not in libs and "qc_balance" not in libs, libs
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "sensitivity swing host logic ok" in r.stdout, r.stdout[-3000:]
