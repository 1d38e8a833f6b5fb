"""CPU: the swing legs' torque tangent's restatement (tests/swing_tangent_restatement.py) - its float64 evaluation against its 50-digit
one (C_ST), the pairing with the adjoint's restatement (C_SDOT), central differences of the restated forward torque, the pass-through
of stance rows and masked entries, the flag bits on constructed legs - and the C ABI of qc_swing_torque_tangent_batch as far as it
goes without a device: the exports, the ctypes mirror against the header, the sanitized host program, the Python refusals.

Measured (committed seeds): the two 50-digit tests print the worst distances; ST.C_ST and ST.C_SDOT hold them rounded up."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import sensitivity_swing_restatement as SW
from tests import swing_tangent_restatement as ST
from tests.device_math_reference import KINS

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EPS = 2.0 ** -52
N_CPU, K_CPU = 65, 3  # the first robots of the pool: every pattern of SW.masks() thirteen times over; three directions


def _case(kin):
    b = {k: v[:N_CPU] for k, v in SW.model_pool(kin).items()}
    swing = SW.masks(N_CPU) == 0
    tans = ST.random_tangents(N_CPU, K_CPU)
    ref, cond, flags, raw = ST.swing_tangent_mp(b, swing, tans, kin=kin)
    return dict(b=b, swing=swing, tans=tans, ref=ref, cond=cond, flags=flags, raw=raw, kin=kin)


@pytest.fixture(scope="module")
def cases():
    class Lazy(dict):  # (a model's 50-digit pass is built when a test first asks for it)
        def __missing__(self, model):
            self[model] = _case(KINS[model])
            return self[model]

    return Lazy()


@pytest.mark.parametrize("model", ("default", "odd"))
def test_float64_against_50_digits(cases, model):
    """C_ST: the float64 restatement (dq_ref = J^-1 dp_b, the kernel's identity) against the 50-digit pass (the atan2 chain
    differentiated as written), per entry in EPS x condition sum - printed, asserted below the recorded figure.  Entries with condition
    sum 0 (stance rows, masked entries) are exact.  The odd model's pool is clamped on both sides in every joint: the two masks agree."""
    c = cases[model]
    kin = c["kin"]
    val, flags, raw = ST.swing_tangent_np(c["b"], c["swing"], c["tans"], kin=kin)
    assert not flags.any() and not c["flags"].any()
    assert ((raw < kin.tau_min) == (c["raw"] < kin.tau_min)).all() and ((raw > kin.tau_max) == (c["raw"] > kin.tau_max)).all()
    live = c["cond"] > 0
    assert live.any() and np.array_equal(val[~live], c["ref"][~live])
    worst = float(np.max(np.abs(val - c["ref"])[live] / (EPS * c["cond"][live])))
    print(f"C_ST[{model}]: {worst:.4f} (recorded {ST.C_ST[model]})")
    assert worst <= ST.C_ST[model], worst
    if model == "odd":
        swing3 = np.broadcast_to(c["swing"][:, :, None], raw.shape)
        assert ((raw < kin.tau_min) & swing3).any() and ((raw > kin.tau_max) & swing3).any()


def test_ik_derivative_is_the_inverse_jacobian(cases):
    """dIK / dp = J(q_ref)^-1 in forward mode: the two 50-digit passes agree to 1e-13 of the value once rounded (they are one function)"""
    c = cases["default"]
    jac = ST.swing_tangent_mp(c["b"], c["swing"], c["tans"], ik="jacobian")[0]
    assert np.allclose(jac, c["ref"], rtol=1e-13, atol=0.0)


@pytest.mark.parametrize("model", ("default", "odd"))
def test_pairing_with_the_adjoint(cases, model):
    """C_SDOT: <joint_tau_bar, dtau - joint_tau_tan_in> against the pairing of the tangents with swing_adjoint_np's cotangents, in EPS x
    the sum of the magnitudes of all terms on both sides - printed, asserted below the recorded figure."""
    c = cases[model]
    kin = c["kin"]
    tb = SW.cotangent(N_CPU)
    bars, flags, _ = SW.swing_adjoint_np(c["b"], c["swing"], tb, kin=kin)
    val, _, _ = ST.swing_tangent_np(c["b"], c["swing"], c["tans"], kin=kin)
    assert not flags.any()
    lhs, rhs, terms = ST.pairing(tb, val, c["tans"], bars, c["b"]["Rwb"])
    live = c["swing"].any(axis=1)
    assert (terms[:, live] > 0).all() and np.array_equal(lhs[:, ~live], rhs[:, ~live])  # (all stance: 0 = 0)
    worst = float(np.max(np.abs(lhs - rhs)[:, live] / (EPS * terms[:, live])))
    print(f"C_SDOT[{model}]: {worst:.4f} (recorded {ST.C_SDOT[model]})")
    assert worst <= ST.C_SDOT[model], worst


FD_H = 1e-5


def _clamped_torque(b, swing, kin):
    """the restated forward torque of every swing leg - oracle/tick_restatement.py's, at the default model - clamped; NaN for stance legs"""
    n = b["x"].shape[0]
    tau = np.full((n, 4, 3), np.nan)
    for i in range(n):
        for leg in range(4):
            if swing[i, leg]:
                sl = slice(3 * leg, 3 * leg + 3)
                tau[i, leg] = SW.swing_torque(leg, b["Rwb"][i], b["x"][i], b["swing_pos"][i, sl], b["swing_vel"][i, sl], b["joint_q"][i, sl], b["joint_qdot"][i, sl])
    return np.clip(tau, kin.tau_min, kin.tau_max), (tau <= kin.tau_min) | (tau >= kin.tau_max)


def test_central_differences_of_the_forward_torque():
    """The tangent against central differences of the restated, CLAMPED forward torque along three committed directions that move every
    input at once, on the saturated pool (every third leg clamped in one joint).  fd_support's rule: an entry is kept where the clamp
    mask is the base point's at -2h, -h, h, 2h (the pool crosses no wrap: |q_ref - q| stays below 1 rad); its bar is the truncation
    estimated from the differences alone, |FD(h) - FD(2h)|, plus 1e-6 |tangent| + 1e-6 for the rounding of the quotient (EPS x 20 N m /
    h = 4e-10) and of the analytic side.  At least 0.9 of the swing entries are kept, clamped ones (tangent 0) among them."""
    kin = KINS["default"]
    n = 33
    b = SW.pool(n, saturate=True)
    swing = SW.masks(n) == 0
    tans = ST.random_tangents(n, 3, seed=53)
    tans["joint_tau_tan_in"] = None
    val, flags, _ = ST.swing_tangent_np(b, swing, tans, kin=kin)
    assert not flags.any()
    base, cl0 = _clamped_torque(b, swing, kin)
    sw3 = np.broadcast_to(swing[:, :, None], base.shape)
    assert cl0[sw3].any() and not cl0[sw3].all()
    kept_all = 0
    for k in range(3):
        pts = {m: _clamped_torque(ST.moved(b, tans, k, m * FD_H), swing, kin) for m in (-2, -1, 1, 2)}
        keep = sw3.copy()
        for _, cl in pts.values():
            keep &= cl == cl0
        fd1, fd2 = (pts[1][0] - pts[-1][0]) / (2 * FD_H), (pts[2][0] - pts[-2][0]) / (4 * FD_H)
        err, bar = np.abs(fd1 - val[k]), np.abs(fd1 - fd2) + 1e-6 * np.abs(val[k]) + 1e-6
        print(f"direction {k}: kept {keep.sum()} of {sw3.sum()}, worst error / bar {np.max(err[keep] / bar[keep]):.3f}")
        assert keep.sum() >= 0.9 * sw3.sum() and (err[keep] <= bar[keep]).all()
        assert (val[k][keep & cl0] == 0.0).all() and (keep & cl0).any() and np.abs(val[k][keep & ~cl0]).min() > 0.0
        kept_all += int(keep.sum())
    assert kept_all > 0


def test_stance_rows_and_masked_entries_pass_the_input_through(cases):
    """A stance leg's row is joint_tau_tan_in bit for bit (0 where it is not given); so is a clamped entry of a swing leg."""
    kin = KINS["default"]
    n = 20
    b = SW.pool(n, saturate=True)
    swing = SW.masks(n) == 0
    tans = ST.random_tangents(n, 2, seed=59)
    val, flags, raw = ST.swing_tangent_np(b, swing, tans, kin=kin)
    tin = tans["joint_tau_tan_in"].reshape(2, n, 4, 3)
    clamped = (raw < kin.tau_min) | (raw > kin.tau_max)
    assert not flags.any() and clamped.any() and (~swing).any()
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    assert np.array_equal(bits(val[:, ~swing]), bits(tin[:, ~swing])) and np.array_equal(bits(val[:, clamped]), bits(tin[:, clamped]))
    passing = np.broadcast_to(swing[:, :, None], raw.shape) & ~clamped
    assert (val[:, passing] != tin[:, passing]).all()
    none = ST.swing_tangent_np(b, swing, dict(tans, joint_tau_tan_in=None), kin=kin)[0]
    assert not none[:, ~swing].any() and not none[:, clamped].any()


@pytest.mark.parametrize("model", ("default", "odd"))
def test_flag_bits_on_constructed_legs(model):
    """Every case of SW.flagged_pool() flags its bit and gives NaN in its row only, in every direction - in both arithmetics."""
    kin = KINS[model]
    b, expect = SW.flagged_pool(kin)
    swing = np.ones((4, 4), bool)
    tans = ST.random_tangents(4, 2, seed=61)
    for val, flags in (ST.swing_tangent_np(b, swing, tans, kin=kin)[:2], (lambda r: (r[0], r[2]))(ST.swing_tangent_mp(b, swing, tans, kin=kin))):
        assert (flags == expect).all(), flags
        for i in range(4):
            bad = np.isnan(val[:, i]).all(axis=(0, 2))
            assert bad.tolist() == [leg == i for leg in range(4)] and np.isfinite(val[:, i][:, ~bad]).all(), i


# ------------------------------------------------------------------ the C ABI without a device
IO_FIELDS = ("struct_size", "n_dir", "Rwb_rot_tan", "x_tan", "swing_pos_tan", "swing_vel_tan", "joint_q_tan", "joint_qdot_tan", "joint_tau_tan_in",
             "joint_tau_tan", "flags")


def test_symbols_are_exported_and_the_abi_stays(built):
    from quadruped_control_amd import _lib, tangent

    lib = ctypes.CDLL(os.path.join(ROOT, "quadruped_control_amd", "libqc_balance.so"))
    for name in ("qc_default_swing_tangent", "qc_swing_torque_tangent_batch"):
        assert hasattr(lib, name), name
    assert _lib.load().qc_abi_version() == 6 and _lib.ABI_VERSION == 6  # new entry points, no change to what existed
    bound = tangent._library()
    assert bound.qc_swing_torque_tangent_batch.restype is ctypes.c_int
    assert ctypes.sizeof(tangent.QcTorqueTangentIo) == 56 and ctypes.sizeof(tangent.QcLegPlantTangentIo) == 248 and ctypes.sizeof(tangent.QcTangentIo) == 136


def test_mirror_matches_the_header(built, tmp_path):
    """sizeof and the member offsets of qc_swing_tangent_io as the C compiler lays the header's struct out, against the ctypes mirror;
    qc_default_swing_tangent fills the record as documented and needs no device."""
    from quadruped_control_amd import tangent

    fields = [f for f, _ in tangent.QcSwingTangentIo._fields_]
    assert fields == list(IO_FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qc_tangent.h"\nint main(void) {\n  printf("%zu", sizeof(qc_swing_tangent_io));\n'
                   + "".join(f'  printf(" %zu", offsetof(qc_swing_tangent_io, {f}));\n' for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(tangent.QcSwingTangentIo) == 88
    assert got[1:] == [getattr(tangent.QcSwingTangentIo, f).offset for f in fields]
    io = tangent.QcSwingTangentIo()
    io.x_tan, io.flags, io.struct_size, io.n_dir = 123, 456, 7, 9
    tangent._library().qc_default_swing_tangent(ctypes.byref(io))
    assert io.struct_size == 88 and io.n_dir == 1
    assert all(getattr(io, f) is None for f in IO_FIELDS[2:])


def test_argument_check_needs_no_device(built):
    """qc_swing_torque_tangent_batch refuses a bad call before it touches the device - the handle is null, so every call below ends in
    the argument check."""
    from quadruped_control_amd import _lib, tangent

    lib = tangent._library()
    io = tangent.QcSwingTangentIo()
    lib.qc_default_swing_tangent(ctypes.byref(io))
    bi = _lib.QcBatchIn()
    for args in ((None, 1, ctypes.byref(bi), ctypes.byref(io), None), (None, 0, ctypes.byref(bi), None, None), (None, 1, None, ctypes.byref(io), None)):
        assert lib.qc_swing_torque_tangent_batch(*args) == -1 and _lib.last_error() == "qc_swing_torque_tangent_batch: null argument"


def test_host_logic_without_a_device():
    """check_swing_tangent_args through every refusal - a null handle, `in` or `io`, a wrong struct_size, n_dir == 0, no tangent, no
    output, swing_state, gait_dt, each of the six arrays missing, 4 n n_dir beyond one launch -, the default record, the kernel's
    arguments and the block count at and one past the cap (csrc/qc_host.hpp), in a stand-alone program built with the address and
    undefined-behaviour sanitizers (tests/cpp/swing_tangent_host_test.cpp)."""
    import __graft_entry__ as g

    assert "swing_tangent_host_test" in g.HOST_TESTS
    exe = g.build_host_test("swing_tangent_host_test")
    assert exe is not None and os.path.exists(exe)
    libs = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "amdhip64" not in libs and "qc_balance" not in libs, libs
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "swing tangent host logic ok" in r.stdout, r.stdout[-3000:]


def test_python_refusals_need_no_device(built):
    """What the three Python entry points refuse before anything is marshalled: unknown tangents, and what the rollouts through a trot
    have no forward mode for - with the words of their docstrings.  (The library's own messages reach Python from launch(): the GPU
    test holds those.)"""
    from quadruped_control_amd import tangent

    class Ctl:  # never reached
        device = 0

    t = object()
    with pytest.raises(ValueError, match="swing_torque_tangent: unknown tangent"):
        tangent.plan_swing_torque_tangent(Ctl(), {}, {"grf_tan": None})
    full = dict(joint_q=t, joint_qdot=t, swing_pos=t, swing_vel=t)
    for fn, extra in ((tangent.rollout_swing_tangent, ({},)), (tangent.rollout_swing_transition, ())):
        who = fn.__name__
        args = lambda batch: (Ctl(), batch, 1, 0.01, 0.02) + extra
        with pytest.raises(ValueError, match=f"{who}: batch\\['swing_state'\\] must be None"):
            fn(*args(dict(full, swing_state=t)))
        with pytest.raises(ValueError, match=f"{who}: batch\\['gait_dt'\\] must be None"):
            fn(*args(dict(full, gait_dt=t)))
        for one in ("swing_pos", "swing_vel"):
            with pytest.raises(ValueError, match=f"{who}: the batch carries swing_pos and swing_vel, both"):
                fn(*args({k: v for k, v in full.items() if k != one}))
        with pytest.raises(ValueError, match=f"{who}: the batch carries joint_q and joint_qdot"):
            fn(*args({k: v for k, v in full.items() if k != "joint_qdot"}))
    with pytest.raises(ValueError, match="rollout_swing_tangent: commander mode has no forward mode"):
        tangent.rollout_swing_tangent(Ctl(), full, 1, 0.01, 0.02, {}, command={})
    with pytest.raises(ValueError, match="rollout_swing_tangent: lean has no forward mode"):
        tangent.rollout_swing_tangent(Ctl(), full, 1, 0.01, 0.02, {}, lean={})
    assert tangent.SWING_FLAGS_SHIFT == 16 and set(tangent.ROLLOUT_SWING_TANGENTS) == set(tangent.ROLLOUT_TICK_TANGENTS) | {"swing_pos_tan", "swing_vel_tan"}
