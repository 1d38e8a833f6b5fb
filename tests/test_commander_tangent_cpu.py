"""CPU: the commander step's forward mode (qc_commander_step_tangent_batch) - its float64 restatement against 50 digits (where C_CT
is measured), the pairing with the adjoint's restatement (C_CDOT), central differences of the forward step at held decisions, the
constructed cases, and the C ABI without a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import commander_adjoint_restatement as CA
from tests import commander_tangent_restatement as CT
from tests.device_math_reference import EPS
from tests.swing_reference_restatement import worst_ratio

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
N, K = 257, 3
bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def case():
    st, Rwb, x, twist, fresh, kinds = CA.pool(N)
    tans = CT.random_tangents(N, K)
    val, flags = CT.tangent_np(st, Rwb, x, twist, fresh, tans)
    applied = np.array([CA.decide(st[i], x[i, 2], bool(fresh[i]), CA.SCALARS["stand_height"], CA.SCALARS["stand_tol"])[2] for i in range(N)])
    assert not flags.any() and set(kinds) == set(CA.KINDS) and applied.any() and (~applied).any()
    return dict(st=st, Rwb=Rwb, x=x, twist=twist, fresh=fresh, kinds=kinds, tans=tans, val=val, applied=applied)


def test_restatement_against_50_digits_on_the_pool(case):
    """C_CT is measured HERE: the worst |float64 - 50 digits| / (EPS x condition sum) per output over the pool of every KINDS kind."""
    c = case
    ref, cond, flags = CT.tangent_mp(c["st"], c["Rwb"], c["x"], c["twist"], c["fresh"], c["tans"])
    assert not flags.any()
    for name in CT.OUTPUTS:
        r = worst_ratio(c["val"][name], ref[name], cond[name])
        print(f"{name}: worst |np - mp| / (EPS cond) = {r:.3f} (C_CT {CT.C_CT[name]})")
        assert r <= CT.C_CT[name], (name, r)


def test_pairing_with_the_adjoint_restatement(case):
    """C_CDOT is measured HERE, in EPS x the magnitudes of all terms: the issue's pairing, with the smooth function's Rwb_d below the
    forward pass's small-angle threshold (commander_tangent_restatement.smooth_Rwb_d says why)."""
    c = case
    bars = CA.cotangents(N)
    adj, _ = CA.adjoint_np(c["st"], c["Rwb"], c["x"], c["twist"], c["fresh"], bars)
    _, out = CA.step_np(c["st"], c["Rwb"], c["x"], c["twist"], c["fresh"])
    Rd = CT.smooth_Rwb_d(out["Rwb_d"], c["st"], c["x"], c["twist"], c["fresh"])
    lhs, rhs, terms = CT.pairing(bars, c["val"], c["tans"], adj, c["Rwb"], Rd, c["st"]["Rwb_d"])
    gap = float(np.max(np.abs(lhs - rhs) / (EPS * terms)))
    print(f"pairing: worst gap {gap:.3f} EPS x terms (C_CDOT {CT.C_CDOT})")
    assert gap <= CT.C_CDOT and (terms > 0).all()


def test_central_differences_at_held_decisions(case):
    """(f(+h) - f(-h)) / 2h of the forward step along each direction, every input moved (the rotations along their left tangents), the
    latches unchanged at both points.  h = 1e-5: the truncation is h^2 |f'''| ~ 1e-10 of values of order 1, the rounding EPS / h ~ 2e-11;
    the bar 1e-8 (absolute, on tangents of order 0.1) stands far above both and far below a wrong term.  The `below` kind is left out
    of the entries that depend on om: at |d| = 0.5e-12 the forward pass's Rb = I branch differs from Exp(d) by |d|, which the quotient
    turns into 1e-12 / 2h = 5e-8 - the tangent is the smooth function's there, and the pairing holds those robots."""
    c = case
    h = 1e-5
    keep = np.array([k != "below" for k in c["kinds"]])
    for k in range(K):
        outs = []
        for s in (+h, -h):
            st, Rwb, x, twist = CT.moved(c["st"], c["Rwb"], c["x"], c["twist"], c["tans"], k, s)
            new, out = CA.step_np(st, Rwb, x, twist, c["fresh"])
            assert np.array_equal(out["applied"].astype(bool), c["applied"])
            outs.append((new, out))
        (np_, op), (nm, om) = outs
        for name in ("x_d", "xdot_d", "w_d"):
            fd = (op[name] - om[name]) / (2 * h)
            assert np.abs(fd - c["val"][name + "_tan"][k])[keep].max() < 1e-8, name
        fd = (np_["Vb"] - nm["Vb"]) / (2 * h)
        assert np.abs(fd - c["val"]["Vb_next_tan"][k]).max() < 1e-8
        # the rotation: log(Rwb_d(+h) Rwb_d(-h)^T) / 2h is the left tangent
        for i in np.flatnonzero(keep):
            E = op["Rwb_d"][i].reshape(3, 3) @ om["Rwb_d"][i].reshape(3, 3).T
            fd = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]]) / (4 * h)
            assert np.abs(fd - c["val"]["Rwb_d_rot_tan"][k, i]).max() < 1e-8, (i, c["kinds"][i])


def test_a_robot_that_applies_nothing_passes_the_record_through(case):
    c = case
    idle = ~c["applied"]
    for out, prev in CT.PREV_OF.items():
        assert np.array_equal(bits(c["val"][out][:, idle]), bits(c["tans"][prev][:, idle])), out
        assert not np.array_equal(c["val"][out][:, c["applied"]], c["tans"][prev][:, c["applied"]])


def test_fresh_against_held_routes_the_command_tangent(case):
    c = case
    f = c["fresh"].astype(bool)
    assert np.array_equal(bits(c["val"]["Vb_next_tan"][:, f]), bits(c["tans"]["twist_tan"][:, f]))
    assert np.array_equal(bits(c["val"]["Vb_next_tan"][:, ~f]), bits(c["tans"]["Vb_tan"][:, ~f]))
    # the other one reaches nothing
    swapped = dict(c["tans"], twist_tan=np.where(f[None, :, None], c["tans"]["twist_tan"], 7.0), Vb_tan=np.where(f[None, :, None], 7.0, c["tans"]["Vb_tan"]))
    other, _ = CT.tangent_np(c["st"], c["Rwb"], c["x"], c["twist"], c["fresh"], swapped)
    for name in CT.OUTPUTS:
        assert np.array_equal(bits(other[name]), bits(c["val"][name])), name


def test_zero_rate_gives_a_nonzero_rotation_tangent_for_a_yaw_rate_seed(case):
    c = case
    om0 = np.array([k == "om0" for k in c["kinds"]]) & c["applied"]
    assert om0.any()
    seed = {k: None for k in CT.TANGENTS}
    seed["twist_tan"] = np.zeros((1, N, 6))
    seed["twist_tan"][0, :, 5] = 1.0
    val, _ = CT.tangent_np(c["st"], c["Rwb"], c["x"], c["twist"], c["fresh"], seed)
    # Jl(0) = I: Rwb_d_rot_tan = Y cmd_dt e_z = cmd_dt e_z
    assert np.allclose(val["Rwb_d_rot_tan"][0, om0], [0.0, 0.0, CA.SCALARS["cmd_dt"]], rtol=0, atol=1e-18)
    assert (val["w_d_tan"][0, om0] != 0).any()


def test_the_height_has_no_tangent_when_applied(case):
    c = case
    assert not bits(c["val"]["x_d_tan"][:, c["applied"], 2]).any()


def test_gimbal_lock_is_nan_in_every_direction_and_the_neighbours_are_clean(case):
    c = case
    Rwb = c["Rwb"].copy()
    i = int(np.flatnonzero(c["applied"])[3])
    Rwb[i] = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]]).reshape(9)  # pitch = -pi / 2: R00 = R10 = 0
    for val, flags in (CT.tangent_np(c["st"], Rwb, c["x"], c["twist"], c["fresh"], c["tans"]),
                       (lambda r: (r[0], r[2]))(CT.tangent_mp(c["st"][:i + 2], Rwb[:i + 2], c["x"][:i + 2], c["twist"][:i + 2], c["fresh"][:i + 2],
                                                              {k: v[:, :i + 2] for k, v in c["tans"].items()}))):
        assert flags[i] == 1 and flags.sum() == 1
        for name in CT.OUTPUTS:
            assert np.isnan(val[name][:, i]).all() and np.isfinite(np.delete(val[name], i, axis=1)).all(), name


# ------------------------------------------------------------------ the C ABI without a device
IO_FIELDS = ("struct_size", "state_before", "n_dir", "twist_tan", "Vb_tan", "Rwb_rot_tan", "x_tan", "Rwb_d_rot_prev_tan", "x_d_prev_tan", "xdot_d_prev_tan",
             "w_d_prev_tan", "Rwb_d_rot_tan", "x_d_tan", "xdot_d_tan", "w_d_tan", "Vb_next_tan", "flags")


def test_symbols_are_exported_and_the_abi_stays(built):
    from quadruped_control_amd import _lib, tangent

    lib = ctypes.CDLL(os.path.join(ROOT, "quadruped_control_amd", "libqc_balance.so"))
    for name in ("qc_default_commander_step_tangent", "qc_commander_step_tangent_batch"):
        assert hasattr(lib, name), name
    assert _lib.load().qc_abi_version() == 6 and _lib.ABI_VERSION == 6
    assert tangent._library().qc_commander_step_tangent_batch.restype is ctypes.c_int
    assert ctypes.sizeof(tangent.QcSwingTangentIo) == 88 and ctypes.sizeof(tangent.QcTorqueTangentIo) == 56 and ctypes.sizeof(tangent.QcTangentIo) == 136 and \
        ctypes.sizeof(tangent.QcSwingReferenceTangentIo) == 128


def test_mirror_matches_the_header(built, tmp_path):
    from quadruped_control_amd import tangent

    fields = [f for f, _ in tangent.QcCommanderStepTangentIo._fields_]
    assert fields == list(IO_FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qc_tangent.h"\nint main(void) {\n  printf("%zu", sizeof(qc_commander_step_tangent_io));\n'
                   + "".join(f'  printf(" %zu", offsetof(qc_commander_step_tangent_io, {f}));\n' for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(tangent.QcCommanderStepTangentIo) == 8 * len(IO_FIELDS)
    assert got[1:] == [getattr(tangent.QcCommanderStepTangentIo, f).offset for f in fields]
    io = tangent.QcCommanderStepTangentIo()
    io.x_tan, io.flags, io.state_before, io.struct_size, io.n_dir = 123, 456, 789, 7, 9
    tangent._library().qc_default_commander_step_tangent(ctypes.byref(io))
    assert io.struct_size == 8 * len(IO_FIELDS) and io.n_dir == 1 and io.state_before is None and all(getattr(io, f) is None for f in IO_FIELDS[3:])


def test_argument_check_needs_no_device(built):
    from quadruped_control_amd import _lib, tangent

    lib = tangent._library()
    io, bi, c = tangent.QcCommanderStepTangentIo(), _lib.QcBatchIn(), _lib.QcCommandIn()
    lib.qc_default_commander_step_tangent(ctypes.byref(io))
    lib.qc_default_command(ctypes.byref(c))
    for args in ((None, 1, ctypes.byref(bi), ctypes.byref(c), ctypes.byref(io), None), (None, 0, ctypes.byref(bi), ctypes.byref(c), None, None),
                 (None, 1, None, ctypes.byref(c), ctypes.byref(io), None), (None, 1, ctypes.byref(bi), None, ctypes.byref(io), None)):
        assert lib.qc_commander_step_tangent_batch(*args) == -1 and _lib.last_error() == "qc_commander_step_tangent_batch: null argument"


def test_host_logic_without_a_device():
    """check_commander_step_tangent_args through every refusal, the kernel's arguments and the block count at and one past the cap, in
    a stand-alone program built with the address and undefined-behaviour sanitizers (tests/cpp/commander_step_tangent_host_test.cpp)."""
    import __graft_entry__ as g

    assert "commander_step_tangent_host_test" in g.HOST_TESTS
    exe = g.build_host_test("commander_step_tangent_host_test")
    assert exe is not None and os.path.exists(exe)
    libs = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "amdhip64" not in libs and "qc_balance" not in libs, libs
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "commander step tangent host logic ok" in r.stdout, r.stdout[-3000:]


def test_python_refusals_need_no_device(built):
    """What the new entry point refuses before anything is marshalled, and the rollouts' refusals of `command` and `lean`, kept in
    their words."""
    from quadruped_control_amd import tangent

    class Ctl:  # never reached
        device = 0

    t = object()
    with pytest.raises(ValueError, match="commander_step_tangent: unknown tangent"):
        tangent.plan_commander_step_tangent(Ctl(), {}, {}, None, {"x_d_tan": None})
    assert tuple(tangent.COMMANDER_STEP_TANGENTS) == IO_FIELDS[3:11] and tangent.COMMANDER_STEP_TANGENT_WANT == IO_FIELDS[11:16]
    with pytest.raises(ValueError, match="rollout_tick_tangent: commander mode has no forward mode - command must be None"):
        tangent.rollout_tick_tangent(Ctl(), dict(joint_q=t, joint_qdot=t), 1, 0.01, 0.02, {}, command={})
    with pytest.raises(ValueError, match="rollout_swing_tangent: commander mode has no forward mode - command must be None"):
        tangent.rollout_swing_tangent(Ctl(), dict(joint_q=t, joint_qdot=t, swing_pos=t, swing_vel=t), 1, 0.01, 0.02, {}, command={})
    with pytest.raises(ValueError, match="rollout_tick_tangent: lean has no forward mode - lean must be None"):
        tangent.rollout_tick_tangent(Ctl(), dict(joint_q=t, joint_qdot=t), 1, 0.01, 0.02, {}, lean={})
