"""CPU: the COM reference's forward mode (qc_com_reference_tangent_batch) - its float64 restatement against 50 digits (where C_MT is
measured), the pairing with the adjoint's restatement (C_MDOT), central differences of the forward map at the held mask, the
constructed cases, and the C ABI without a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import com_reference_restatement as CM
from tests import com_reference_tangent_restatement as MT
from tests import support_polygon_restatement as SP
from tests.device_math_reference import EPS

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
N, K, GAIN = 24, 3, 0.7
CASES = tuple((form, shared, mode) for form in ("feet", "joint_q") for shared in (False, True) for mode in CM.MODES)
bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)


def _case(form, shared, saturating=6):
    b, sched = SP.pool(N, saturating=saturating)
    b = {k: a for k, a in b.items() if k != ("joint_q" if form == "feet" else "feet")}
    return b, (sched[0] if shared else sched), MT.random_tangents(N, K, joint_q=form == "joint_q", shared=shared)


@pytest.mark.parametrize("form,shared,mode", CASES)
def test_restatement_against_50_digits_and_the_pairing(form, shared, mode):
    """C_MT and C_MDOT are measured HERE: the worst |float64 - 50 digits| / (EPS x condition sum) per output, and the worst gap of the
    pairing with reference_adjoint_np in EPS x the magnitudes of all terms - with a shared schedule_tan against the rows' sum."""
    b, sched, tans = _case(form, shared)
    val, flags = MT.tangent_np(b, sched, tans, mode, GAIN)
    ref, cond, _ = MT.tangent_mp(b, sched, tans, mode, GAIN)
    assert not flags.any()
    for name in MT.OUTPUTS:
        r = SP.worst_ratio(val[name], ref[name], cond[name])
        print(f"{form} shared={shared} {mode} {name}: worst |np - mp| / (EPS cond) = {r:.3f} (C_MT {MT.C_MT[name]})")
        assert r <= MT.C_MT[name], (name, r)
    bar = np.random.default_rng(5).uniform(-1, 1, (N, 3))
    adj, _ = CM.reference_adjoint_np(b, sched, bar, mode, GAIN)
    lhs, rhs, terms = MT.pairing(bar, val["x_d_out_tan"], tans, adj, b, shared_sum=adj["schedule_bar"].sum(axis=0) if shared else None)
    gap = float(np.max(np.abs(lhs - rhs) / (EPS * terms)))
    print(f"{form} shared={shared} {mode}: pairing gap {gap:.3f} EPS x terms (C_MDOT {MT.C_MDOT})")
    assert gap <= MT.C_MDOT


@pytest.mark.parametrize("form,shared,mode", CASES)
def test_central_differences_at_the_held_mask(form, shared, mode):
    """(f(+h) - f(-h)) / 2h of reference_np along each direction with the stance bytes of the unmoved batch.  The regular family only
    (widths >= 0.05: the map is smooth on the scale of h): h = 1e-6 leaves a truncation of h^2 |f'''| ~ 1e-12 / width^3 <= 1e-8 and a
    rounding of EPS / h ~ 2e-10; the bar 1e-6 on tangents of order 1e-2 stands above both and far below a wrong term."""
    b, sched, tans = _case(form, shared, saturating=0)
    x_d = np.random.default_rng(9).uniform(-1, 1, (N, 3))
    val, _ = MT.tangent_np(b, sched, tans, mode, GAIN)
    h = 1e-6
    for k in range(K):
        outs = [CM.reference_np(*MT.moved(b, sched, x_d, tans, k, s)[:2], MT.moved(b, sched, x_d, tans, k, s)[2], mode, GAIN)["x_d"] for s in (+h, -h)]
        fd = (outs[0] - outs[1]) / (2 * h)
        assert np.abs(fd - val["x_d_out_tan"][k]).max() < 1e-6, (k, np.abs(fd - val["x_d_out_tan"][k]).max())


def test_replace_copies_z_and_ignores_x_d_in_tan_in_x_and_y():
    b, sched, tans = _case("feet", False)
    val, _ = MT.tangent_np(b, sched, tans, "replace")
    assert np.array_equal(bits(val["x_d_out_tan"][..., 2]), bits(tans["x_d_in_tan"][..., 2]))
    other, _ = MT.tangent_np(b, sched, dict(tans, x_d_in_tan=tans["x_d_in_tan"] * [3.0, -2.0, 1.0]), "replace")
    assert np.array_equal(bits(other["x_d_out_tan"]), bits(val["x_d_out_tan"]))
    assert np.array_equal(bits(val["x_d_out_tan"][..., :2]), bits(val["com_xy_tan"]))


def test_offset_at_gain_zero_is_the_identity():
    b, sched, tans = _case("joint_q", False)
    val, _ = MT.tangent_np(b, sched, tans, "offset", 0.0)
    assert np.array_equal(bits(val["x_d_out_tan"]), bits(tans["x_d_in_tan"]))


def test_a_shared_schedule_tan_is_the_same_block_for_every_robot():
    b, sched, tans = _case("feet", True)
    val, _ = MT.tangent_np(b, sched, tans, "offset", GAIN)
    per_robot = dict(tans, schedule_tan=np.ascontiguousarray(np.broadcast_to(tans["schedule_tan"][:, None, :], (K, N, 16))))
    other, _ = MT.tangent_np(b, np.ascontiguousarray(np.broadcast_to(sched, (N, 4, 4))), per_robot, "offset", GAIN)
    for name in MT.OUTPUTS:
        assert np.array_equal(bits(val[name]), bits(other[name])), name


def test_a_zero_over_zero_robot_is_nan_and_flagged():
    """all four weights 0: every leg a swing leg deep in its swing with tiny widths - the reference's 0/0"""
    b, sched, tans = _case("feet", False, saturating=0)
    i = 5
    b = dict(b, stance=np.array([SP.contact_mask(b, r, SP.TROT_DUTY) for r in range(N)], np.uint8), gait_phase=b["gait_phase"].copy())
    sched = sched.copy()
    b["stance"][i], b["gait_phase"][i], sched[i] = 0, 0.5, 1e-3
    assert CM.reference_np(b, sched, np.zeros((N, 3)))["flags"][i] == 15
    for val, flags in (MT.tangent_np(b, sched, tans), (lambda r: (r[0], r[2]))(MT.tangent_mp(b, sched, tans))):
        assert flags[i] == 15 and not np.delete(flags, i).any()
        for name in MT.OUTPUTS:
            assert np.isnan(val[name][:, i]).all() and np.isfinite(np.delete(val[name], i, axis=1)).all(), name


# ------------------------------------------------------------------ the C ABI without a device
IO_FIELDS = ("struct_size", "schedule", "schedule_shared", "mode", "gain", "n_dir", "x_d_in_tan", "feet_tan", "joint_q_tan", "Rwb_rot_tan", "x_tan", "phase_tan",
             "schedule_tan", "x_d_out_tan", "com_xy_tan", "flags")


def test_symbols_are_exported_and_the_abi_stays(built):
    from quadruped_control_amd import _lib, tangent

    lib = ctypes.CDLL(os.path.join(ROOT, "quadruped_control_amd", "libqc_balance.so"))
    for name in ("qc_default_com_reference_tangent", "qc_com_reference_tangent_batch"):
        assert hasattr(lib, name), name
    assert _lib.load().qc_abi_version() == 6 and _lib.ABI_VERSION == 6
    assert tangent._library().qc_com_reference_tangent_batch.restype is ctypes.c_int
    assert ctypes.sizeof(_lib.QcComReferenceIo) == 64 and ctypes.sizeof(tangent.QcPlantTangentIo) == 160 and ctypes.sizeof(tangent.QcLegPlantTangentIo) == 248


def test_mirror_matches_the_header(built, tmp_path):
    from quadruped_control_amd import tangent

    fields = [f for f, _ in tangent.QcComReferenceTangentIo._fields_]
    assert fields == list(IO_FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qc_tangent.h"\nint main(void) {\n  printf("%zu", sizeof(qc_com_reference_tangent_io));\n'
                   + "".join(f'  printf(" %zu", offsetof(qc_com_reference_tangent_io, {f}));\n' for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(tangent.QcComReferenceTangentIo) == 120
    assert got[1:] == [getattr(tangent.QcComReferenceTangentIo, f).offset for f in fields]
    io = tangent.QcComReferenceTangentIo()
    io.x_tan, io.flags, io.schedule, io.struct_size, io.n_dir, io.mode, io.gain = 123, 456, 789, 7, 9, 1, 3.0
    tangent._library().qc_default_com_reference_tangent(ctypes.byref(io))
    assert io.struct_size == 120 and io.n_dir == 1 and io.mode == 0 and io.gain == 1.0 and io.schedule is None and io.schedule_shared == 0
    assert all(getattr(io, f) is None for f in IO_FIELDS[6:])


def test_argument_check_needs_no_device(built):
    from quadruped_control_amd import _lib, tangent

    lib = tangent._library()
    io, bi = tangent.QcComReferenceTangentIo(), _lib.QcBatchIn()
    lib.qc_default_com_reference_tangent(ctypes.byref(io))
    for args in ((None, 1, ctypes.byref(bi), ctypes.byref(io), None), (None, 0, ctypes.byref(bi), None, None), (None, 1, None, ctypes.byref(io), None)):
        assert lib.qc_com_reference_tangent_batch(*args) == -1 and _lib.last_error() == "qc_com_reference_tangent_batch: null argument"


def test_host_logic_without_a_device():
    """check_com_reference_tangent_args through every refusal and the kernel's arguments, in a stand-alone program built with the
    address and undefined-behaviour sanitizers (tests/cpp/com_reference_tangent_host_test.cpp)."""
    import __graft_entry__ as g

    assert "com_reference_tangent_host_test" in g.HOST_TESTS
    exe = g.build_host_test("com_reference_tangent_host_test")
    assert exe is not None and os.path.exists(exe)
    libs = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "amdhip64" not in libs and "qc_balance" not in libs, libs
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "com reference tangent host logic ok" in r.stdout, r.stdout[-3000:]


def test_python_refusals_need_no_device(built):
    """What the new entry point refuses before anything is marshalled, and rollout_gait_tangent()'s refusal of `lean`, kept in its words."""
    from quadruped_control_amd import tangent

    class Ctl:  # never reached
        device = 0

    t = object()
    with pytest.raises(ValueError, match="com_reference_tangent: mode is one of"):
        tangent.plan_com_reference_tangent(Ctl(), {}, None, None, {}, mode="lean")
    with pytest.raises(ValueError, match="com_reference_tangent: unknown tangent"):
        tangent.plan_com_reference_tangent(Ctl(), {}, None, None, {"x_d_tan": None})
    assert tuple(tangent.COM_REFERENCE_TANGENTS) == IO_FIELDS[6:13]
    full = dict(joint_q=t, joint_qdot=t, gait_phase=t, swing_state=t)
    with pytest.raises(ValueError, match="rollout_gait_tangent: lean has no forward mode - lean must be None \\(the com reference has no forward mode\\)"):
        tangent.rollout_gait_tangent(Ctl(), full, 1, 0.01, 0.02, 0.01, {}, lean={})
    assert set(tangent.ROLLOUT_GAIT_TANGENTS) == set(tangent.ROLLOUT_TICK_TANGENTS) | {"p_start_tan", "p_final_tan"}
