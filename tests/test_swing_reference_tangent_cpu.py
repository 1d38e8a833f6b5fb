"""CPU: the swing references' forward mode restated (tests/swing_reference_tangent_restatement.py) - its float64 evaluation against its
50-digit one (C_RT, per output), the pairing with the adjoint's restatement in both arithmetics (C_RDOT), central differences of the
restated forward call at held decisions, constructed cases (zero rows, pass-through rows, dpf_z, the flag bits) - and the C ABI of
qc_swing_reference_tangent_batch as far as it goes without a device: the exports, the ctypes mirror against the header, the sanitized
host program, the Python refusals.

Measured (committed seeds): the 50-digit tests print the worst distances; RT.C_RT and RT.C_RDOT hold them rounded up."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import swing_reference_restatement as RR
from tests import swing_reference_tangent_restatement as RT

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EPS = 2.0 ** -52
K_CPU = 3


def _case(M):
    b, before, after, planned, kinds = RT.pool_after(M)
    n = b["x"].shape[0]
    tans = RT.random_tangents(n, K_CPU)
    val, flags = RT.reference_tangent_np(M, b, before, tans)
    ref, cond, flags_mp = RT.reference_tangent_mp(M, b, before, tans)
    return dict(M=M, b=b, before=before, after=after, planned=planned, kinds=kinds, n=n, tans=tans, val=val, flags=flags, ref=ref, cond=cond, flags_mp=flags_mp)


@pytest.fixture(scope="module")
def cases():
    class Lazy(dict):  # (a model's 50-digit pass is built when a test first asks for it)
        def __missing__(self, model):
            self[model] = _case(RR.MODELS[model])
            return self[model]

    return Lazy()


@pytest.mark.parametrize("model", ("default", "odd"))
def test_float64_against_50_digits(cases, model):
    """C_RT: the float64 restatement against the 50-digit pass on the whole pool, per output and entry in EPS x condition sum - printed,
    asserted below the recorded figure.  Entries with condition sum 0 (rows of legs that do not track, dpf_z of a replanned leg) are
    exact."""
    c = cases[model]
    assert not c["flags"].any() and not c["flags_mp"].any()
    assert set(c["kinds"]) == set(RR.KINDS)
    worst = {k: RR.worst_ratio(c["val"][k], c["ref"][k], c["cond"][k]) for k in RT.OUTPUTS}
    print(f"C_RT[{model}]: " + ", ".join(f"{k} {v:.4f} (recorded {RT.C_RT[k]})" for k, v in worst.items()))
    for k, v in worst.items():
        assert 0.0 < v <= RT.C_RT[k], (k, v)


@pytest.mark.parametrize("model", ("default", "odd"))
def test_pairing_with_the_adjoint(cases, model):
    """<cotangents, the tangent's outputs> against <reference_adjoint's outputs, the tangents> on the whole pool.  Float64 with
    reference_adjoint_np: C_RDOT, in EPS x the sum of the magnitudes of all terms on both sides - printed, asserted below the recorded
    figure.  50 digits with reference_adjoint_mp: both passes hand over values rounded to double once, and the products are summed at
    50 digits, so the two sides agree to (1 + EPS / 4) EPS x the magnitudes - the bar is 1.01 EPS."""
    c = cases[model]
    M, b, n = c["M"], c["b"], c["n"]
    bars = RR.cotangents(n)
    adj, flags = RR.reference_adjoint_np(M, b, c["before"], bars)
    assert not flags.any()
    lhs, rhs, terms = RT.pairing(bars, c["val"], c["tans"], adj, b["Rwb"])
    assert (terms > 0).all()
    worst = float(np.max(np.abs(lhs - rhs) / (EPS * terms)))
    print(f"C_RDOT[{model}]: {worst:.4f} (recorded {RT.C_RDOT})")
    assert worst <= RT.C_RDOT, worst
    adj_mp, _, _ = RR.reference_adjoint_mp(M, b, c["before"], bars)
    lhs, rhs, terms = RT.pairing(bars, c["ref"], c["tans"], adj_mp, b["Rwb"], exact=True)
    gap = max(float(abs(l - r)) / (EPS * t) for l, r, t in zip(lhs.ravel(), rhs.ravel(), terms.ravel()))
    print(f"50-digit pairing[{model}]: {gap:.4f} EPS x magnitudes")
    assert gap <= 1.01, gap


FD_H = 1e-4


@pytest.mark.parametrize("model", ("default", "odd"))
def test_central_differences_at_held_decisions(model):
    """The tangent against central differences of reference_np - the restated FORWARD call, no clock: the phases, and so the mask and
    the decisions, are held - along three committed directions that move the state and the record at once.  The pool keeps x_z in
    [0.2, 0.35] and every swing phase 5 % inside the clamp's open interval, where the map is smooth: no entry is excluded.  The bar per
    entry is the truncation estimated from the differences alone, |FD(h) - FD(2h)| (three times the truncation of FD(h)), plus
    1e-9 + 1e-8 |tangent| for the rounding of the quotient: EPS x |value| / h = 2e-12 x |value|, values up to 5 (swing_vel)."""
    M = RR.MODELS[model]
    n = 61
    b, before, _, planned, kinds = RT.pool_after(M, n)
    tans = RT.random_tangents(n, 3, seed=73)
    val, flags = RT.reference_tangent_np(M, b, before, tans)
    assert not flags.any() and planned.any() and set(kinds) == set(RR.KINDS)
    names = {"swing_pos_tan": "swing_pos", "swing_vel_tan": "swing_vel", "p_start_next_tan": "p_start", "p_final_next_tan": "p_final"}
    for k in range(3):
        pts = {}
        for m in (-2, -1, 1, 2):
            bm, rec = RT.moved(b, before, tans, k, m * FD_H)
            out, after, phases, pl = RR.reference_np(M, bm, rec)
            assert np.array_equal(pl, planned) and np.array_equal(phases, b["gait_phase"])
            pts[m] = out
        for name, fwd in names.items():
            fd1, fd2 = (pts[1][fwd] - pts[-1][fwd]) / (2 * FD_H), (pts[2][fwd] - pts[-2][fwd]) / (4 * FD_H)
            err, bar = np.abs(fd1 - val[name][k]), np.abs(fd1 - fd2) + 1e-8 * np.abs(val[name][k]) + 1e-9
            print(f"{model} direction {k} {name}: worst error / bar {np.max(err / bar):.3f}, worst error {err.max():.2e}")
            assert (err <= bar).all(), (name, k)


def test_constructed_cases(cases):
    """What the held decisions do to the rows, bit for bit, in both arithmetics: a stance leg and a swing leg without a trajectory give
    zero rows; a leg that is not replanned passes its record's tangents through; dpf_z of a replanned leg is exactly 0; a replanned
    leg's rows do not depend on the record's tangents."""
    c = cases["default"]
    b, before, after, planned, n = c["b"], c["before"], c["after"], c["planned"], c["n"]
    stance = after["leg_state"] == 1
    tracks = ~stance & (after["has_traj"] == 1)
    plan = ((planned[:, None] >> np.arange(4)) & 1).astype(bool)
    untracked_swing = ~stance & ~tracks
    assert stance.any() and tracks.any() and untracked_swing.any() and plan.any() and (~plan & tracks).any()
    rows = lambda a: a.reshape(K_CPU, n, 4, 3)
    bits = lambda a: np.ascontiguousarray(a).view(np.int64)
    for out in (c["val"], c["ref"]):
        for name in ("swing_pos_tan", "swing_vel_tan"):
            assert not bits(rows(out[name])[:, ~tracks]).any(), name  # +0.0 exactly
            assert (rows(out[name])[:, tracks] != 0.0).any(axis=-1).all(), name
        for name, tan in (("p_start_next_tan", "p_start_tan"), ("p_final_next_tan", "p_final_tan")):
            assert np.array_equal(bits(rows(out[name])[:, ~plan]), bits(rows(c["tans"][tan])[:, ~plan])), name
            assert (rows(out[name])[:, plan] != rows(c["tans"][tan])[:, plan]).any(axis=-1).all(), name
        assert not bits(rows(out["p_final_next_tan"])[:, plan][..., 2]).any()
        assert (rows(out["p_final_next_tan"])[:, plan][..., :2] != 0.0).all() and (rows(out["p_start_next_tan"])[:, plan] != 0.0).all()
    other = RT.reference_tangent_np(c["M"], b, before, dict(c["tans"], p_start_tan=None, p_final_tan=None))[0]
    for name in RT.OUTPUTS:
        replanned_rows = plan if name.startswith("p_") else (plan & tracks)
        assert np.array_equal(bits(rows(other[name])[:, replanned_rows]), bits(rows(c["val"][name])[:, replanned_rows])), name


@pytest.mark.parametrize("x_z", (0.0, -0.3, float("nan"), float("inf"), float("-inf")))
def test_flags_for_a_replanned_leg_only(x_z):
    """flags on x_z <= 0, NaN and inf: bit l for every REPLANNED leg l, every row of that robot NaN in every direction - and no bit, and
    finite rows, for a robot at the same x_z that replans nothing (carried, cleared, stance).  Both arithmetics."""
    M = RR.DEFAULT_MODEL
    n = 12
    b, before, _, planned, kinds = RT.pool_after(M, n)
    b = dict(b, x=b["x"].copy())
    b["x"][:, 2] = x_z
    tans = RT.random_tangents(n, 2, seed=79)
    assert (planned != 0).any() and (planned == 0).any()
    for val, flags in (RT.reference_tangent_np(M, b, before, tans), (lambda r: (r[0], r[2]))(RT.reference_tangent_mp(M, b, before, tans))):
        assert np.array_equal(flags, planned.astype(np.int32)), (flags, planned)
        for name in RT.OUTPUTS:
            assert np.isnan(val[name][:, planned != 0]).all() and np.isfinite(val[name][:, planned == 0]).all(), name
    # a healthy x_z: no bit anywhere
    ok = dict(b, x=np.c_[b["x"][:, :2], np.full(n, 0.3)])
    assert not RT.reference_tangent_np(M, ok, before, tans)[1].any()


# ------------------------------------------------------------------ the C ABI without a device
IO_FIELDS = ("struct_size", "state_before", "n_dir", "Rwb_rot_tan", "x_tan", "xdot_tan", "w_tan", "xdot_d_tan", "joint_q_tan", "p_start_tan", "p_final_tan",
             "swing_pos_tan", "swing_vel_tan", "p_start_next_tan", "p_final_next_tan", "flags")


def test_symbols_are_exported_and_the_abi_stays(built):
    from quadruped_control_amd import _lib, tangent

    lib = ctypes.CDLL(os.path.join(ROOT, "quadruped_control_amd", "libqc_balance.so"))
    for name in ("qc_default_swing_reference_tangent", "qc_swing_reference_tangent_batch"):
        assert hasattr(lib, name), name
    assert _lib.load().qc_abi_version() == 6 and _lib.ABI_VERSION == 6  # new entry points, no change to what existed
    bound = tangent._library()
    assert bound.qc_swing_reference_tangent_batch.restype is ctypes.c_int
    assert ctypes.sizeof(tangent.QcSwingTangentIo) == 88 and ctypes.sizeof(tangent.QcTorqueTangentIo) == 56 and ctypes.sizeof(tangent.QcTangentIo) == 136


def test_mirror_matches_the_header(built, tmp_path):
    """sizeof and the member offsets of qc_swing_reference_tangent_io as the C compiler lays the header's struct out, against the ctypes
    mirror; qc_default_swing_reference_tangent fills the record as documented and needs no device."""
    from quadruped_control_amd import tangent

    fields = [f for f, _ in tangent.QcSwingReferenceTangentIo._fields_]
    assert fields == list(IO_FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qc_tangent.h"\nint main(void) {\n  printf("%zu", sizeof(qc_swing_reference_tangent_io));\n'
                   + "".join(f'  printf(" %zu", offsetof(qc_swing_reference_tangent_io, {f}));\n' for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(tangent.QcSwingReferenceTangentIo) == 128
    assert got[1:] == [getattr(tangent.QcSwingReferenceTangentIo, f).offset for f in fields]
    io = tangent.QcSwingReferenceTangentIo()
    io.x_tan, io.flags, io.state_before, io.struct_size, io.n_dir = 123, 456, 789, 7, 9
    tangent._library().qc_default_swing_reference_tangent(ctypes.byref(io))
    assert io.struct_size == 128 and io.n_dir == 1 and io.state_before is None
    assert all(getattr(io, f) is None for f in IO_FIELDS[3:])


def test_argument_check_needs_no_device(built):
    """qc_swing_reference_tangent_batch refuses a bad call before it touches the device - the handle is null, so every call below ends
    in the argument check."""
    from quadruped_control_amd import _lib, tangent

    lib = tangent._library()
    io = tangent.QcSwingReferenceTangentIo()
    lib.qc_default_swing_reference_tangent(ctypes.byref(io))
    bi = _lib.QcBatchIn()
    for args in ((None, 1, ctypes.byref(bi), ctypes.byref(io), None), (None, 0, ctypes.byref(bi), None, None), (None, 1, None, ctypes.byref(io), None)):
        assert lib.qc_swing_reference_tangent_batch(*args) == -1 and _lib.last_error() == "qc_swing_reference_tangent_batch: null argument"


def test_host_logic_without_a_device():
    """check_swing_reference_tangent_args through every refusal - a null handle, `in` or `io`, a wrong struct_size, n_dir == 0, no
    tangent, no output, gait_dt, swing_pos, swing_vel, feet without joint_q, a missing state_before, each of the six arrays missing,
    n n_dir beyond one launch -, the default record, the kernel's arguments and the block count at and one past the cap
    (csrc/qc_host.hpp), in a stand-alone program built with the address and undefined-behaviour sanitizers
    (tests/cpp/swing_reference_tangent_host_test.cpp)."""
    import __graft_entry__ as g

    assert "swing_reference_tangent_host_test" in g.HOST_TESTS
    exe = g.build_host_test("swing_reference_tangent_host_test")
    assert exe is not None and os.path.exists(exe)
    libs = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "amdhip64" not in libs and "qc_balance" not in libs, libs
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "swing reference tangent host logic ok" in r.stdout, r.stdout[-3000:]


def test_python_refusals_need_no_device(built):
    """What the Python entry points refuse before anything is marshalled: unknown tangents, and what the rollouts through the planner
    refuse - with the words of their docstrings.  The entry points that were there keep their refusals.  (The library's own messages
    reach Python from launch(): the GPU test holds those.)"""
    from quadruped_control_amd import tangent

    class Ctl:  # never reached
        device = 0

    t = object()
    with pytest.raises(ValueError, match="swing_reference_tangent: unknown tangent"):
        tangent.plan_swing_reference_tangent(Ctl(), {}, None, {"swing_pos_tan": None})
    full = dict(joint_q=t, joint_qdot=t, gait_phase=t, swing_state=t)
    for fn, extra in ((tangent.rollout_gait_tangent, ({},)), (tangent.rollout_gait_transition, ())):
        who = fn.__name__
        args = lambda batch: (Ctl(), batch, 1, 0.01, 0.02, 0.01) + extra
        for name in ("stance", "swing_pos", "swing_vel", "gait_dt", "feet"):
            with pytest.raises(ValueError, match=f"{who}: batch\\['{name}'\\] must be None"):
                fn(*args(dict(full, **{name: t})))
        for name in full:
            with pytest.raises(ValueError, match=f"{who}: the batch carries joint_q, joint_qdot, gait_phase and swing_state - missing \\['{name}'\\]"):
                fn(*args({k: v for k, v in full.items() if k != name}))
    with pytest.raises(ValueError, match="rollout_gait_tangent: lean has no forward mode - lean must be None \\(the com reference has no forward mode\\)"):
        tangent.rollout_gait_tangent(Ctl(), full, 1, 0.01, 0.02, 0.01, {}, lean={})
    with pytest.raises(ValueError, match="rollout_gait_tangent: unknown tangent"):
        tangent.rollout_gait_tangent(Ctl(), full, 1, 0.01, 0.02, 0.01, {"swing_pos_tan": t})  # (the references' tangents are computed, not taken)
    assert tangent.REFERENCE_FLAGS_SHIFT == 20 and set(tangent.ROLLOUT_GAIT_TANGENTS) == set(tangent.ROLLOUT_TICK_TANGENTS) | {"p_start_tan", "p_final_tan"}
    assert tangent.GAIT_TRANSITION_COLUMNS[:36] == tangent.TICK_TRANSITION_COLUMNS and len(tangent.GAIT_TRANSITION_COLUMNS) == 60
    assert tangent.GAIT_TRANSITION_COLUMNS[36] == ("p_start", 0) and tangent.GAIT_TRANSITION_COLUMNS[48] == ("p_final", 0)
    # the entry points that were there refuse what they refused, in their words
    swings = dict(joint_q=t, joint_qdot=t, swing_pos=t, swing_vel=t)
    with pytest.raises(ValueError, match="rollout_swing_tangent: batch\\['swing_state'\\] must be None - the swing planner has no forward mode"):
        tangent.rollout_swing_tangent(Ctl(), dict(swings, swing_state=t), 1, 0.01, 0.02, {})
    with pytest.raises(ValueError, match="rollout_tick_tangent: batch\\['gait_dt'\\] must be None - the gait clock \\(the contact mask is held\\) has no forward mode"):
        tangent.rollout_tick_tangent(Ctl(), dict(joint_q=t, joint_qdot=t, gait_dt=t), 1, 0.01, 0.02, {})
