"""CPU: the forward mode around the tick restated in numpy (tests/leg_plant_tangent_restatement.py) against its own 50-digit variants,
against the EXISTING reverse-pass restatements (the dot-product identities with leg_plant_adjoint_np and kin_cotangents), against
central differences of leg_plant_step_np and of the oracle's torque map, and on the flagged pool; and the C ABI of
qc_torque_tangent_batch and qc_leg_plant_step_tangent_batch as far as it goes without a device.

Measured here and asserted not to exceed what tests/leg_plant_tangent_restatement.py records (C_LT, C_TT, C_LDOT, C_TDOT); the numbers
are in that module's comments and in profiles/leg_plant_tangent.md.  tests/test_gpu_leg_plant_tangent.py holds the device to 4 x each."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import quadruped_control_amd as q
from tests import leg_plant_adjoint_restatement as LA
from tests import leg_plant_restatement as LR
from tests import leg_plant_tangent_restatement as LT
from tests import sensitivity_kinematics_restatement as SK

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EPS = LT.EPS
TORQUE_N = 65  # the robots of the torque map's 50-digit and dot-product cases (the central differences take LA.FD_N)


@pytest.fixture(scope="module")
def P(built):
    return q.cheetah_params()


def _np(P, s, mask, tans, kin=LT.DEFAULT_KIN):
    return LT.leg_plant_tangent_np(P["mass"], P["Ib"], *(s[k] for k in LT.INPUTS), mask, LT.INERTIA, LT.DT, tans, kin=kin)


def _limits(kin_name):
    return (SK.TAU_MIN, SK.TAU_MAX) if kin_name == "default" else (SK.ODD_TAU_MIN, SK.ODD_TAU_MAX)


def test_leg_plant_restatement_against_50_digits_on_the_pool(P):
    """leg_plant_tangent_np against leg_plant_tangent_mp (the IK's atan2 chain differentiated as written) on the adjoint's pool - 257
    robots, every contact mask - at both kinematic models, every output entry, in units of EPS x condition sum: c_lt.  An entry whose
    condition sum is 0 is exact."""
    worst = {k: 0.0 for k in LT.OUTPUTS}
    for name in LT.KINS:
        kin = LT.kin_of(name)
        s, mask, _ = LA.pool(kin)
        ref = LT.pool_reference(name)
        got = _np(P, s, mask, LT.pool_tangents(), kin)
        assert not got["flags"].any()
        for k in LT.OUTPUTS:
            val, cond = ref[k]
            assert np.allclose(got[k][1], cond, rtol=1e-9, atol=0), k  # (the two condition sums are one expression)
            zero = cond == 0
            assert np.array_equal(got[k][0][zero], val[zero]), k
            worst[k] = max(worst[k], float((np.abs(got[k][0] - val)[~zero] / (EPS * cond[~zero])).max()))
    print("c_lt", worst)
    for k in LT.OUTPUTS:
        assert worst[k] <= LT.C_LT[k], (k, worst[k])


def _torque_cases():
    for name in LT.KINS:
        for source in ("stance", "phase"):
            b, grf, status, cot = SK.case(TORQUE_N, source)
            yield name, source, b, grf, status, cot, LT.random_torque_tangents(TORQUE_N, 2, 0x7A46E8)


def test_torque_restatement_against_50_digits():
    """torque_tangent_np against torque_tangent_mp over every leg of sensitivity_kinematics_restatement.case(65, ...), both contact
    sources, both models, two directions, in EPS x terms: c_tt.  A masked entry is exactly 0."""
    worst = 0.0
    for name, _, b, grf, status, _, t in _torque_cases():
        kin = LT.kin_of(name)
        got = LT.torque_tangent_np(b, grf, status, *_limits(name), t["grf_tan"], t["joint_q_tan"], kin=kin)
        assert 0.1 < got["mask"].mean() < 0.9  # (both sides of the mask are well populated)
        qq, g = b["joint_q"].reshape(-1, 4, 3), grf.reshape(-1, 4, 3)
        for d in range(2):
            dg, dq = t["grf_tan"][d].reshape(-1, 4, 3), t["joint_q_tan"][d].reshape(-1, 4, 3)
            for i in range(TORQUE_N):
                for l in range(4):
                    exact = LT.torque_tangent_mp(l, qq[i, l], g[i, l], got["mask"][i, l], dg[i, l], dq[i, l], kin=kin)
                    val, terms = got["joint_tau_tan"][d, i, l], got["terms"][d, i, l]
                    for c in range(3):
                        if terms[c] == 0:
                            assert val[c] == 0.0 and exact[c] == 0
                        else:
                            worst = max(worst, float(abs(val[c] - exact[c])) / (EPS * terms[c]))
    print("c_tt", worst)
    assert worst <= LT.C_TT, worst


def test_torque_restatement_resolves_every_contact_way_alike():
    """torque_tangent_np on case(257, "stance") with the mask given in each of LT.TORQUE_WAYS: the first four resolve the same mask and
    give the same bits; a per-robot duty that varies is read per robot (shifted by one robot it gives another mask); with no contact
    input every leg of a solved robot emits."""
    n = 257
    b, grf, status, _ = SK.case(n, "stance")
    t = LT.random_torque_tangents(n, 2, 0x7A46EB)
    mask = b["stance"] != 0
    ref = LT.torque_tangent_np({"joint_q": b["joint_q"], "stance": b["stance"]}, grf, status, SK.TAU_MIN, SK.TAU_MAX, t["grf_tan"], t["joint_q_tan"])
    assert 0.2 < mask.mean() < 0.9
    for way in LT.TORQUE_WAYS:
        contact, resolved = LT.torque_contact_inputs(mask, way)
        got = LT.torque_tangent_np(dict(contact, joint_q=b["joint_q"]), grf, status, SK.TAU_MIN, SK.TAU_MAX, t["grf_tan"], t["joint_q_tan"])
        assert np.array_equal(got["emit"], resolved & (status == 0)[:, None]), way
        if way != "none":
            assert np.array_equal(got["joint_tau_tan"], ref["joint_tau_tan"]) and np.array_equal(got["terms"], ref["terms"]), way
        else:
            assert got["emit"].sum() > ref["emit"].sum()
    contact, _ = LT.torque_contact_inputs(mask, "varying_duty")
    shifted = LT.torque_tangent_np(dict(contact, joint_q=b["joint_q"], gait_duty=np.roll(contact["gait_duty"], 1)), grf, status, SK.TAU_MIN, SK.TAU_MAX,
                                   t["grf_tan"], t["joint_q_tan"])
    assert not np.array_equal(shifted["emit"], ref["emit"])


def test_dot_product_identity_against_the_leg_plant_adjoint(P):
    """sum <out_bar, out_tan> = sum <in_bar, in_tan> with the EXISTING leg_plant_adjoint_np and the pool's cotangents on all six
    outputs, at both models; the gap in EPS x the magnitudes of all terms on both sides: c_ldot."""
    worst = 0.0
    for name in LT.KINS:
        kin = LT.kin_of(name)
        s, mask, bars = LA.pool(kin)
        tans = LT.pool_tangents()
        out = {k: v[0] for k, v in _np(P, s, mask, tans, kin).items() if k != "flags"}
        adj = LA.leg_plant_adjoint_np(P["mass"], P["Ib"], *(s[k] for k in LA.INPUTS), mask, LT.INERTIA, LT.DT, bars, kin=kin)
        Rn = LR.leg_plant_step_np(P["mass"], P["Ib"], *(s[k] for k in LA.INPUTS), mask, LT.INERTIA, LT.DT, kin=kin)["Rwb"]
        for k in range(LT.REF_K):
            lhs, rhs, mag = LT.dot_sides(s, Rn, bars, adj, tans, out, k)
            assert (mag > 0).all() and (np.abs(lhs) > 1e-6 * mag).mean() > 0.9  # (the identity is not 0 = 0)
            worst = max(worst, float((np.abs(lhs - rhs) / (EPS * mag)).max()))
    print("c_ldot", worst)
    assert worst <= LT.C_LDOT, worst


def test_dot_product_identity_against_the_kinematics_cotangents():
    """<joint_tau_bar, joint_tau_tan> = <grf_bar, grf_tan> + <joint_q_bar, joint_q_tan> with the EXISTING kin_cotangents (its torque
    half alone: no feet_bar, no `_in`), in EPS x the magnitudes of all terms: c_tdot."""
    worst = 0.0
    for name, _, b, grf, status, cot, t in _torque_cases():
        kin = LT.kin_of(name)
        lo, hi = _limits(name)
        adj = SK.kin_cotangents(b, grf, status, lo, hi, joint_tau_bar=cot["joint_tau_bar"], kin=kin)
        got = LT.torque_tangent_np(b, grf, status, lo, hi, t["grf_tan"], t["joint_q_tan"], kin=kin)
        for d in range(2):
            lhs, rhs, mag = LT.torque_dot_sides(cot["joint_tau_bar"], got["joint_tau_tan"][d], adj["grf_bar"], adj["joint_q_bar"], t["grf_tan"][d], t["joint_q_tan"][d])
            live = mag > 0
            assert live.mean() > 0.5 and np.array_equal(lhs[~live], rhs[~live])
            worst = max(worst, float((np.abs(lhs - rhs)[live] / (EPS * mag[live])).max()))
    print("c_tdot", worst)
    assert worst <= LT.C_TDOT, worst


def test_leg_plant_tangent_against_central_differences_of_the_step(P):
    """<c, out_tan> against central differences of <c, leg_plant_step_np> along the committed tangents in all seven inputs at once, on
    the first LA.FD_N robots of the pool with the adjoint's step LA.FD_H and LA.fd_bar's bar: |FD(h) - FD(2h)| plus the rounding of the
    quotient plus the analytic side's own rounding, 4 EPS x (sum |c| x condition sum).  The rotation moves entrywise along [delta]x Rwb,
    the direction the adjoint's tests use; Rwb's cotangent is paired with [delta']x Rn.  Flagged robots are excluded (the plant has no
    clamp); the excluded share is at most 25 %: measured 0 of 65."""
    n, h = LA.FD_N, LA.FD_H
    s_all, mask_all, bars_all = LA.pool()
    s, mask, bars = {k: a[:n] for k, a in s_all.items()}, mask_all[:n], {k: a[:n] for k, a in bars_all.items()}
    t = {k: v[:, :n] for k, v in LT.pool_tangents().items()}
    out = _np(P, s, mask, t)
    keep = out["flags"] == 0
    print("excluded share", 1.0 - keep.mean())
    assert 1.0 - keep.mean() <= 0.25
    step = lambda d: LR.leg_plant_step_np(P["mass"], P["Ib"], *(d[k] for k in LA.INPUTS), mask, LT.INERTIA, LT.DT)
    Rn = step(s)["Rwb"]
    v = LT.entrywise_direction(s, t)
    fd1, fd2 = LA.fd_of(step, s, bars, v, h)
    an, cond = LT.paired(bars, Rn, out)
    bar = LA.fd_bar(P, s, mask, bars, v, {LA.BAR_OF[k]: np.zeros_like(v[k]) for k in LA.INPUTS}, fd1, fd2, h) + 4 * EPS * cond
    err = np.abs(fd1 - an)
    print("worst error / bar", float((err / bar)[keep].max()), "median bar / |value|", float(np.median((bar / np.abs(an))[keep])))
    assert np.median((bar / np.abs(an))[keep]) < 1e-3  # (the bar is tight: three digits of the loss at least)
    assert np.all(err[keep] <= bar[keep])


def test_torque_tangent_against_central_differences_of_the_oracle(built):
    """joint_tau_tan against central differences of the oracle's torque map, tau = clamp(J(q)^T g) with the oracle's leg Jacobian,
    along the committed tangents in grf_body and joint_q, entry by entry, on case(LA.FD_N, "stance") with the step LA.FD_H at the
    default model.  Entries whose
    raw torque is within 1e-3 N m of a limit at the base point are excluded (the clamp has a kink there) and so are masked legs, whose
    tangent and quotient are both exactly 0.  Bar: |FD(h) - FD(2h)| + 16 EPS terms(tau) / h + 4 EPS terms."""
    from oracle import c_oracle

    kin = c_oracle.default_kinematics()
    n, h = LA.FD_N, LA.FD_H
    b, grf, status, _ = SK.case(n, "stance")
    t = LT.random_torque_tangents(n, 1, 0x7A46E9)
    lo, hi = SK.TAU_MIN, SK.TAU_MAX
    got = LT.torque_tangent_np(b, grf, status, lo, hi, t["grf_tan"], t["joint_q_tan"])
    geo = SK.geometry(b["joint_q"])
    mag = np.einsum("nlrc,nlr->nlc", geo["aJ"], np.abs(grf.reshape(-1, 4, 3)))

    def tau_at(k):
        qq = (b["joint_q"] + k * h * t["joint_q_tan"][0]).reshape(-1, 4, 3)
        g = (grf + k * h * t["grf_tan"][0]).reshape(-1, 4, 3)
        out = np.zeros_like(g)
        for i in range(n):
            for l in range(4):
                if got["emit"][i, l]:
                    out[i, l] = np.clip(np.asarray(c_oracle.leg_jacobian(l, qq[i, l], kin)).reshape(3, 3).T @ g[i, l], lo, hi)
        return out

    fd1, fd2 = (tau_at(1) - tau_at(-1)) / (2 * h), (tau_at(2) - tau_at(-2)) / (4 * h)
    near = (np.abs(got["tau_raw"] - lo) < 1e-3) | (np.abs(got["tau_raw"] - hi) < 1e-3)
    live = got["emit"][..., None] & ~near
    print("excluded share of the emitting entries", float(near[got["emit"]].mean()))
    assert near[got["emit"]].mean() <= 0.25
    val, terms = got["joint_tau_tan"][0], got["terms"][0]
    bar = np.abs(fd1 - fd2) + 16 * EPS * mag / h + 4 * EPS * terms
    assert np.all(np.abs(fd1 - val)[live] <= bar[live]), float((np.abs(fd1 - val) / np.maximum(bar, 1e-300))[live].max())
    assert not val[~got["emit"]].any() and not fd1[~got["emit"]].any()


def test_flagged_pool(P):
    """LA.flagged_pool(): exactly the expected bits, and NaN in every entry of every direction"""
    s, mask, _, expect = LA.flagged_pool()
    n = len(expect)
    out = _np(P, s, mask, LT.random_tangents(n, 3, 0x7A46EA))
    assert np.array_equal(out["flags"], expect)
    for k in LT.OUTPUTS:
        assert np.isnan(out[k][0]).all(), k


# ------------------------------------------------------------------ the C ABI without a device
TORQUE_IO_FIELDS = ["struct_size", "grf_body", "status", "n_dir", "grf_tan", "joint_q_tan", "joint_tau_tan"]
LEG_PLANT_IO_FIELDS = ["struct_size", "Rwb", "x", "xdot", "w", "joint_q", "joint_qdot", "joint_tau", "stance", "gait_phase", "gait_duty", "cmd_state", "leg_inertia",
                       "dt", "n_dir", "Rwb_rot_tan", "x_tan", "xdot_tan", "w_tan", "joint_q_tan", "joint_qdot_tan", "joint_tau_tan", "Rwb_rot_next_tan", "x_next_tan",
                       "xdot_next_tan", "w_next_tan", "joint_q_next_tan", "joint_qdot_next_tan", "flags"]


def test_symbols_are_exported_and_the_abi_stays(built):
    from quadruped_control_amd import _lib, tangent

    lib = ctypes.CDLL(os.path.join(ROOT, "quadruped_control_amd", "libqc_balance.so"))
    for name in ("qc_default_torque_tangent", "qc_torque_tangent_batch", "qc_default_leg_plant_tangent", "qc_leg_plant_step_tangent_batch"):
        assert hasattr(lib, name), name
        assert name not in _lib.EXPORTS  # (bound by tangent.py: the pinned surface is untouched)
    assert _lib.load().qc_abi_version() == 6 and _lib.ABI_VERSION == 6  # new entry points, no change to what existed
    assert ctypes.sizeof(tangent.QcTangentIo) == 136 and ctypes.sizeof(tangent.QcPlantTangentIo) == 160
    for name in ("plan_torque_tangent", "torque_tangent", "plan_leg_plant_step_tangent", "leg_plant_step_tangent", "rollout_tick_tangent",
                 "rollout_tick_transition", "tick_transition_seeds"):
        assert callable(getattr(tangent, name)), name
    assert len(tangent.TICK_TRANSITION_COLUMNS) == 36


@pytest.mark.parametrize("record, fields, size", [("qc_torque_tangent_io", TORQUE_IO_FIELDS, 56), ("qc_leg_plant_tangent_io", LEG_PLANT_IO_FIELDS, 248)])
def test_mirror_matches_the_header(built, tmp_path, record, fields, size):
    """sizeof and the member offsets of the two records as the C compiler lays the header's structs out, against the ctypes mirrors;
    the qc_default_* fill them as documented and need no device."""
    from quadruped_control_amd import tangent

    mirror = {"qc_torque_tangent_io": tangent.QcTorqueTangentIo, "qc_leg_plant_tangent_io": tangent.QcLegPlantTangentIo}[record]
    assert [f for f, _ in mirror._fields_] == fields
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qc_tangent.h"\nint main(void) {\n  printf("%zu", sizeof(' + record + '));\n'
                   + "".join(f'  printf(" %zu", offsetof({record}, {f}));\n' for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(mirror) == size
    assert got[1:] == [getattr(mirror, f).offset for f in fields]
    io = mirror()
    io.grf_body if record == "qc_torque_tangent_io" else io.Rwb
    io.joint_tau_tan, io.struct_size, io.n_dir = 456, 7, 0
    lib = tangent._library()
    if record == "qc_torque_tangent_io":
        lib.qc_default_torque_tangent(ctypes.byref(io))
    else:
        io.dt, io.leg_inertia[1] = -1.0, 3.0
        lib.qc_default_leg_plant_tangent(ctypes.byref(io))
        assert io.dt == 1.0 / 300.0 and list(io.leg_inertia) == [0.0, 0.0, 0.0]
    assert io.struct_size == size and io.n_dir == 1
    assert all(getattr(io, f) is None for f in fields[1:] if f not in ("dt", "n_dir", "leg_inertia"))


def test_argument_checks_need_no_device(built):
    """Both calls refuse a bad call before they touch the device - the handle is null - and the message is their own."""
    from quadruped_control_amd import _lib, tangent

    lib = tangent._library()
    io = tangent.QcLegPlantTangentIo()
    lib.qc_default_leg_plant_tangent(ctypes.byref(io))
    assert lib.qc_leg_plant_step_tangent_batch(None, 1, ctypes.byref(io), None) == -1
    assert _lib.last_error() == "qc_leg_plant_step_tangent_batch: null argument"
    tio = tangent.QcTorqueTangentIo()
    lib.qc_default_torque_tangent(ctypes.byref(tio))
    assert lib.qc_torque_tangent_batch(None, 1, None, ctypes.byref(tio), None) == -1
    assert _lib.last_error() == "qc_torque_tangent_batch: null argument"


@pytest.mark.parametrize("name, ok", [("torque_tangent_host_test", "torque tangent host logic ok"), ("leg_plant_tangent_host_test", "leg plant tangent host logic ok")])
def test_host_logic_without_a_device(name, ok):
    """check_torque_tangent_args / check_leg_plant_tangent_args through every refusal with its message, the kernels' arguments and the
    capped grids (csrc/qc_host.hpp), in stand-alone programs built with the address and undefined-behaviour sanitizers."""
    import __graft_entry__ as g

    assert name in g.HOST_TESTS
    exe = g.build_host_test(name)
    assert exe is not None and os.path.exists(exe)
    libs = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "amdhip64" not in libs and "qc_balance" not in libs, libs
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and ok in r.stdout, r.stdout[-3000:]
