"""The COM reference on the CPU: the float64 restatement (tests/com_reference_restatement.py) against the 50-digit restatement and
central differences, the two identities of its modes, the equal-weights case of the offset, the documented order of schedule_bar_sum
against math.fsum, the sanitized host test and the exports of the built library."""
from __future__ import annotations

import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from tests import com_reference_restatement as CR
from tests import support_polygon_restatement as SP
from tests.device_math_reference import DEFAULT_KIN, EPS, ODD_KIN

N = 24
GAIN = 0.7


@pytest.fixture(scope="module")
def drawn():
    b, sched = SP.pool(N, seed=61, saturating=6)
    rng = np.random.default_rng(5)
    return b, sched, rng.standard_normal((N, 3)), rng.uniform(-1.0, 1.0, (N, 3))


@pytest.mark.parametrize("mode", CR.MODES)
@pytest.mark.parametrize("kin,model", [pytest.param(False, DEFAULT_KIN, id="False"), pytest.param(True, DEFAULT_KIN, id="True"),
                                       pytest.param(True, ODD_KIN, id="odd")])
def test_float64_agrees_with_50_digits(drawn, mode, kin, model):
    """the measurement behind CR.C_FWD and CR.C_REV (the library's model, both input forms) and CR.C_FWD_ODD / C_REV_ODD (ODD_KIN, joint_q)"""
    b, sched, bar, x_d = drawn
    b = {k: v for k, v in b.items() if k != ("feet" if kin else "joint_q")}
    c_fwd, c_rev = (CR.C_FWD_ODD, CR.C_REV_ODD) if model is ODD_KIN else (CR.C_FWD, CR.C_REV)
    f = CR.reference_np(b, sched, x_d, mode, GAIN, kin=model)
    ref, cond = CR.reference_mp(b, sched, x_d, mode, GAIN, kin=model)
    assert not f["flags"].any() and not ref["flags"].any()
    r = SP.worst_ratio(f["x_d"], ref["x_d"], cond["x_d"])
    print(f"forward mode={mode} kin={kin} model={model.name}: {r:.3f} EPS x condition sum")
    assert r <= c_fwd and np.array_equal(f["x_d"][:, 2], x_d[:, 2])
    g, _ = CR.reference_adjoint_np(b, sched, bar, mode, GAIN, kin=model)
    gref, gcond, _ = CR.reference_adjoint_mp(b, sched, bar, mode, GAIN, kin=model)
    for k in CR.OUTPUTS:
        r = SP.worst_ratio(g[k], gref[k], gcond[k])
        print(f"reverse {k} mode={mode} kin={kin} model={model.name}: {r:.3f} EPS x condition sum")
        assert r <= c_rev


@pytest.mark.parametrize("mode", CR.MODES)
def test_the_odd_model_moves_every_robot(mode):
    """x_d from joint_q at ODD_KIN against x_d at the library's model, over the first 65 robots of the GPU tests' draw: every robot moves
    by far more than the device's bar (4 C_FWD_ODD EPS x condition sum) - a kernel that ignored the handle's model cannot pass the GPU
    tests at ODD_KIN.  (In offset mode only gain x (com - centroid) moves, a smaller step than the polygon's own.)"""
    b, sched = SP.pool(257, seed=61, saturating=16)
    b, sched = {k: v[:65] for k, v in b.items() if k != "feet"}, sched[:65]
    x_d = np.random.default_rng(79).uniform(-1.0, 1.0, (65, 3))
    odd, cond = CR.reference_mp(b, sched, x_d, mode, GAIN, kin=ODD_KIN)
    plain = CR.reference_np(b, sched, x_d, mode, GAIN)
    moved = np.abs(odd["x_d"] - plain["x_d"])[:, :2].max(axis=1)
    bar = 4.0 * CR.C_FWD_ODD * EPS * cond["x_d"][:, :2].max(axis=1)
    print(f"mode={mode}: x_d moves by {moved.min():.2e} ... {moved.max():.2e} m; the device's bar is at most {bar.max():.2e} m")
    assert not odd["flags"].any() and (moved > 1e6 * bar).all()


def test_replace_is_the_polygon_and_zero_gain_is_the_input(drawn):
    b, sched, bar, x_d = drawn
    b = {k: v for k, v in b.items() if k != "joint_q"}
    r = CR.reference_np(b, sched, x_d)
    assert np.array_equal(r["x_d"][:, :2], SP.reference_np(b, sched, world=True)["com_xy"]) and np.array_equal(r["com_xy"], r["x_d"][:, :2])
    assert np.array_equal(CR.reference_np(b, sched, x_d, "offset", 0.0)["x_d"], x_d)
    g, _ = CR.reference_adjoint_np(b, sched, bar)
    p, _ = SP.reference_adjoint_np(b, sched, bar[:, :2], world=True)
    assert all(np.array_equal(g[k], p[k]) for k in SP.OUTPUTS), "replace: the polygon's reverse pass from the cotangent's x, y"
    assert np.array_equal(g["x_d_in_bar"], bar * np.array([0.0, 0.0, 1.0]))
    assert np.array_equal(CR.reference_adjoint_np(b, sched, bar, "offset", GAIN)[0]["x_d_in_bar"], bar)


@pytest.mark.parametrize("mode", CR.MODES)
def test_central_differences(mode):
    """every output of the float64 reverse pass against central differences of the float64 forward pass (h = 1e-6; the bound as
    tests/test_support_polygon_cpu.py argues it): phases at least 1e-3 from the mask's boundaries, the mask held"""
    n = 6
    b, sched = SP.pool(n, seed=63)
    b = {k: v for k, v in b.items() if k != "joint_q"}
    b["stance"] = np.array([[SP.in_stance(float(p), SP.TROT_DUTY) for p in row] for row in b["gait_phase"]], np.uint8)
    rng = np.random.default_rng(6)
    bar, x_d = rng.standard_normal((n, 3)), rng.uniform(-1.0, 1.0, (n, 3))
    g, flags = CR.reference_adjoint_np(b, sched, bar, mode, GAIN)
    assert not flags.any()
    h = 1e-6
    loss = lambda bb, ss, xx: (CR.reference_np(bb, ss, xx, mode, GAIN)["x_d"] * bar).sum(1)
    for name, key, arr in (("feet_bar", "feet", b["feet"]), ("phase_bar", "gait_phase", b["gait_phase"]), ("schedule_bar", "schedule", sched),
                           ("Rwb_bar", "Rwb", b["Rwb"]), ("x_bar", "x", b["x"]), ("x_d_in_bar", "x_d", x_d)):
        flat = arr.reshape(n, -1)
        fd = np.zeros_like(flat)
        for j in range(flat.shape[1]):
            vals = []
            for sign in (1.0, -1.0):
                moved = flat.copy()
                moved[:, j] += sign * h
                moved = moved.reshape(arr.shape)
                vals.append(loss(b if key in ("schedule", "x_d") else dict(b, **{key: moved}), moved if key == "schedule" else sched,
                                 moved if key == "x_d" else x_d))
            fd[:, j] = (vals[0] - vals[1]) / (2 * h)
        err = np.abs(fd - g[name]).max()
        print(f"{name} mode={mode}: central differences within {err:.2e}")
        assert err < 1e-7 * max(1.0, np.abs(g[name]).max())
        assert np.abs(g[name]).max() > 0


def test_equal_weights_leave_the_offset_at_its_input(drawn):
    """All four widths huge, every leg in stance: with d = width sqrt2 the two erf arguments phi / d and (1 - phi) / d are tiny,
    erf a = 2 a / sqrt(pi) (1 - a^2 / 3 + ...), so w_l = 1 / (d sqrt(pi)) (1 + O(d^-2)) whatever the phase - the weights are equal to
    a relative d^-2.  Equal weights w make the mean of the virtual points the centroid in exact arithmetic (each foot enters once as
    itself and once as each neighbour: (1 + 2 w + 2 (1 - w)) / 3 = 1), so x_d_out lies within the condition bar of x_d_in: C_FWD x
    EPS x condition sum for the float64 restatement, plus the d^-2 spread of the weights times gain times the size of the polygon
    (feet within 0.5 m of their centroid)."""
    b, _, _, x_d = drawn
    b = dict({k: v for k, v in b.items() if k != "joint_q"}, stance=np.ones((N, 4), np.uint8))
    width = 1.0e8
    got = CR.reference_np(b, np.full((4, 4), width), x_d, "offset", GAIN)
    _, cond = CR.reference_mp(b, np.full((4, 4), width), x_d, "offset", GAIN)
    assert not got["flags"].any()
    spread = (width * math.sqrt(2.0)) ** -2 * GAIN * 0.5
    excess = np.abs(got["x_d"] - x_d) / (CR.C_FWD * EPS * cond["x_d"] + spread)
    print(f"equal weights: |x_d_out - x_d_in| at most {excess.max():.3f} of the condition bar")
    assert excess.max() <= 1.0
    assert np.array_equal(got["x_d"][:, 2], x_d[:, 2])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 64 * CR.SUM_MAX_BLOCKS + 1])
def test_ordered_sum_against_fsum(n):
    """the documented order adds n numbers per entry one by one in some order: within n EPS sum |rows| of the exact sum"""
    rng = np.random.default_rng(n)
    rows = rng.standard_normal((n, 16)) * np.exp(rng.uniform(-6.0, 6.0, (n, 1)))
    if n > 1000:  # (the pure-Python walk of 65 537 rows: keep four entries moving, the rest zero)
        rows[:, 4:] = 0.0
    got = CR.ordered_sum(rows)
    for e in range(16):
        exact, mag = math.fsum(rows[:, e]), math.fsum(np.abs(rows[:, e]))
        assert abs(got[e] - exact) <= n * EPS * mag
    if n == 1:
        assert np.array_equal(got, rows[0])


def test_ordered_sum_takes_the_grid_stride():
    """past 1024 x 64 robots partial 0 also owns robot 65 536: moving that row between pieces changes which partial it enters"""
    n = 64 * CR.SUM_MAX_BLOCKS + 1
    rows = np.zeros((n, 16))
    rows[0, 0], rows[n - 1, 0], rows[64, 0] = 1.0, 2.0 ** -53, -1.0
    # partial 0 = (1 + 2^-53) = 1 (rounded), partial 1 = -1: the sum is 0; in plain index order it would be 2^-53
    assert CR.ordered_sum(rows)[0] == 0.0 and np.sum(rows[:, 0]) != 1.0


def test_host_logic_binary():
    """tests/cpp/com_reference_host_test.cpp: every refusal of check_com_reference_args and check_com_reference_adjoint_args and the
    geometry of the summing reverse pass, sanitized, stand-alone."""
    import __graft_entry__ as g

    assert "com_reference_host_test" in g.HOST_TESTS
    exe = g.build_host_test("com_reference_host_test")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "com reference host logic ok" in r.stdout


def test_exported_symbols():
    from quadruped_control_amd import _lib

    names = ("qc_default_com_reference", "qc_com_reference_batch", "qc_default_com_reference_adjoint", "qc_com_reference_adjoint_batch")
    for name in names:
        assert name in _lib.EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    for name in names:
        assert f" T {name}\n" in out
    assert ctypes.sizeof(_lib.QcComReferenceIo) == 8 * 8 and ctypes.sizeof(_lib.QcComReferenceAdjointIo) == 18 * 8
    assert os.path.exists(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "qc_com_reference.hpp"))
