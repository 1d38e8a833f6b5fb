"""The virtual support polygon on the CPU: the float64 restatement (tests/support_polygon_restatement.py) against the reference's
known vector, the 50-digit restatement, its symmetries and central differences; the 0/0 case; the exports of the built library."""
from __future__ import annotations

import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from tests import support_polygon_restatement as SP
from tests.device_math_reference import DEFAULT_KIN, EPS, ODD_KIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 24


def node_batch():
    return dict(feet=SP.NODE_FEET[None], gait_phase=SP.NODE_PHASE[None], stance=SP.NODE_STANCE[None])


def test_known_vector():
    """test_node.cpp:41-57: weights 0.9452... (RL, FR) and 0.2118... (FL, RR); com_xy = 0 by symmetry"""
    r = SP.reference_np(node_batch(), SP.NODE_SCHEDULE)
    hi, lo = SP.NODE_WEIGHTS
    assert np.allclose(r["weights"][0], [hi, lo, lo, hi], rtol=4 * EPS, atol=0)
    assert np.abs(r["com_xy"]).max() <= 1e-17 and r["flags"][0] == 0


def test_adjacency_is_the_reference():
    names = ("RL", "FL", "RR", "FR")
    ref = {"RL": ("FL", "RR"), "FL": ("FR", "RL"), "FR": ("RR", "FL"), "RR": ("RL", "FR")}  # trajectory.cpp:75-78
    for l, name in enumerate(names):
        assert (names[SP.MINUS[l]], names[SP.PLUS[l]]) == ref[name]
    assert [names[l] for l in SP.SUM_ORDER] == sorted(names)


@pytest.fixture(scope="module")
def drawn():
    b, sched = SP.pool(N, seed=61, saturating=6)
    bar = np.random.default_rng(5).standard_normal((N, 2))
    return b, sched, bar


@pytest.mark.parametrize("world", [False, True])
@pytest.mark.parametrize("kin,model", [pytest.param(False, DEFAULT_KIN, id="False"), pytest.param(True, DEFAULT_KIN, id="True"),
                                       pytest.param(True, ODD_KIN, id="odd")])
def test_float64_agrees_with_50_digits(drawn, world, kin, model):
    """the measurement behind SP.C_FWD / C_REV (the library's model, both input forms) and SP.C_FWD_ODD / C_REV_ODD (ODD_KIN, joint_q)"""
    b, sched, bar = drawn
    b = {k: v for k, v in b.items() if k != ("feet" if kin else "joint_q")}
    c_fwd, c_rev = (SP.C_FWD_ODD, SP.C_REV_ODD) if model is ODD_KIN else (SP.C_FWD, SP.C_REV)
    f = SP.reference_np(b, sched, world, kin=model)
    ref, cond = SP.reference_mp(b, sched, world, kin=model)
    assert not f["flags"].any() and not ref["flags"].any()
    r = SP.worst_ratio(f["com_xy"], ref["com_xy"], cond["com_xy"])
    print(f"forward world={world} kin={kin} model={model.name}: {r:.3f} EPS x condition sum")
    assert r <= c_fwd
    g, _ = SP.reference_adjoint_np(b, sched, bar, world, kin=model)
    gref, gcond, _ = SP.reference_adjoint_mp(b, sched, bar, world, kin=model)
    for k in SP.OUTPUTS:
        r = SP.worst_ratio(g[k], gref[k], gcond[k])
        print(f"reverse {k} world={world} kin={kin} model={model.name}: {r:.3f} EPS x condition sum")
        assert r <= c_rev


@pytest.mark.parametrize("world", [False, True])
def test_the_odd_model_moves_every_robot(world):
    """com_xy from joint_q at ODD_KIN against com_xy at the library's model, over the first 65 robots of the GPU tests' draw: every
    robot moves by a millimetre or more (printed: 1.1e-3 ... 1.9e-2 m), more than a million times the device's bar (4 C_FWD_ODD EPS x
    condition sum, below 1e-13 m) - a kernel that ignored the handle's model cannot pass the GPU tests at ODD_KIN"""
    b, sched = SP.pool(257, seed=61, saturating=16)
    b, sched = {k: v[:65] for k, v in b.items() if k != "feet"}, sched[:65]
    odd, cond = SP.reference_mp(b, sched, world, kin=ODD_KIN)
    plain = SP.reference_np(b, sched, world)
    moved = np.abs(odd["com_xy"] - plain["com_xy"]).max(axis=1)
    bar = 4.0 * SP.C_FWD_ODD * EPS * cond["com_xy"].max(axis=1)
    print(f"world={world}: com_xy moves by {moved.min():.2e} ... {moved.max():.2e} m; the device's bar is at most {bar.max():.2e} m")
    assert not odd["flags"].any() and (moved > 1e6 * bar).all()


def test_affine_equivariance():
    b, sched = SP.pool(N, seed=62)
    b = {k: v for k, v in b.items() if k != "joint_q"}
    th, t = 0.7, np.array([0.31, -0.22])
    Q = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
    moved = dict(b, feet=b["feet"].copy())
    moved["feet"][:, :, :2] = b["feet"][:, :, :2] @ Q.T + t
    a, c = SP.reference_np(b, sched)["com_xy"], SP.reference_np(moved, sched)["com_xy"]
    assert np.abs(c - (a @ Q.T + t)).max() < 64 * EPS


@pytest.mark.parametrize("world", [False, True])
def test_central_differences(world):
    """every output of the float64 reverse pass against central differences of the float64 forward pass: phases at least 1e-3 from
    the mask's boundaries, so the function is smooth and nothing is left out"""
    n = 6
    b, sched = SP.pool(n, seed=63)
    b = {k: v for k, v in b.items() if k != "joint_q"}
    b["stance"] = np.array([[SP.in_stance(float(p), SP.TROT_DUTY) for p in row] for row in b["gait_phase"]], np.uint8)  # the mask is held
    bar = np.random.default_rng(6).standard_normal((n, 2))
    g, flags = SP.reference_adjoint_np(b, sched, bar, world)
    assert not flags.any()
    h = 1e-6
    loss = lambda bb, ss: (SP.reference_np(bb, ss, world)["com_xy"] * bar).sum(1)
    for name, key, arr in (("feet_bar", "feet", b["feet"]), ("phase_bar", "gait_phase", b["gait_phase"]), ("schedule_bar", None, sched)) + \
            ((("Rwb_bar", "Rwb", b["Rwb"]), ("x_bar", "x", b["x"])) if world else ()):
        flat = arr.reshape(n, -1)
        fd = np.zeros_like(flat)
        for j in range(flat.shape[1]):
            up, dn = flat.copy(), flat.copy()
            up[:, j] += h
            dn[:, j] -= h
            if key is None:
                fd[:, j] = (loss(b, up.reshape(arr.shape)) - loss(b, dn.reshape(arr.shape))) / (2 * h)
            else:
                fd[:, j] = (loss(dict(b, **{key: up.reshape(arr.shape)}), sched) - loss(dict(b, **{key: dn.reshape(arr.shape)}), sched)) / (2 * h)
        err = np.abs(fd - g[name]).max()
        print(f"{name} world={world}: central differences within {err:.2e}")
        assert err < 1e-7 * max(1.0, np.abs(g[name]).max())


def test_zero_over_zero():
    """three swing legs with all widths 0, phases mid-swing: their weights are 0, the point between them is 0/0 - NaN and the flag"""
    b = dict(feet=SP.NODE_FEET[None], gait_phase=np.array([[0.2, 0.75, 0.75, 0.75]]), stance=np.array([[1, 0, 0, 0]], np.uint8))
    sched = np.zeros((4, 4))
    r = SP.reference_np(b, sched)
    assert list(r["weights"][0][1:]) == [0.0, 0.0, 0.0]
    assert r["flags"][0] == 1 << 3 and np.isnan(r["com_xy"]).all()  # FR: its neighbours are RR and FL
    g, flags = SP.reference_adjoint_np(b, sched, np.ones((1, 2)))
    assert flags[0] == 1 << 3 and all(np.isnan(v).all() for v in g.values())
    ref, _ = SP.reference_mp(b, sched)
    assert ref["flags"][0] == 1 << 3


def test_no_robot_of_the_draw_is_flagged():
    b, sched = SP.pool(257, seed=61, saturating=16)
    r = SP.reference_np({k: v for k, v in b.items() if k != "joint_q"}, sched)
    assert not r["flags"].any() and np.isfinite(r["com_xy"]).all()


def test_host_logic_binary():
    """tests/cpp/support_polygon_host_test.cpp: every refusal of check_support_polygon_args and check_support_polygon_adjoint_args and
    the adjacency table, sanitized, stand-alone."""
    import __graft_entry__ as g

    assert "support_polygon_host_test" in g.HOST_TESTS
    exe = g.build_host_test("support_polygon_host_test")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "support polygon host logic ok" in r.stdout


def test_exported_symbols():
    from quadruped_control_amd import _lib

    names = ("qc_default_support_polygon", "qc_support_polygon_batch", "qc_default_support_polygon_adjoint", "qc_support_polygon_adjoint_batch")
    for name in names:
        assert name in _lib.EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    for name in names:
        assert f" T {name}\n" in out
    assert ctypes.sizeof(_lib.QcSupportPolygonIo) == 6 * 8 and ctypes.sizeof(_lib.QcSupportPolygonAdjointIo) == 15 * 8
