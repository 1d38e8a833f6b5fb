"""CPU: the plant step's restatement (tests/plant_restatement.py) on cases with a closed form, the numpy version against the
50-digit one, and the C ABI of qc_plant_step_batch as far as it goes without a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import plant_restatement as PR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EPS = PR.EPS
MASS = 11.0
IB = np.diag([0.011253, 0.036203, 0.042673])  # cheetah_params()
FEET_XY = np.array([[-0.196, 0.127], [0.196, 0.127], [-0.196, -0.127], [0.196, -0.127]])


def _level(n=1, height=0.26):
    """n level robots at rest over four symmetric feet on the ground, no forces"""
    pw = np.zeros((n, 4, 3))
    pw[:, :, :2] = FEET_XY
    z = np.zeros((n, 3))
    return dict(Rwb=np.tile(np.eye(3).reshape(9), (n, 1)), x=np.tile([0.0, 0.0, height], (n, 1)), xdot=z.copy(), w=z.copy(),
                grf_body=np.zeros((n, 12)), foot_world=pw.reshape(n, 12))


def _iterate(s, k, dt):
    s = dict(s)
    for _ in range(k):
        o = PR.plant_step_np(MASS, IB, s["Rwb"], s["x"], s["xdot"], s["w"], s["grf_body"], s["foot_world"], dt)
        s.update({name: o[name] for name in ("Rwb", "x", "xdot", "w")})
    return s


@pytest.mark.parametrize("dt", [1e-4, 1.0 / 300.0, 1e-2])
def test_free_fall_closed_form(dt):
    """No forces: xdot_k = v_0 - k dt g e_z and x_k = x_0 + k dt v_0 - g dt^2 k (k + 1) / 2 (semi-implicit Euler sums the NEW
    velocities); the rotation does not move.  k steps round 2 k additions of terms no larger than the final values: 4 k EPS."""
    k = 300
    s = _level()
    s["xdot"][0] = [0.3, -0.2, 1.5]
    x0, v0 = s["x"].copy(), s["xdot"].copy()
    o = _iterate(s, k, dt)
    ez = np.array([0.0, 0.0, 1.0])
    v_k = v0 - k * dt * PR.G * ez
    x_k = x0 + k * dt * v0 - PR.G * dt * dt * k * (k + 1) / 2 * ez
    scale = np.abs(x0) + k * dt * np.abs(v0) + PR.G * dt * dt * k * (k + 1) / 2
    assert np.all(np.abs(o["xdot"] - v_k) <= 4 * k * EPS * (np.abs(v0) + k * dt * PR.G))
    assert np.all(np.abs(o["x"] - x_k) <= 4 * k * EPS * scale)
    assert np.array_equal(o["Rwb"], s["Rwb"]) and np.array_equal(o["w"], s["w"])


def test_level_body_in_balance_stays_put():
    """Four symmetric feet, each carrying m g / 4: the moments cancel exactly (the lever arms are mirror images, the forces equal),
    so w and Rwb do not move at all; 4 (m g / 4) / m - g is a rounding of g (<= 2 EPS g), which k steps integrate to at most
    EPS g (k dt)^2."""
    k, dt = 300, 1.0 / 300.0
    s = _level()
    s["grf_body"][:] = np.tile([0.0, 0.0, -MASS * PR.G / 4], 4)  # grf_body is the NEGATED force on the body
    o = _iterate(s, k, dt)
    assert np.array_equal(o["Rwb"], s["Rwb"]) and np.array_equal(o["w"], s["w"])
    assert np.all(np.abs(o["x"] - s["x"]) <= EPS * PR.G * (k * dt) ** 2) and np.all(np.abs(o["xdot"]) <= 2 * EPS * PR.G * k * dt)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_spin_about_a_principal_axis(axis):
    """No forces, w along a principal axis of a diagonal Ib: w x (Iw w) = 0, w is constant and after k steps the body has turned
    by exactly k dt w about that axis.  Each step multiplies by a rotation accurate to a few EPS: 8 k EPS."""
    k, dt, rate = 250, 1.0 / 300.0, 2.5
    s = _level()
    s["w"][0, axis] = rate
    o = _iterate(s, k, dt)
    assert np.array_equal(o["w"], s["w"])
    ang = k * dt * rate
    c, sn = np.cos(ang), np.sin(ang)
    i, j = (axis + 1) % 3, (axis + 2) % 3
    want = np.eye(3)
    want[i, i], want[i, j], want[j, i], want[j, j] = c, -sn, sn, c
    assert np.max(np.abs(o["Rwb"].reshape(3, 3) - want)) <= 8 * k * EPS


def _random_cases(rng, n):
    from scipy.spatial.transform import Rotation

    R = Rotation.from_rotvec(rng.uniform(-1, 1, (n, 3)) * rng.uniform(0, np.pi, (n, 1))).as_matrix()
    x = np.array([0.0, 0.0, 0.26]) + rng.uniform(-0.05, 0.05, (n, 3))
    pw = np.zeros((n, 4, 3))
    pw[:, :, :2] = FEET_XY + rng.uniform(-0.03, 0.03, (n, 4, 2))
    grf = rng.uniform(-1, 1, (n, 4, 3)) * np.array([20.0, 20.0, 60.0])
    grf[rng.random((n, 4)) < 0.3] = 0.0
    return dict(Rwb=R.reshape(n, 9), x=x, xdot=rng.uniform(-0.5, 0.5, (n, 3)), w=rng.uniform(-3, 3, (n, 3)),
                grf_body=grf.reshape(n, 12), foot_world=pw.reshape(n, 12))


def test_feet_are_the_new_body_frame_feet():
    s = _random_cases(np.random.default_rng(7), 50)
    o = PR.plant_step_np(MASS, IB, dt=1.0 / 300.0, **s)
    R1 = o["Rwb"].reshape(-1, 3, 3)
    want = np.einsum("nji,nlj->nli", R1, s["foot_world"].reshape(-1, 4, 3) - o["x"][:, None, :])
    assert np.max(np.abs(o["feet"].reshape(-1, 4, 3) - want)) <= 4 * EPS
    assert np.max(np.abs(R1 @ R1.transpose(0, 2, 1) - np.eye(3))) <= 16 * EPS


@pytest.mark.parametrize("dt", [1e-4, 1.0 / 300.0, 1e-2])
def test_numpy_agrees_with_the_50_digit_version(dt):
    """A plain double evaluation of the model stays inside the bars the tracked 50-digit evaluation derives (Er, per output
    entry) - the bars tests/test_gpu_plant.py holds the kernel to.  numpy inverts Ib by LU instead of
    the library's Cholesky: one division per diagonal entry, fewer roundings than the count assumes."""
    s = _random_cases(np.random.default_rng(11), 40)
    s["w"][:4] = 0.0
    s["w"][4:8] = 1e-12
    s["grf_body"][:8:2] = 0.0  # theta = 0 exactly and a tiny theta occur
    o = PR.plant_step_np(MASS, IB, dt=dt, **s)
    worst = {}
    for i in range(40):
        ref = PR.plant_step_mp(MASS, IB, *(s[k][i] for k in ("Rwb", "x", "xdot", "w", "grf_body", "foot_world")), dt)
        for name, r in ref.items():
            worst[name] = max(worst.get(name, 0.0), PR.worst_over_bar(o[name][i], r))
    print(f"dt {dt}: worst error / bar of the numpy restatement: {worst}")
    assert max(worst.values()) <= 1.0, worst
    assert np.array_equal(o["Rwb"][0], s["Rwb"][0]) and np.array_equal(o["Rwb"][2], s["Rwb"][2])  # theta = 0: Exp = I exactly


def test_the_bars_are_a_few_ulps_of_the_largest_term():
    """What the derived bars amount to on an ordinary robot: below 100 ulps of the largest term of each output, i.e. they pin the
    arithmetic and not merely the formula (a wrong sign or a transposed rotation is off by far more: shown on the rotation)."""
    s = _random_cases(np.random.default_rng(3), 1)
    args = [s[k][0] for k in ("Rwb", "x", "xdot", "w", "grf_body", "foot_world")]
    ref = PR.plant_step_mp(MASS, IB, *args, 1.0 / 300.0)
    for name, (val, bar) in ref.items():
        assert np.all(bar <= 100 * EPS * max(1.0, np.max(np.abs(val)))), (name, bar / EPS)
    wrong = PR.plant_step_np(MASS, IB, s["Rwb"].reshape(1, 3, 3).transpose(0, 2, 1).reshape(1, 9), s["x"], s["xdot"], s["w"], s["grf_body"],
                             s["foot_world"], 1.0 / 300.0)
    val, bar = ref["w"]
    assert np.max(np.abs(wrong["w"][0] - val) / bar) > 1e6


def test_the_rollout_start_converges_under_the_checker(built):
    """The start of the closed-loop GPU tests (65 config-2 robots, the reference's default gains): the oracle solves every robot
    at every one of the 200 steps, with and without the 1e-6 force perturbation, the bodies stay upright and near the stand
    height, and the perturbation moves the final state by what tests/test_gpu_plant.py::test_rollout_against_the_cpu_loop quotes."""
    import quadruped_control_amd as q

    P = q.cheetah_params()
    b, pw = PR.rollout_start(65)
    end, status = PR.cpu_rollout(P, b, pw, 200, 1.0 / 300.0)
    end_p, status_p = PR.cpu_rollout(P, b, pw, 200, 1.0 / 300.0, perturb=1e-6)
    assert (status == 0).all() and (status_p == 0).all()
    assert np.all(np.abs(end["x"][:, 2] - 0.26) < 0.05) and np.all(end["Rwb"][:, 8] > 0.99) and np.all(np.abs(end["w"]) < 0.5)
    spread = {k: float(np.abs(end_p[k] - end[k]).max()) for k in ("Rwb", "x", "xdot", "w", "feet")}
    print(f"spread of the final state under a 1e-6 force perturbation: {spread}")
    quoted = dict(Rwb=5.0e-8, x=8.1e-9, xdot=9.0e-8, w=1.0e-5, feet=1.3e-8)
    for k, v in quoted.items():
        assert 0.5 * v <= spread[k] <= 2.0 * v, (k, spread[k])


# ------------------------------------------------------------------ the C ABI without a device
def test_plant_symbols_are_exported(built):
    from quadruped_control_amd import _lib

    lib = ctypes.CDLL(os.path.join(ROOT, "quadruped_control_amd", "libqc_balance.so"))
    for name in ("qc_default_plant", "qc_plant_step_batch"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert _lib.load().qc_abi_version() == 6  # a new entry point, no change to what existed


def test_plant_io_mirror_matches_the_header(built, tmp_path):
    """sizeof and the member offsets of qc_plant_io as the C compiler lays the header's struct out, against the ctypes mirror;
    qc_default_plant fills it as documented and needs no device."""
    from quadruped_control_amd import _lib

    fields = [f for f, _ in _lib.QcPlantIo._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qc_balance.h"\nint main(void) {\n  printf("%zu", sizeof(qc_plant_io));\n'
                   + "".join(f'  printf(" %zu", offsetof(qc_plant_io, {f}));\n' for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_lib.QcPlantIo) == 72
    assert got[1:] == [getattr(_lib.QcPlantIo, f).offset for f in fields]
    io = _lib.QcPlantIo()
    io.Rwb, io.dt, io.struct_size = 123, -1.0, 7
    _lib.load().qc_default_plant(ctypes.byref(io))
    assert io.struct_size == 72 and io.dt == 1.0 / 300.0
    assert all(getattr(io, f) is None for f in fields if f not in ("struct_size", "dt"))


def test_plant_argument_check_needs_no_device(built):
    """qc_plant_step_batch refuses a bad call before it touches the device: the message is its own."""
    from quadruped_control_amd import _lib

    lib = _lib.load()
    io = _lib.QcPlantIo()
    lib.qc_default_plant(ctypes.byref(io))
    assert lib.qc_plant_step_batch(None, 1, ctypes.byref(io), None) == -1 and _lib.last_error() == "qc_plant_step_batch: null argument"


def test_plant_host_logic_without_a_device():
    """The Ib^-1 computation with everything it refuses, the kernel's constants and check_plant_args (csrc/qc_host.hpp) in a
    stand-alone program built with the address and undefined-behaviour sanitizers (tests/cpp/plant_host_test.cpp)."""
    import __graft_entry__ as g

    exe = g.build_host_test("plant_host_test")
    assert exe is not None and os.path.exists(exe)
    libs = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "amdhip64" not in libs and "qc_balance" not in libs, libs
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "plant host logic ok" in r.stdout, r.stdout[-3000:]
