"""CPU: the plant steps with a model restated in numpy (tests/plant_model_restatement.py) against their own 50-digit variants, the
reverse pass against the forward restatement, and the host logic of include/qc_plant_model.h as far as it goes without a device.

c_np, the worst |numpy - 50 digits| / (EPS x condition sum) per output over the pools (257 robots each, dt = 1/300) and over the seven
combinations of present and absent mass / Ib / wrench, measured here and asserted not to exceed plant_model_restatement.C_NP:
    step      measured  Rwb 1.15  x 0.94  xdot 1.00  w 1.70  feet 1.44
              C_NP      Rwb 1.2   x 1.0   xdot 1.1   w 1.8   feet 1.5
    adjoint   measured  Rwb_bar 1.68  x_bar 1.24  xdot_bar 0.96  w_bar 0.99  grf_bar 1.79  foot_world_bar 1.78  wrench_bar 1.72  mass_bar 1.14  Ib_bar 2.38
              C_NP      Rwb_bar 1.7   x_bar 1.3   xdot_bar 1.0   w_bar 1.0   grf_bar 1.8   foot_world_bar 1.8   wrench_bar 1.8   mass_bar 1.2   Ib_bar 2.4
    leg       measured  Rwb 0.002  x 0.72  xdot 0.04  w 0.0003  foot_world 0.53  joint_q (swing) 0.95  joint_qdot (swing) 1.00
              C_NP      Rwb 0.01   x 0.8   xdot 0.05  w 0.01    foot_world 0.6   joint_q 1.0           joint_qdot 1.1
tests/test_gpu_plant_model.py holds the device to 4 C_NP of the same scale."""
import os
import subprocess

import numpy as np
import pytest

import quadruped_control_amd as q
from tests import plant_model_restatement as MR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def P(built):
    return q.cheetah_params()


def test_numpy_restatements_against_50_digits(P):
    """The three numpy maps within C_NP EPS condition sum of the 50-digit maps on the same doubles, for every combination; the legged
    step's stance joints, which have no condition sum, are left to the GPU test's measured bar."""
    s, bars, model = MR.pool()
    ls, mask, lmodel = MR.leg_pool()
    worst = {"step": {}, "adjoint": {}, "leg": {}}
    up = lambda d, k, v: d.__setitem__(k, max(d.get(k, 0.0), v))
    for combo in MR.COMBOS:
        kw = MR.select(model, combo)
        got, ref = MR.plant_step_model_np(P, s, MR.DT, **kw), MR.step_reference(combo)
        assert not got["flags"].any()
        for k in MR.STEP_OUTPUTS:
            up(worst["step"], k, MR.worst_ratio(got[k], ref[k]))
        got, ref = MR.plant_adjoint_model_np(P, s, MR.DT, bars, **kw), MR.adjoint_reference(combo)
        for k in MR.ADJOINT_OUTPUTS:
            up(worst["adjoint"], k, MR.worst_ratio(got[k], ref[k]))
        got, ref = MR.leg_plant_step_model_np(P, ls, mask, MR.LEG_INERTIA, MR.DT, **MR.select(lmodel, combo)), MR.leg_reference(combo)
        assert not got["flags"].any() and not got["leg_flags"].any()
        for k in MR.LEG_OUTPUTS:
            up(worst["leg"], k, MR.worst_ratio(got[k], ref[k]))
    print("worst |numpy - 50 digits| / (EPS condition sum):", worst)
    for call, w in worst.items():
        for k, v in w.items():
            assert v <= MR.C_NP[call][k], (call, k, v, MR.C_NP[call][k])
            assert v > 0.0, (call, k)


def test_pool_covers_what_it_claims():
    s, bars, model = MR.pool()
    assert 0.5 <= model["mass"].min() and model["mass"].max() <= 50.0
    I = model["Ib"].reshape(-1, 3, 3)
    assert np.array_equal(I, I.transpose(0, 2, 1)) and np.linalg.cond(I).max() > 300.0 and (np.linalg.cond(I) <= 1.001e3).all()
    w = model["wrench"]
    assert (~w.any(axis=1)).sum() >= 50 and np.abs(w[:, :3]).max() > 250.0 and np.abs(w[:, 3:]).max() > 80.0
    assert ((~w[:, :3].any(axis=1)) & w[:, 3:].any(axis=1)).any() and ((~w[:, 3:].any(axis=1)) & w[:, :3].any(axis=1)).any()


def _directions(n):
    rng = np.random.default_rng(0xB0D4)
    return {k: rng.normal(0.0, 1.0, (n, m)) for k, m in (("Rwb", 9), ("x", 3), ("xdot", 3), ("w", 3), ("grf_body", 12), ("foot_world", 12), ("wrench", 6),
                                                          ("mass", 1), ("Ib", 9))}


BAR_OF = {"Rwb": "Rwb_bar", "x": "x_bar", "xdot": "xdot_bar", "w": "w_bar", "grf_body": "grf_bar", "foot_world": "foot_world_bar", "wrench": "wrench_bar",
          "mass": "mass_bar", "Ib": "Ib_bar"}


def _moved(s, model, v, k):
    """the inputs and the model moved by k along v (mass [n] along v["mass"][:, 0])"""
    s2 = {name: np.ascontiguousarray(a + k * v[name]) for name, a in s.items()}
    m2 = dict(wrench=model["wrench"] + k * v["wrench"], mass=model["mass"] + k * v["mass"][:, 0], Ib=model["Ib"] + k * v["Ib"])
    return s2, m2


def test_adjoint_against_the_forward_restatement(P):
    """The dot-product identity <y_bar, J v> = <x_bar, v> in all nine inputs at once - the six of the step, the wrench, the mass and
    Ib ENTRYWISE (the perturbed Ib is not symmetric: the arithmetic assumes no symmetry) - with J v from central differences:
      - of the 50-digit step at h = 1e-6 on 12 robots against the 50-digit adjoint: the differences carry no rounding, their
        truncation is h^2 times the third derivative, 1e-12 of the scale |x_bar| |v|; asserted to 1e-9 of it;
      - of the numpy step at h = 1e-5 on the first 65 robots against the numpy adjoint, to |FD(h) - FD(2h)| + 1e-7 of the scale
        (rounding of the quotient: EPS / h = 2e-11 times the loss's condition, tests/test_plant_adjoint_cpu.py's sweep)."""
    n = 65
    s, bars, model = ({k: a[:n] for k, a in d.items()} for d in MR.pool())
    v = _directions(n)
    v["mass"] = v["mass"] * 0.1  # (masses down to 0.5 kg)
    v["Ib"] = v["Ib"] * 1e-4     # (moments down to 1e-5 kg m^2)
    loss = lambda out: sum((np.asarray(out[k]).reshape(bars[k].shape) * bars[k]).sum(axis=1) for k in bars)
    an = MR.plant_adjoint_model_np(P, s, MR.DT, bars, **model)
    dd = sum((an[BAR_OF[k]].reshape(n, -1) * v[k]).sum(axis=1) for k in v)
    scale = np.sqrt(sum((an[BAR_OF[k]].reshape(n, -1) ** 2).sum(axis=1) for k in v)) * np.sqrt(sum((v[k] ** 2).sum(axis=1) for k in v))

    def at(k, h):
        s2, m2 = _moved(s, model, v, k * h)
        return loss(MR.plant_step_model_np(P, s2, MR.DT, check=False, **m2))  # (the moved Ib is not symmetric: the arithmetic alone)

    h = 1e-5
    fd1, fd2 = (at(1, h) - at(-1, h)) / (2 * h), (at(2, h) - at(-2, h)) / (4 * h)
    err = np.abs(fd1 - dd)
    print("numpy: worst relative error", float((err / scale).max()), "worst |FD(h) - FD(2h)|", float((np.abs(fd1 - fd2) / scale).max()))
    assert np.all(err <= np.abs(fd1 - fd2) + 1e-7 * scale)
    # 50 digits
    h, rows = 1e-6, (0, 1, 2, 3, 4, 5, 6, 7, 30, 40, 50, 64)
    for i in rows:
        row = lambda d: {k: a[i] for k, a in d.items()}
        ref = MR.plant_adjoint_model_mp(P, row(s), MR.DT, row(bars), **row(model))
        pair = sum((ref[BAR_OF[k]][0] * v[k][i]).sum() for k in v)

        def at_mp(k):
            s2, m2 = _moved(s, model, v, k * h)
            out = MR.plant_step_model_mp(P, row(s2), MR.DT, **row(m2))
            return sum((out[name][0] * bars[name][i]).sum() for name in bars)

        fd = (at_mp(1) - at_mp(-1)) / (2 * h)
        assert abs(fd - pair) <= 1e-9 * scale[i], (i, fd, pair, scale[i])


def _faces(P, b, grf_body, act_tol=1e-7):
    """The active face of the forces `grf_body` [n, 12]: per foot and axis -1, 0 or +1 - tests/kkt_batch.py's row classification at
    act_tol (the lower / upper friction row of x and of y, fzmin / fzmax), the rule qc_certify_batch and the sensitivity calls read
    the face by.  Returns an int array [n, 4, 3]."""
    n = b["x"].shape[0]
    mu, fzmin, fzmax = P["mu"], P["fzmin"], P["fzmax"]
    fw = -np.einsum("nij,nkj->nki", b["Rwb"].reshape(n, 3, 3), grf_body.reshape(n, 4, 3))
    fx, fy, fz = fw[..., 0], fw[..., 1], fw[..., 2]
    tol = act_tol * (1.0 + np.abs(fz) * mu)
    sx = np.where(mu * fz - fx <= tol, 1, 0) - np.where(mu * fz + fx <= tol, 1, 0)
    sy = np.where(mu * fz - fy <= tol, 1, 0) - np.where(mu * fz + fy <= tol, 1, 0)
    sz = np.where(fzmax - fz <= act_tol * (1.0 + fzmax), 1, 0) - np.where(fz - fzmin <= act_tol * (1.0 + fzmin), 1, 0)
    return np.stack([sx, sy, sz], axis=-1)


def test_active_sets_of_the_rollout_gradient_test_stay_within_the_cap(P):
    """The C oracle's active sets alone, on the CPU, on the inputs of tests/test_gpu_plant_model.py's rollout gradient test: the base
    rollout and the four displaced ones (k = -2 ... 2 times h along the committed directions in the plant's mass, Ib and the step-0
    push; C oracle in the loop, numpy plant with the model's body and pushes).  A robot is kept when every solve succeeded and the
    face of its forces (_faces, act_tol = 1e-7) is the same at all five points at EVERY step - the GPU test's rule on the device's
    working-set word; at least 0.8 of the robots must remain, the cap that test applies."""
    from oracle import c_oracle

    n, H, h = MR.ROLLOUT_N, MR.ROLLOUT_STEPS, MR.ROLLOUT_H
    b, pw, model = MR.standing(n)
    v = MR.rollout_directions(n)

    def run(k):
        cur = {name: np.array(a) for name, a in b.items()}
        m = {name: model[name] + k * h * v[name] for name in ("mass", "Ib")}
        push = model["wrench"].copy()
        push[0] += k * h * v["wrench"]
        ok, faces = np.ones(n, bool), []
        for step in range(H):
            grf, st, _ = c_oracle.control_batch(P, cur)
            ok &= st == 0
            faces.append(_faces(P, cur, grf))
            s = dict({name: cur[name] for name in ("Rwb", "x", "xdot", "w")}, grf_body=grf, foot_world=pw)
            out = MR.plant_step_model_np(P, s, MR.DT, mass=m["mass"], Ib=m["Ib"], wrench=push[step])
            assert not out["flags"].any()
            cur.update({name: a for name, a in out.items() if name != "flags"})
        return ok, np.stack(faces)  # [H, n, 4, 3]

    ok0, f0 = run(0)
    keep = ok0.copy()
    for k in (-2, -1, 1, 2):
        ok, f = run(k)
        keep &= ok & (f == f0).all(axis=(0, 2, 3))
    print("kept", keep.mean(), "robots with a non-empty face at some step of the base rollout:", int(f0.any(axis=(0, 2, 3)).sum()), "of", n)
    assert keep.mean() >= 0.8, keep.mean()
    # the classification sees a face where there is one: a force put on a row is on the face, one moved off it by 1e-3 N is not
    R = np.eye(3).reshape(1, 9)
    one = {"x": np.zeros((1, 3)), "Rwb": R}
    fz = 50.0
    g = -np.tile(np.array([P["mu"] * fz, 0.0, fz]), 4).reshape(1, 12)
    assert _faces(P, one, g)[0].tolist() == [[1, 0, 0]] * 4
    g[0, 0] += 1e-3
    assert _faces(P, one, g)[0].tolist() == [[0, 0, 0]] + [[1, 0, 0]] * 3
    g = -np.tile(np.array([0.0, -P["mu"] * P["fzmin"], P["fzmin"]]), 4).reshape(1, 12)
    assert _faces(P, one, g)[0].tolist() == [[0, -1, -1]] * 4


def test_flags_of_the_restatement():
    nan = float("nan")
    mass = np.array([1.0, 0.0, -2.0, nan, np.inf, 5e-324])
    assert MR.model_flags_np(6, mass=mass).tolist() == [0, 1, 1, 1, 1, 0]
    eye = np.eye(3).reshape(9)
    bad = np.stack([eye, np.diag([1.0, -1.0, 1.0]).reshape(9), np.array([1, 2, 0, 2, 1, 0, 0, 0, 1.0]), np.array([1, 0, 0, 0, 1, 0.25, 0, 0, 1.0]),
                    np.array([1, 0, 0, 0, nan, 0, 0, 0, 1.0]), np.zeros(9), np.array([1, 1e-13, 0, 0, 1, 0, 0, 0, 1.0])])
    assert MR.model_flags_np(7, Ib=bad).tolist() == [0, 2, 2, 2, 2, 2, 0]
    full = np.array([[0.05, 0.01, -0.004], [0.01, 0.08, 0.006], [-0.004, 0.006, 0.11]])
    assert np.abs(MR.inverse3_np(full.reshape(1, 9))[0] @ full - np.eye(3)).max() < 64 * MR.EPS


def test_host_logic_without_a_device():
    """Every refusal of the three calls of include/qc_plant_model.h with its message, the body's constants under a model and the
    instantiation a model selects (csrc/qc_host.hpp), in a stand-alone program built with the address and undefined-behaviour
    sanitizers (tests/cpp/plant_model_host_test.cpp)."""
    import __graft_entry__ as g

    assert "plant_model_host_test" in g.HOST_TESTS
    exe = g.build_host_test("plant_model_host_test")
    assert exe is not None and os.path.exists(exe)
    libs = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "amdhip64" not in libs and "qc_balance" not in libs, libs
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "plant model host logic ok" in r.stdout, r.stdout[-3000:]


def test_module_and_symbols(built):
    """q.plant_model is reachable as q.tangent is, binds its own symbols, and leaves _lib.EXPORTS alone"""
    from quadruped_control_amd import _lib

    pm = q.plant_model
    lib = pm._library()
    for name in ("qc_default_plant_model", "qc_default_plant_model_bar", "qc_plant_step_model_batch", "qc_leg_plant_step_model_batch",
                 "qc_plant_step_model_adjoint_batch"):
        assert hasattr(lib, name) and name not in _lib.EXPORTS, name
    rec = pm.QcPlantModel()
    lib.qc_default_plant_model(rec)
    assert rec.struct_size == 40 and not (rec.mass or rec.Ib or rec.wrench_world or rec.flags)
    assert lib.qc_plant_step_model_batch(None, 0, None, None, None) == -1 and _lib.last_error() == "qc_plant_step_model_batch: null argument"
