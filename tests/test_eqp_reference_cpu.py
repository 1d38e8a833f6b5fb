"""CPU: the 50-digit EQP reference (tests/eqp_reference.py) checked against itself and against recorded forces, before
tests/test_gpu_eqp.py holds the device's working-set recalculations to it."""
import json
import os

import mpmath as mp
import numpy as np

from oracle import numpy_restatement as NR
from tests import eqp_reference as E

GOLD = os.path.join(os.path.dirname(__file__), "golden", "balance_golden.json")
MU, FZMIN, FZMAX = 0.6, 10.0, 120.0
S_DIAG = np.diag([1.0, 1.0, 1.0, 10.0, 10.0, 5.0])


def _robots(n, seed):
    rng = np.random.default_rng(seed)
    nominal = np.array([[-0.196, 0.127, -0.26], [0.196, 0.127, -0.26], [-0.196, -0.127, -0.26], [0.196, -0.127, -0.26]])
    for _ in range(n):
        r = nominal + rng.uniform(-0.04, 0.04, (4, 3))
        b = np.array([20.0, 10.0, 108.0, 3.0, 3.0, 1.0]) * rng.uniform(-1.0, 1.0, 6) + np.array([0, 0, 108.0, 0, 0, 0])
        stance = int(rng.integers(0, 16))
        cube = rng.integers(-1, 2, (4, 3))
        yield r, b, stance, cube, rng


def _spd(rng, n, lo, hi):
    q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    M = (q * np.exp(rng.uniform(np.log(lo), np.log(hi), n))) @ q.T
    return (M + M.T) / 2


def test_reduced_gradient_vanishes():
    """T^T g = 0 to 1e-40 (relative to |T|^T (|Q| |f| + |c|)) on random working sets, S and W full SPD"""
    worst = 0.0
    for r, b, stance, cube, rng in _robots(40, 11):
        S, W = _spd(rng, 6, 0.5, 20.0), _spd(rng, 12, 1e-6, 1e-3)
        prep = E.prepare(S, W, r, b)
        o = E.solve(prep, MU, FZMIN, FZMAX, stance, cube)
        with mp.workdps(E.DPS):
            g = mp.matrix(o["g"])
            red = o["T"].T * g if o["slots"] else mp.zeros(0, 1)
            Qa, fa, ca = np.abs(E.to_np(prep["Q"])), np.abs(E.as_float(o["f"])), np.abs(E.as_float([prep["c"][k] for k in range(12)]))
            scale = float(np.max(Qa @ fa + ca)) + 1.0
            for k in range(len(o["slots"])):
                worst = max(worst, float(abs(red[k])) / scale)
    assert worst <= 1e-40, worst


def test_dual_and_primal_statements_agree_on_diagonal_w():
    """the 6 x 6 dual statement and the 12 x 12 primal one: the same f, g and v to 1e-40 (relative) for diagonal W, S full SPD"""
    worst = 0.0
    for r, b, stance, cube, rng in _robots(40, 12):
        S = _spd(rng, 6, 0.5, 20.0)
        w = np.exp(rng.uniform(np.log(1e-7), np.log(1e-3), 12))
        a = E.solve(E.prepare(S, np.diag(w), r, b), MU, FZMIN, FZMAX, stance, cube)
        d = E.solve_dual(S, w, r, b, MU, FZMIN, FZMAX, stance, cube)
        assert a["slots"] == d["slots"]
        with mp.workdps(E.DPS):
            for key in ("f", "g", "v"):
                scale = max(1.0, max(float(abs(x)) for x in a[key]))
                worst = max(worst, max(float(abs(x - y)) for x, y in zip(a[key], d[key])) / scale)
    assert worst <= 1e-40, worst


def test_swing_and_fixed_feet_are_exact():
    """a swing foot's force is exactly 0 and a fully fixed foot's exactly p = fz (sx mu, sy mu, 1), whatever the other feet do"""
    for r, b, stance, cube, rng in _robots(30, 13):
        fixed = int(rng.integers(0, 4))
        stance |= 1 << fixed
        cube[fixed] = [rng.choice([-1, 1]), rng.choice([-1, 1]), rng.choice([-1, 1])]
        o = E.solve(E.prepare(S_DIAG, _spd(rng, 12, 1e-6, 1e-3), r, b), MU, FZMIN, FZMAX, stance, cube)
        with mp.workdps(E.DPS):
            for i in range(4):
                if not (stance >> i) & 1:
                    assert all(o["f"][3 * i + k] == 0 for k in range(3))
            fz = mp.mpf(FZMAX if cube[fixed][2] > 0 else FZMIN)
            p = [mp.mpf(MU) * int(cube[fixed][0]) * fz, mp.mpf(MU) * int(cube[fixed][1]) * fz, fz]
            assert [o["f"][3 * fixed + k] for k in range(3)] == p and [o["p"][3 * fixed + k] for k in range(3)] == p


def _golden_working_set(f, stance, mu, fzmin, fzmax, tol=1e-9):
    """the faces of the cones the recorded force sits on, within `tol` relative"""
    cube = np.zeros((4, 3), int)
    for i in range(4):
        if not stance[i]:
            continue
        fx, fy, fz = f[3 * i:3 * i + 3]
        cube[i, 2] = 1 if fz >= fzmax * (1 - tol) else (-1 if fz <= fzmin * (1 + tol) else 0)
        m = mu * fz
        for k, v in ((0, fx), (1, fy)):
            cube[i, k] = 1 if v >= m - tol * max(1.0, m) else (-1 if v <= -m + tol * max(1.0, m) else 0)
    return cube


def test_eqp_on_the_optimal_working_set_reproduces_the_golden_forces():
    """balance_golden.json: the recorded world-frame forces are the EQP's solution on the working set read off them (the faces tight
    within 1e-9 relative), to the 1e-8 of max(1, |f|) the file's forces hold (tests/test_oracle_cpu.py)"""
    with open(GOLD) as fh:
        cases = json.load(fh)["cases"]
    worst = 0.0
    for c in cases:
        P = NR.cheetah_params(c["mu"])
        P["fzmin"], P["fzmax"] = c["fzmin"], c["fzmax"]
        qp = NR.assemble(P, np.array(c["Rwb"]).reshape(3, 3), np.array(c["Rwb_d"]).reshape(3, 3), np.array(c["x"]), np.array(c["xdot"]),
                         np.array(c["w"]), np.array(c["x_d"]), np.array(c["xdot_d"]), np.array(c["w_d"]), c["feet"], c["stance"])
        A, b = qp["A"], qp["b"]
        r = np.array([[A[5, 3 * i + 1], A[3, 3 * i + 2], A[4, 3 * i + 0]] for i in range(4)])  # [r]x: (5,1) = x, (3,2) = y, (4,0) = z
        fw = np.array(c["f_world"], np.float64)
        mask = sum(1 << i for i in range(4) if c["stance"][i])
        cube = _golden_working_set(fw, c["stance"], c["mu"], c["fzmin"], c["fzmax"])
        o = E.solve(E.prepare(P["S"], P["W"], r, b), c["mu"], c["fzmin"], c["fzmax"], mask, cube)
        err = float(np.max(E.err_vs(fw, o["f"]))) / max(1.0, float(np.abs(fw).max()))
        worst = max(worst, err)
        assert err <= 1e-8, (c.get("name"), err, cube.tolist())
    print(f"golden forces vs the EQP on their working set: worst {worst:.2e}")
