"""What the finite-difference tests share, CPU and GPU (a plain module, no fixtures): the 480-robot batch and its keep rule, the
hand-picked robots on faces, the committed directions and steps of the rotation and parameter sweeps, and the plant adjoint's bar.
The sweeps that settled each step are recorded in the docstrings of the CPU tests that own them."""
import numpy as np

import quadruped_control_amd as q
from quadruped_control_amd import workloads
from tests import kkt_certificate_restatement as KR
from tests import plant_adjoint_restatement as AR
from tests import plant_restatement as PR

N_FD = 480
FD_H = 1e-4  # the rotation sweep's step (tests/test_sensitivity_rotation_cpu.py settles it); the GPU test uses it too

# parameter groups: (the parameter set's changes, the relative step h, the least share of kept robots with a non-zero contribution
# or None).  tests/test_sensitivity_params_cpu.py holds the sweep that settled each h.  fzmin is raised to 25 N and fzmax lowered to
# 60 N for their own groups, so that feet actually sit on them.
GROUPS = {"gains": ({}, 1e-3, None), "mass": ({}, 1e-2, None), "Ib": ({}, 1e-2, None), "S": ({}, 1e-3, None), "W_diag": ({}, 1e-3, None),
          "W": ({}, 1e-3, None), "mu": ({}, 1e-4, 0.9), "fzmin": ({"fzmin": 25.0}, 1e-3, 0.4), "fzmax": ({"fzmax": 60.0}, 1e-3, 0.5)}


def fd_batch(n=N_FD):
    """config3's states with the 15 non-empty contact patterns in turn"""
    b = workloads.config3(n=n)
    pats = np.array([[(p >> l) & 1 for l in range(4)] for p in range(1, 16)], np.uint8)
    b["stance"] = np.ascontiguousarray(pats[np.arange(n) % 15])
    return b


def fd_directions(n=N_FD):
    """the committed directions: (delta, delta_d) [n, 3] tangent directions and (D, Dd) [n, 9] entrywise ones"""
    rng = np.random.default_rng(8)
    return rng.normal(0.0, 1.0, (n, 3)), rng.normal(0.0, 1.0, (n, 3)), rng.normal(0.0, 1.0, (n, 9)), rng.normal(0.0, 1.0, (n, 9))


def _kept(c, points):
    """the keep rule: solved, no code 3 (flags 0), and the certificate's working set of the oracle's forces unchanged at every point"""
    keep = (c["st0"] == 0) & (c["s"]["flags"] == 0)
    for F, st, a in points:
        keep &= (st == 0) & (a == c["s"]["active"]).all(axis=1)
    return keep


def _check_kept(c, keep):
    assert keep.mean() >= 0.75, ("kept share", keep.mean())
    pats = set((c["b"]["stance"][keep].astype(int) * [1, 2, 4, 8]).sum(axis=1).tolist())
    assert pats == set(range(1, 16)), ("contact patterns among the kept", sorted(pats))


def pinned_cases():
    """Hand-picked robots with forces placed exactly on faces: (name, P, batch of one, grf_body, expected codes of the four feet).
    Foot 0 tied (fx = +mu fz, fz free), foot 1 pinned at fz = fzmax with fy = -mu fz, foot 2 interior, foot 3 swing or fz = fzmin."""
    base = q.cheetah_params(mu=0.6)
    rng = np.random.default_rng(17)
    G = rng.normal(0.0, 1.0, (6, 6))
    S_gen = np.asarray(base["S"], float).reshape(6, 6) + 0.2 * (G @ G.T)
    G = rng.normal(0.0, 1.0, (12, 12))
    W_dense = np.asarray(base["W"], float).reshape(12, 12) + 2e-6 * (G @ G.T)
    cases = []
    for name, P, swing in (("uniform", base, True), ("general-S-dense-W", dict(base, S=S_gen, W=W_dense), True),
                           ("general-S-dense-W-all-stance", dict(base, S=S_gen, W=W_dense), False)):
        mu, fzmin, fzmax = P["mu"], P["fzmin"], P["fzmax"]
        b = workloads.slice_batch(workloads.config3(n=8), 5, 6)
        b["stance"] = np.array([[1, 1, 1, 0 if swing else 1]], np.uint8)
        fw = np.array([[mu * 40.0, 3.0, 40.0], [5.0, -mu * fzmax, fzmax], [2.0, -1.0, 30.0], [0.0, 0.0, 0.0] if swing else [1.0, 2.0, fzmin]])
        R = b["Rwb"][0].reshape(3, 3)
        grf = -(fw @ R).reshape(1, 12)  # grf_body = -R^T f (the round trip through R is not exact: the codes are asserted)
        codes = [2, (1 << 2) | (2 << 4), 0, KR.SWING if swing else (1 << 4)]
        cases.append((name, P, b, grf, codes))
    name, P, b, grf, codes = cases[1]
    b = workloads.with_joint_angles(b)
    cases.append((name + "-joint_q", P, b, grf, codes))
    return cases


BAR_OF = {"Rwb": "Rwb_bar", "x": "x_bar", "xdot": "xdot_bar", "w": "w_bar", "grf_body": "grf_bar", "foot_world": "foot_world_bar"}


def fd_bar(P, s, bars, v, cond, fd1, fd2, h, dt):
    """The bar of <x_bar, v> against FD(h) of the plant step, per robot: the truncation estimated from the differences alone,
    |FD(h) - FD(2h)| (three times the h^2 term of FD(h)), plus the rounding of the quotient - each of its two losses is <c, y> with
    every entry of y within plant_restatement.plant_step_mp's derived bar of the exact step (for a plain double evaluation:
    tests/test_plant_cpu.py; for the device: tests/test_gpu_plant.py), so the quotient is off by at most sum |c_j| bar_j / h - plus the
    analytic side's own rounding, 4 EPS sum condsum_i |v_i| (four times what c_np leaves it, see tests/test_plant_adjoint_cpu.py)."""
    n = fd1.shape[0]
    rounding = np.zeros(n)
    for i in range(n):
        ref = PR.plant_step_mp(P["mass"], P["Ib"], *(s[k][i] for k in AR.INPUTS), dt)
        rounding[i] = sum((np.abs(bars[k][i]) * ref[k][1]).sum() for k in bars)
    analytic = 4 * AR.EPS * sum((cond[BAR_OF[k]] * np.abs(v[k])).sum(axis=1) for k in AR.INPUTS)
    return np.abs(fd1 - fd2) + rounding / h + analytic
