"""TEST INFRASTRUCTURE - numpy restatement of the parameter cotangents (csrc/qc_sensitivity_params.hpp, qc_sensitivity_param_batch),
and the same definitions for single robots at 50 digits.

The layout of a cotangent is the 211 doubles of qc_params in its order (LAYOUT below).  Everything is on the active face at fixed
codes (tests/sensitivity_restatement.face).  Re-derivation: on the face f = Z y + f0 the minimiser has Z^T g(f) = 0.  A parameter
theta moves the face (dphi = dZ y + df0), the gradient at fixed f (dg) and the columns (dZ):
    0 = d(Z^T g) = dZ^T g + Z^T (H (dphi + Z dy) + dg)    =>    dy = -(Z^T H Z)^-1 (Z^T H dphi + dZ^T g + Z^T dg),
    <f_bar, df> = <f_bar, dphi + Z dy> = <f_bar - H z, dphi> - <z, dg> - <dZ lambda, g>,   z = Z lambda, lambda = (Z^T H Z)^-1 Z^T f_bar.
With u = A f - b, v = S u, g = 2 (A^T v + W f), q = S A z, b_bar = 2 q, rho = f_bar - 2 (A^T q + W z):
    S:  dg = 2 A^T dS u           S_bar = -2 (A z) u^T              W:  dg = 2 dW f        W_bar = -2 z f^T
    b:  dg = -2 A^T S db          every parameter of the PD law gets b_bar through the law as tests/kkt_batch.wrench_data states it
    mu: a tied or pinned fx = sx mu fz has dphi_l = (sx fz, sy fz, 0) d mu, and where fz is free the column of fz moves by (sx, sy, 0):
        mu_bar = sum_l <rho_l, (sx f_lz, sy f_lz, 0)> - [fz free] z_lz (sx g_lx + sy g_ly)
    fzmin (z code 1), fzmax (z code 2): f0_l = (sx mu, sy mu, 1) fz_pinned:  <rho_l, (sx mu, sy mu, 1)>
A foot with a code 3 contributes nothing to the three face entries; a NaN adjoint makes the whole row NaN.

One routine serves three uses: float64 (numpy arrays), 50 digits (object arrays of mpmath numbers), and - with mag=True - the
`terms`: every input replaced by its absolute value and every subtraction by an addition, i.e. per entry the sum of the magnitudes
of its contributions, the scale rounding errors are measured against."""
from __future__ import annotations

import mpmath as mp
import numpy as np

from tests import device_math_reference as DMR
from tests import kkt_certificate_restatement as KR
from tests.kkt_certificate_restatement import distance  # noqa: F401 - the one definition, under this module's name too
from tests import sensitivity_rotation_restatement as RR

COUNT = 211
LAYOUT = {}
for _name, _shape in (("mu", ()), ("mass", ()), ("fzmin", ()), ("fzmax", ()), ("Ib", (3, 3)), ("S", (6, 6)), ("W", (12, 12)), ("kff", (6,)),
                      ("kp_p", (3,)), ("kd_p", (3,)), ("kp_w", (3,)), ("kd_w", (3,))):
    _at = sum(int(np.prod(s, dtype=int)) for _, s in LAYOUT.values())
    LAYOUT[_name] = (slice(_at, _at + int(np.prod(_shape, dtype=int))), _shape)
GRAVITY = 9.81


def pack(P):
    """the 211 values of a parameter dict, in LAYOUT's order"""
    return np.concatenate([np.asarray(P[k], np.float64).reshape(-1) for k in LAYOUT])


def unpack(theta, like):
    """a parameter dict with the 211 values of `theta` in the shapes of `like` (other keys of `like` kept)"""
    P = dict(like)
    for k, (sl, shape) in LAYOUT.items():
        v = np.asarray(theta[sl], np.float64).reshape(shape)
        P[k] = float(v) if shape == () else v
    return P


def direction(rng, group, P):
    """a random direction [211] inside one parameter group: "gains" (kp_p, kd_p, kp_w, kd_w, kff), "mass", "Ib" / "S" / "W" (dense
    symmetric), "W_diag", "mu", "fzmin", "fzmax" - scaled by the size of the parameters it moves, so that h is a RELATIVE step"""
    d = np.zeros(COUNT)
    sym = lambda k: (lambda G: (G + G.T) / 2.0)(rng.normal(0.0, 1.0, LAYOUT[k][1]))
    if group == "gains":
        for k in ("kp_p", "kd_p", "kp_w", "kd_w"):
            d[LAYOUT[k][0]] = rng.normal(0.0, 1.0, 3) * np.abs(np.asarray(P[k], float))
        d[LAYOUT["kff"][0]] = rng.normal(0.0, 1.0, 6)
    elif group in ("mass", "mu", "fzmin", "fzmax"):
        d[LAYOUT[group][0]] = float(P[group])
    elif group in ("Ib", "S", "W"):
        M = np.asarray(P[group], float).reshape(LAYOUT[group][1])
        dg = np.sqrt(np.abs(np.diag(M)))
        d[LAYOUT[group][0]] = (sym(group) * np.outer(dg, dg)).reshape(-1)
    elif group == "W_diag":
        d[LAYOUT["W"][0]] = np.diag(rng.normal(0.0, 1.0, 12) * np.diag(np.asarray(P["W"], float).reshape(12, 12))).reshape(-1)
    else:
        raise ValueError(group)
    return d


def _cross(a, b, m):
    return np.array([a[1] * b[2] + m * (a[2] * b[1]), a[2] * b[0] + m * (a[0] * b[2]), a[0] * b[1] + m * (a[1] * b[0])], dtype=a.dtype)


def _row(Pn, st, p, gb, gbar, z, codes, e, mag=False):
    """One robot's row [211].  Pn: dict of arrays / numbers (mu, mass, fzmin, fzmax, Ib [3,3], S [6,6], W [12,12], kff, kp_p, kd_p,
    kp_w, kd_w); st: dict R, Rd [3,3], x, xd, xdot, xdotd, w, wd [3]; p, gb, gbar [4,3]; z [12]; codes [4] ints; e [3] the rotation
    error.  Works on float and on object (mpmath) arrays.  mag: the magnitude sums (see the module's docstring)."""
    m = 1 if mag else -1
    ab = (lambda a: abs(a)) if mag else (lambda a: a)
    R, x, xd, xdot, xdotd, w, wd = (ab(st[k]) for k in ("R", "x", "xd", "xdot", "xdotd", "w", "wd"))
    p, gb, gbar, z, e = ab(p), ab(gb), ab(gbar), ab(z), ab(e)
    P = {k: ab(v) for k, v in Pn.items()}
    mu, mass, S, W, Ib, kff = P["mu"], P["mass"], P["S"], P["W"], P["Ib"], P["kff"]
    g9 = P["g"]
    f = (gb @ R.T) * m
    fbar = (gbar @ R.T) * m
    r = p @ R.T
    zz = z.reshape(4, 3)
    zero = f[0, 0] * 0
    Af = np.array([zero] * 6, dtype=f.dtype)
    Az = np.array([zero] * 6, dtype=f.dtype)
    for l in range(4):
        Af[:3] = Af[:3] + f[l]
        Af[3:] = Af[3:] + _cross(r[l], f[l], m)
        Az[:3] = Az[:3] + zz[l]
        Az[3:] = Az[3:] + _cross(r[l], zz[l], m)
    # the PD law
    a = P["kp_p"] * (xd + m * x) + P["kd_p"] * (xdotd + m * xdot)
    a = a + np.array([kff[0] * xdotd[0], kff[1] * xdotd[1], kff[2] * mass * g9], dtype=f.dtype)
    a_g = a + m * np.array([zero, zero, g9], dtype=f.dtype)
    blin = mass * a_g
    al = P["kp_w"] * e + P["kd_w"] * (wd + m * w) + np.array([kff[3] * wd[0], kff[4] * wd[1] + kff[5] * wd[2], zero], dtype=f.dtype)
    Iw = R @ Ib @ R.T
    bang = Iw @ al + _cross(wd, Iw @ wd, m)
    b = np.concatenate([blin, bang])
    u = Af + m * b
    v = S @ u
    q = S @ Az
    bb = 2 * q
    fl, zl = f.reshape(12), zz.reshape(12)
    Wf, Wz = (W @ fl).reshape(4, 3), (W @ zl).reshape(4, 3)
    g = np.array([2 * (v[:3] + _cross(v[3:], r[l], m) + Wf[l]) for l in range(4)])
    hz = np.array([2 * (q[:3] + _cross(q[3:], r[l], m) + Wz[l]) for l in range(4)])
    rho = fbar + m * hz
    mub = fminb = fmaxb = zl.sum() * 0  # (a NaN adjoint reaches the three face entries whatever the codes, as on the device)
    for l in range(4):
        code = int(codes[l])
        if code & KR.SWING:
            continue
        cx, cy, cz = code & 3, (code >> 2) & 3, (code >> 4) & 3
        if 3 in (cx, cy, cz):
            continue
        sx, sy = (0, -1, 1)[cx], (0, -1, 1)[cy]
        if mag:
            sx, sy = abs(sx), abs(sy)
        tie = sx * rho[l, 0] + sy * rho[l, 1]
        mub = mub + tie * f[l, 2]
        if cz == 0:
            mub = mub + m * (zz[l, 2] * (sx * g[l, 0] + sy * g[l, 1]))
        lim = mu * tie + rho[l, 2]
        if cz == 1:
            fminb = fminb + lim
        if cz == 2:
            fmaxb = fmaxb + lim
    massb = bb[0] * a_g[0] + bb[1] * a_g[1] + bb[2] * a_g[2] + bb[2] * mass * (kff[2] * g9)
    abl = mass * bb[:3]
    ba = bb[3:]
    alb = Iw.T @ ba
    Iw_bar = np.outer(ba, al) + np.outer(_cross(ba, wd, m), wd)
    Ibb = R.T @ Iw_bar @ R
    kffb = np.array([abl[0] * xdotd[0], abl[1] * xdotd[1], abl[2] * (mass * g9), alb[0] * wd[0], alb[1] * wd[1], alb[1] * wd[2]], dtype=f.dtype)
    parts = [np.array([mub, massb, fminb, fmaxb], dtype=f.dtype), Ibb.reshape(9), (m * 2 * np.outer(Az, u)).reshape(36),
             (m * 2 * np.outer(zl, fl)).reshape(144), kffb, abl * (xd + m * x), abl * (xdotd + m * xdot), alb * e, alb * (wd + m * w)]
    return np.concatenate(parts)


def _params(P, conv=float):
    dt = float if conv is float else object
    arr = lambda k, shape: np.array([conv(v) for v in np.asarray(P[k], np.float64).reshape(-1)], dtype=dt).reshape(shape)
    out = {k: (conv(float(P[k])) if shape == () else arr(k, shape)) for k, (_, shape) in LAYOUT.items()}
    out["g"] = conv(GRAVITY)
    return out


_STATE = (("R", "Rwb", (3, 3)), ("Rd", "Rwb_d", (3, 3)), ("x", "x", (3,)), ("xd", "x_d", (3,)), ("xdot", "xdot", (3,)), ("xdotd", "xdot_d", (3,)),
          ("w", "w", (3,)), ("wd", "w_d", (3,)))


def param_cotangents(P, b, grf_body, grf_bar, adjoint, act_tol=1e-7, active=None, default_duty=KR.DEFAULT_DUTY):
    """dict(rows [n,211], terms [n,211], active [n,4]) of qc_sensitivity_param_batch's per-robot output, float64, from the batch the
    solve read, its forces, the cotangent on them and the adjoint z qc_sensitivity_batch returned for it."""
    with np.errstate(invalid="ignore", divide="ignore"):
        b = KR.with_feet(b)
        n = b["x"].shape[0]
        if active is None:
            active = KR.certificate(P, b, grf_body, act_tol, default_duty=default_duty)["active"]
        Pn = _params(P)
        rows, terms = np.zeros((n, COUNT)), np.zeros((n, COUNT))
        for i in range(n):
            st = {k: np.asarray(b[src][i], float).reshape(shape) for k, src, shape in _STATE}
            e = RR.log_jacobian(st["Rd"] @ st["R"].T)[0]
            args = (b["feet"][i].reshape(4, 3), np.asarray(grf_body[i], float).reshape(4, 3), np.asarray(grf_bar[i], float).reshape(4, 3),
                    np.asarray(adjoint[i], float).reshape(12), active[i], e)
            rows[i] = _row(Pn, st, *args)
            terms[i] = _row(Pn, st, *args, mag=True)
        return dict(rows=rows, terms=terms, active=active)


def param_cotangents_mp(P, b, grf_body, grf_bar, adjoint, i, active, kin=None):
    """Robot i's row at 50 digits on the exact doubles, with the active codes `active` [4].  kin = (hip [12], links [12]): the feet
    come from joint_q.  Returns a flat list of 211 mpmath numbers."""
    with mp.workdps(DMR.DPS):
        lift = lambda v: DMR.mpf(float(v))
        arr = lambda a, shape: np.array([lift(x) for x in np.asarray(a, np.float64).reshape(-1)], dtype=object).reshape(shape)
        st = {k: arr(b[src][i], shape) for k, src, shape in _STATE}
        if kin is not None:
            hip, links = ([DMR.Tr(lift(v)) for v in np.asarray(a, np.float64).reshape(-1)] for a in kin)
            q = [DMR.Tr(lift(v)) for v in np.asarray(b["joint_q"][i], np.float64).reshape(-1)]
            p = np.array([[x.v for x in DMR._fk_tr(l, q[3 * l:3 * l + 3], hip, links)] for l in range(4)], dtype=object)
        else:
            p = arr(b["feet"][i], (4, 3))
        Re = mp.matrix((st["Rd"] @ st["R"].T).tolist())
        e = np.array(RR.log_jacobian_mp(Re)[0], dtype=object)
        row = _row(_params(P, conv=lift), st, p, arr(grf_body[i], (4, 3)), arr(grf_bar[i], (4, 3)), arr(adjoint[i], (12,)), active, e)
        return list(row)
