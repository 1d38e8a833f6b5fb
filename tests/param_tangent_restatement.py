"""TEST INFRASTRUCTURE - numpy restatement of the forward mode of the balance QP in the handle's parameters
(csrc/qc_param_tangent.hpp, qc_param_tangent_batch, include/qc_tangent.h), float64, and the same definitions for single robots at 50
digits.  It stands on tests/tangent_restatement.py (EPS, hat) and tests/sensitivity_params_restatement.py (LAYOUT, the parameter
arrays, the state keys), which transposes it.

A direction is 211 doubles in LAYOUT's order, shared by the batch.  On the active face f = Z y + f0 at fixed codes
(sensitivity_restatement.face), with u = A f - b, v = S u, g = 2 (A^T v + W f), H = 2 (A^T S A + W), sx, sy in {-1, 0, +1} from the
x / y codes of a foot that moves (stance, no code 3):
  db    the PD law as tests/kkt_batch.wrench_data states it, differentiated in mass, kff, kp_p, kd_p, kp_w, kd_w and Ib
  df0_l (sx, sy, 0) f_lz dmu with fz free; (sx (dmu f_lz + mu dlim), sy (...), dlim) at a z code 1 (dlim = dfzmin) or 2 (dfzmax)
  w     = H df0 + 2 (A^T dS u + dW f - A^T S db), and on the z entry of a foot with fz free + dmu (sx g_lx + sy g_ly): the moving column
  dy    = -(Z^T H Z)^-1 Z^T w,   df = df0 + Z dy,   grf_tan_l = -R^T df_l,   b_tan = db.
Here A is the explicit 6 x 12 matrix and the reduced system is solved on the EXPLICIT variable-size Z by numpy; the device pads it to
12 x 12.  A reduced matrix that is not positive definite or not finite: every output of the robot NaN in all directions, bit 1.

param_tangent() also returns the CONDITION SUMS the rounding of its outputs is measured against, entry by entry: every term with
the absolute values of all its factors, and through the solve |df0| + |Z| |M^-1| (|Z|^T |w| + |M| |y|), M = Z^T H Z,
|M| = |Z|^T 2 (|A|^T |S| |A| + |W|) |Z| - tangent_restatement's rule - then |R|^T of that.

param_tangent_mp() evaluates one robot and one direction at 50 digits on the exact doubles (the rotation error from
sensitivity_rotation_restatement.log_jacobian_mp, the feet of a joint_q batch from the 50-digit forward kinematics, the reduced
system by mpmath's LU).  C_PT below is the float64 restatement's measured distance from it in EPS x condition sum."""
from __future__ import annotations

import mpmath as mp
import numpy as np

from tests import device_math_reference as DMR
from tests import kkt_certificate_restatement as KR
from tests import sensitivity_params_restatement as PR
from tests import sensitivity_restatement as SR
from tests import sensitivity_rotation_restatement as RR
from tests.tangent_restatement import EPS, hat  # noqa: F401 - the one definition of each, under this module's name too

COUNT, LAYOUT = PR.COUNT, PR.LAYOUT
GROUPS = ("gains", "mass", "Ib", "S", "W", "mu", "fzmin", "fzmax")  # sensitivity_params_restatement.direction()'s groups, one test case each

# The float64 restatement's worst |value - 50-digit value| / (EPS x condition sum) over grf_tan and b_tan, per parameter group (one
# direction of sensitivity_params_restatement.direction(np.random.default_rng(70), group, P) each) on every eighth robot (0, 8, ...
# 128) of solved_batch_support.inputs(130, .), from `feet` and from joint_q - tests/test_param_tangent_cpu.py::
# test_restatement_against_50_digits prints it per group (b_tan: Ib 1.15, gains 1.02, mass 0.47; grf_tan: W 0.63 from joint_q, Ib 0.41,
# gains 0.41, mu 0.39, mass 0.26, fzmax 0.27, fzmin 0.21, S 0.08), rounded up; the device's bar is 4 x it.
C_PT = 1.2
# The measured constant of the pairing identity <grf_bar, grf_tan> = <param_bar_row, param_tan> in float64 numpy against
# sensitivity_params_restatement.param_cotangents, in EPS x (the magnitudes of all terms on both sides) x the reduced condition number
# (pairing_gap), the worst over the groups and the four kinds of robot of tests/test_param_tangent_cpu.py::
# test_pairing_identity_in_numpy, cotangent seed 2 (measured 0.92 in the "W" group on robots at a z code 1 / 2, Ib 0.63, mass 0.44,
# fzmax 0.43, fzmin 0.41, gains 0.37, mu 0.36, S 0.26), rounded up; the device's bar is 4 x it.
C_PAIR = 1.0


def _cross(a, b, m):
    return np.array([a[1] * b[2] + m * (a[2] * b[1]), a[2] * b[0] + m * (a[0] * b[2]), a[0] * b[1] + m * (a[1] * b[0])], dtype=object if a.dtype == object else None)


def _foot_codes(code):
    """(moves, sx, sy, cz) of one foot's active code"""
    code = int(code)
    if code & KR.SWING:
        return False, 0, 0, 0
    cx, cy, cz = code & 3, (code >> 2) & 3, (code >> 4) & 3
    if 3 in (cx, cy, cz):
        return False, 0, 0, 0
    return True, (0, -1, 1)[cx], (0, -1, 1)[cy], cz


def _core(Pn, dP, st, p, gb, codes, e, mag=False):
    """One robot and one direction up to the solve: (db [6], df0 [12], w [12], f [12], R, A [6,12]).  Pn / dP: the parameters and
    their direction as sensitivity_params_restatement._params makes them; st, p, gb, e as its _row takes them.  Works on float and
    on object (mpmath) arrays.  mag: every input replaced by its absolute value and every subtraction by an addition."""
    m = 1 if mag else -1
    ab = (lambda a: abs(a)) if mag else (lambda a: a)
    R, x, xd, xdot, xdotd, w, wd = (ab(st[k]) for k in ("R", "x", "xd", "xdot", "xdotd", "w", "wd"))
    p, gb, e = ab(p), ab(gb), ab(e)
    P = {k: ab(v) for k, v in Pn.items()}
    D = {k: ab(v) for k, v in dP.items()}
    mu, mass, S, W, Ib, kff, g9 = P["mu"], P["mass"], P["S"], P["W"], P["Ib"], P["kff"], P["g"]
    f = (gb @ R.T) * m
    r = p @ R.T
    zero = f[0, 0] * 0
    one = zero + 1
    A = np.array([[zero] * 12 for _ in range(6)], dtype=f.dtype)
    for l in range(4):
        for c in range(3):
            A[c, 3 * l + c] = one
        hr = np.array([[zero, m * r[l, 2], r[l, 1]], [r[l, 2], zero, m * r[l, 0]], [m * r[l, 1], r[l, 0], zero]], dtype=f.dtype)
        A[3:, 3 * l:3 * l + 3] = hr
    fl = f.reshape(12)
    # the PD law and its derivative
    a = P["kp_p"] * (xd + m * x) + P["kd_p"] * (xdotd + m * xdot)
    a = a + np.array([kff[0] * xdotd[0], kff[1] * xdotd[1], kff[2] * mass * g9], dtype=f.dtype)
    a_g = a + m * np.array([zero, zero, g9], dtype=f.dtype)
    al = P["kp_w"] * e + P["kd_w"] * (wd + m * w) + np.array([kff[3] * wd[0], kff[4] * wd[1] + kff[5] * wd[2], zero], dtype=f.dtype)
    Iw = R @ Ib @ R.T
    b = np.concatenate([mass * a_g, Iw @ al + _cross(wd, Iw @ wd, m)])
    u = A @ fl + m * b
    v = S @ u
    g = 2 * (A.T @ v + W @ fl)
    dkff = D["kff"]
    da = D["kp_p"] * (xd + m * x) + D["kd_p"] * (xdotd + m * xdot)
    da = da + np.array([dkff[0] * xdotd[0], dkff[1] * xdotd[1], dkff[2] * mass * g9 + kff[2] * D["mass"] * g9], dtype=f.dtype)
    dal = D["kp_w"] * e + D["kd_w"] * (wd + m * w) + np.array([dkff[3] * wd[0], dkff[4] * wd[1] + dkff[5] * wd[2], zero], dtype=f.dtype)
    dIw = R @ D["Ib"] @ R.T
    db = np.concatenate([D["mass"] * a_g + mass * da, Iw @ dal + dIw @ al + _cross(wd, dIw @ wd, m)])
    # the face's own motion and the moving column
    df0 = np.array([zero] * 12, dtype=f.dtype)
    col = np.array([zero] * 12, dtype=f.dtype)
    for l in range(4):
        moves, sx, sy, cz = _foot_codes(codes[l])
        if not moves:
            continue
        if mag:
            sx, sy = abs(sx), abs(sy)
        dlim = (zero, D["fzmin"], D["fzmax"])[cz]
        tie = D["mu"] * f[l, 2] + mu * dlim
        df0[3 * l:3 * l + 3] = np.array([sx * tie, sy * tie, dlim], dtype=f.dtype)
        if cz == 0:
            col[3 * l + 2] = D["mu"] * (sx * g[3 * l] + sy * g[3 * l + 1])
    wv = 2 * (A.T @ (S @ (A @ df0) + D["S"] @ u + m * (S @ db)) + W @ df0 + D["W"] @ fl) + col
    return db, df0, wv, fl, R, A


def _state(b, i, lift=float):
    """robot i's state arrays as sensitivity_params_restatement._row takes them, and the converter that made them"""
    arr = lambda a, shape: np.array([lift(float(x)) for x in np.asarray(a, np.float64).reshape(-1)], dtype=float if lift is float else object).reshape(shape)
    return {k: arr(b[src][i], shape) for k, src, shape in PR._STATE}, arr


def _direction_params(P, d, conv=float):
    """the direction d [211] in the shapes of sensitivity_params_restatement._params (no "g": gravity has no direction)"""
    out = PR._params(PR.unpack(d, P), conv)
    out.pop("g")
    return out


def param_tangent(P, b, grf_body, param_tan, act_tol=1e-7, kin=None, default_duty=KR.DEFAULT_DUTY):
    """dict(grf_tan [K,n,4,3], b_tan [K,n,6], flags [n], active [n,4], grf_sum [K,n,4,3] and b_sum [K,n,6]: the condition sums of the
    two outputs (module docstring), cond [n]: the reduced condition number) for param_tan [K,211] (or [211]: K = 1).  kin: the
    kinematic model (device_math_reference.Kin) of a batch with joint_q."""
    with np.errstate(invalid="ignore", divide="ignore"):
        b = KR.with_feet(b, kin)
        n = b["x"].shape[0]
        param_tan = np.asarray(param_tan, np.float64).reshape(-1, COUNT)
        K = param_tan.shape[0]
        Pn = PR._params(P)
        dPs = [_direction_params(P, param_tan[k]) for k in range(K)]
        S, Wm, mu = np.asarray(P["S"], float).reshape(6, 6), np.asarray(P["W"], float).reshape(12, 12), float(P["mu"])
        active = KR.certificate(P, b, grf_body, act_tol, default_duty=default_duty)["active"]
        out = dict(grf_tan=np.zeros((K, n, 4, 3)), b_tan=np.zeros((K, n, 6)), flags=np.zeros(n, np.int32), active=active, grf_sum=np.zeros((K, n, 4, 3)),
                   b_sum=np.zeros((K, n, 6)), cond=np.ones(n))
        for i in range(n):
            st, arr = _state(b, i)
            e = RR.log_jacobian(st["Rd"] @ st["R"].T)[0]
            p, gb = arr(b["feet"][i], (4, 3)), arr(grf_body[i], (4, 3))
            Z, flagged = SR.face(active[i], mu)
            Minv, bad, M = None, False, None
            for k in range(K):
                db, df0, wv, fl, R, A = _core(Pn, dPs[k], st, p, gb, active[i], e)
                adb, adf0, awv, _, aR, aA = _core(Pn, dPs[k], st, p, gb, active[i], e, mag=True)
                if k == 0 and Z.shape[1]:
                    M = Z.T @ (2.0 * (A.T @ S @ A + Wm)) @ Z
                    try:
                        if not np.isfinite(M).all():
                            raise np.linalg.LinAlgError
                        np.linalg.cholesky(M)
                        Minv = np.linalg.inv(M)
                        out["cond"][i] = np.linalg.cond(M)
                    except np.linalg.LinAlgError:
                        bad = True
                    out["flags"][i] = 2 if bad else 0
                df, adf = df0.copy(), adf0.copy()
                if bad:
                    df = np.full(12, np.nan)
                elif Minv is not None:
                    y = -np.linalg.solve(M, Z.T @ wv)
                    df = df0 + Z @ y
                    aM = np.abs(Z).T @ (2.0 * (aA.T @ np.abs(S) @ aA + np.abs(Wm))) @ np.abs(Z)
                    adf = adf0 + np.abs(Z) @ (np.abs(Minv) @ (np.abs(Z).T @ awv + aM @ np.abs(y)))
                out["grf_tan"][k, i] = -(df.reshape(4, 3) @ R)  # -R^T df_l, row by row
                out["grf_sum"][k, i] = adf.reshape(4, 3) @ aR
                out["b_tan"][k, i] = db + (np.nan if bad else 0.0)
                out["b_sum"][k, i] = adb
            out["flags"][i] |= 1 if flagged else 0
        return out


def param_tangent_mp(P, b, grf_body, param_tan, i, k, active, kin=None):
    """Robot i, direction k at 50 digits on the exact doubles, with the active codes `active` [4] (as param_tangent() classified
    them).  kin = (hip [12], links [12]): the feet come from joint_q.  Returns dict(grf_tan: 12 mpmath numbers, b_tan: 6)."""
    with mp.workdps(DMR.DPS):
        lift = lambda v: DMR.mpf(float(v))
        st, arr = _state(b, i, lift)
        if kin is not None:
            hip, links = ([DMR.Tr(lift(v)) for v in np.asarray(a, np.float64).reshape(-1)] for a in kin)
            qj = [DMR.Tr(lift(v)) for v in np.asarray(b["joint_q"][i], np.float64).reshape(-1)]
            p = np.array([[x.v for x in DMR._fk_tr(l, qj[3 * l:3 * l + 3], hip, links)] for l in range(4)], dtype=object)
        else:
            p = arr(b["feet"][i], (4, 3))
        e = np.array(RR.log_jacobian_mp(mp.matrix((st["Rd"] @ st["R"].T).tolist()))[0], dtype=object)
        d = np.asarray(param_tan, np.float64).reshape(-1, COUNT)[k]
        Pn = PR._params(P, conv=lift)
        db, df0, wv, fl, R, A = _core(Pn, _direction_params(P, d, lift), st, p, arr(grf_body[i], (4, 3)), active, e)
        Zn, _ = SR.face(active, float(P["mu"]))
        df = df0
        if Zn.shape[1]:
            Z = np.array([[lift(x) for x in row] for row in Zn], dtype=object)
            M = Z.T @ (2 * (A.T @ Pn["S"] @ A + Pn["W"])) @ Z
            y = mp.lu_solve(mp.matrix(M.tolist()), mp.matrix(list(Z.T @ wv)))
            df = df0 - Z @ np.array([y[j] for j in range(len(y))], dtype=object)
        gt = -(df.reshape(4, 3) @ R)
        return dict(grf_tan=list(gt.reshape(-1)), b_tan=list(db))


def pairing(rows, param_tan, k):
    """<param_bar_row, param_tan_k> per robot [n] and the sum of the magnitudes of its terms; rows [n,211] (param_cotangents' or the
    device's), param_tan [K,211]"""
    prod = np.asarray(rows) * np.asarray(param_tan, np.float64).reshape(-1, COUNT)[k][None, :]
    return prod.sum(axis=1), np.abs(prod).sum(axis=1)


def pairing_gap(gbar, grf_tan, rows, param_tan, k, cond, terms=None):
    """(|<grf_bar, grf_tan_k> - <row, param_tan_k>| in units of EPS x (the magnitudes of all terms on both sides) x the reduced
    condition number, <grf_bar, grf_tan_k>) per robot, as tangent_restatement.dot_gap measures it.  terms [n,211]: the adjoint's own
    magnitude sums (param_cotangents' "terms") in place of |rows| on the right - an entry of a row is itself a sum that cancels."""
    n = gbar.shape[0]
    prod = gbar * grf_tan[k].reshape(n, 12)
    rhs, rmag = pairing(rows, param_tan, k)
    if terms is not None:
        rmag = (np.asarray(terms) * np.abs(np.asarray(param_tan, np.float64).reshape(-1, COUNT)[k])[None, :]).sum(axis=1)
    lhs, lmag = prod.sum(axis=1), np.abs(prod).sum(axis=1)
    return np.abs(lhs - rhs) / (EPS * np.maximum(lmag + rmag, 1e-300) * cond), lhs
