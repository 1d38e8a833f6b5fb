"""50-digit statement of one working-set recalculation (the equality-constrained QP on a face of the friction cones), for
tests/test_gpu_eqp.py and tests/test_eqp_reference_cpu.py.  Written from the mathematics, not from either device form:

    Q = 2 (A^T S A + W),  c = -2 A^T S b            (balance_controller.cpp:152-153),  A_i = [I; [r_i]x]
    working set:  f = T y + p                        (T, p from the stance mask and the cube states, below)
    (T^T Q T) y = -T^T (Q p + c),   g = Q f + c,   v = S (A f - b)

A foot's cube state (sx, sy, sz) in {-1, 0, 1}^3: sz = +-1 fixes fz at fzmax / fzmin, sx = +-1 binds fx = sx mu fz (so fx follows
fz: a free fz carries it as a multiple, a fixed fz makes it a constant), same for sy; a swing foot has f_i = 0 whatever its state.
The free variables are ordered by their slot 3 i + axis.  Everything is mpmath at DPS digits; the condition numbers and the
magnitudes the bars are stated in are float64 (numpy) of the 50-digit matrices, which is all a bar needs."""
from __future__ import annotations

import mpmath as mp
import numpy as np

DPS = 50


def _m(a):
    a = np.asarray(a, np.float64)
    return mp.matrix([[mp.mpf(float(x)) for x in row] for row in np.atleast_2d(a)])


def _col(a):
    return mp.matrix([mp.mpf(float(x)) for x in np.asarray(a, np.float64).reshape(-1)])


def to_np(M):
    return np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)], np.float64)


def a_matrix(r):
    """A = [A_0 ... A_3], A_i = [I; [r_i]x] (6 x 12) of the exact doubles r [4, 3]"""
    r = np.asarray(r, np.float64).reshape(4, 3)
    A = mp.zeros(6, 12)
    for i in range(4):
        x, y, z = (mp.mpf(float(v)) for v in r[i])
        for k in range(3):
            A[k, 3 * i + k] = mp.mpf(1)
        A[3, 3 * i + 1], A[3, 3 * i + 2] = -z, y
        A[4, 3 * i + 0], A[4, 3 * i + 2] = z, -x
        A[5, 3 * i + 0], A[5, 3 * i + 1] = -y, x
    return A


def prepare(S, W, r, b):
    """What does not depend on the working set: A, S, W, b, Q, c (50 digits) of one robot"""
    with mp.workdps(DPS):
        A, Sm, Wm, bm = a_matrix(r), _m(S), _m(W), _col(b)
        SA = Sm * A
        Q = 2 * (A.T * SA + Wm)
        c = -2 * (SA.T * bm)  # S symmetric: (S A)^T b = A^T S b
        return dict(A=A, S=Sm, W=Wm, b=bm, Q=Q, c=c)


def working_set(mu, fzmin, fzmax, stance, cube):
    """T (12 x nf), p (12) and the slot (3 foot + axis) of every free variable.  stance: 4-bit mask, cube [4, 3] = (sx, sy, sz)."""
    cube = np.asarray(cube, int).reshape(4, 3)
    mu, fzmin, fzmax = (mp.mpf(float(v)) for v in (mu, fzmin, fzmax))
    cols, slots = [], []
    p = mp.zeros(12, 1)
    for i in range(4):
        if not (int(stance) >> i) & 1:
            continue
        sx, sy, sz = (int(v) for v in cube[i])
        if sx == 0:
            cols.append({3 * i: mp.mpf(1)}); slots.append(3 * i)
        if sy == 0:
            cols.append({3 * i + 1: mp.mpf(1)}); slots.append(3 * i + 1)
        if sz == 0:
            cols.append({3 * i: mu * sx, 3 * i + 1: mu * sy, 3 * i + 2: mp.mpf(1)}); slots.append(3 * i + 2)
        else:
            fz = fzmax if sz > 0 else fzmin
            p[3 * i], p[3 * i + 1], p[3 * i + 2] = mu * sx * fz, mu * sy * fz, fz
    order = sorted(range(len(slots)), key=lambda k: slots[k])
    T = mp.zeros(12, len(slots))
    for j, k in enumerate(order):
        for row, val in cols[k].items():
            T[row, j] = val
    return T, p, [slots[k] for k in order]


def solve(prep, mu, fzmin, fzmax, stance, cube):
    """The EQP of one robot on one working set.  Returns 50-digit f, g, v (lists of mpf), y, the working set, and - float64 - the
    masked reduced Hessian the dense forms factorise (H = T^T Q T on the free slots, the identity on the others) with its 2-norm
    condition number."""
    with mp.workdps(DPS):
        A, Q, c, S, b = prep["A"], prep["Q"], prep["c"], prep["S"], prep["b"]
        T, p, slots = working_set(mu, fzmin, fzmax, stance, cube)
        gp = Q * p + c
        if slots:
            Hr = T.T * Q * T
            y = mp.lu_solve(Hr, -(T.T * gp))
            f = T * y + p
        else:
            Hr, y, f = mp.zeros(0, 0), mp.zeros(0, 1), p
        g = Q * f + c
        v = S * (A * f - b)
        H = np.eye(12)
        if slots:
            Hn = to_np(Hr)
            H[np.ix_(slots, slots)] = Hn
        return dict(f=[f[k] for k in range(12)], g=[g[k] for k in range(12)], v=[v[k] for k in range(6)], y=[y[k] for k in range(len(slots))],
                    T=T, p=[p[k] for k in range(12)], slots=slots, H=H, cond_H=float(np.linalg.cond(H, 2)))


def solve_dual(S, w, r, b, mu, fzmin, fzmax, stance, cube):
    """The same EQP for a DIAGONAL W = diag(w) through its dual: (S^-1 + A~ B^-1 A~^T) v = A p - b with A~ = A T and B = T^T W T
    (diagonal: the columns of T have disjoint supports), y = -B^-1 A~^T v, f = T y + p.  Returns f, g = 2 (A^T v + W f), v at 50
    digits and - float64 - the 6 x 6 matrix M the 6x6 device forms factorise with its 2-norm condition number."""
    with mp.workdps(DPS):
        A, Sm, bm, wm = a_matrix(r), _m(S), _col(b), _col(w)
        T, p, slots = working_set(mu, fzmin, fzmax, stance, cube)
        V = mp.inverse(Sm)
        nf = len(slots)
        At = A * T if nf else mp.zeros(6, 0)
        Binv = []
        for j in range(nf):
            s = mp.mpf(0)
            for k in range(12):
                s += T[k, j] * wm[k] * T[k, j]
            Binv.append(1 / s)
        M = V.copy()
        for j in range(nf):
            for a in range(6):
                for c_ in range(6):
                    M[a, c_] += At[a, j] * Binv[j] * At[c_, j]
        v = mp.lu_solve(M, A * p - bm)
        f = p.copy()
        if nf:
            y = mp.matrix([-Binv[j] * sum(At[a, j] * v[a] for a in range(6)) for j in range(nf)])
            f = T * y + p
        Atv = A.T * v
        g = [2 * (Atv[k] + wm[k] * f[k]) for k in range(12)]
        Mn = to_np(M)
        return dict(f=[f[k] for k in range(12)], g=g, v=[v[k] for k in range(6)], slots=slots, M=Mn, cond_M=float(np.linalg.cond(Mn, 2)),
                    At=to_np(At) if nf else np.zeros((6, 0)), Binv=np.array([float(x) for x in Binv]), T=to_np(T) if nf else np.zeros((12, 0)))


def as_float(vals):
    return np.array([float(x) for x in vals], np.float64)


def err_vs(dev, vals):
    """|dev - vals| per entry, the difference taken at 50 digits (dev: float64 array)"""
    with mp.workdps(DPS):
        return np.array([float(abs(mp.mpf(float(d)) - x)) for d, x in zip(np.asarray(dev, np.float64).reshape(-1), vals)], np.float64)
