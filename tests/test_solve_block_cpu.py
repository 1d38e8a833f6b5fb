"""No GPU: the two decisions of the strided 4-lane lanes' 6x6 solve block (eqp_diagw, ARITH) that DESIGN 7 entry 26 rewrote,
restated in float64 and held against the forms they replace.

* The SPD flag.  The general form tests `d_k > 0` at each of the six pivots.  The ARITH lanes keep the running minimum of the first
  five pivots (v_min_f64, which DROPS a NaN operand: restated as numpy's fmin) and compare twice: `min(d_0 .. d_4) > 0` and
  `d_5 > 0`.  One compare on the minimum of all six would NOT do - a NaN last pivot would be dropped by the minimum and pass; the
  test shows that case.  With the last pivot's own compare the two forms decide alike on every pivot sequence the factorisation
  can produce: a NaN pivot k makes every later pivot NaN (the recurrence, restated below, shows it on seeded matrices with NaN,
  inf, zero and negative entries planted), so it fails `d_5 > 0` as it failed `d_k > 0`.
* Half the gradient.  The ARITH lanes' solve hands over h = g / 2 and the lane halves its tolerance; every consumer in
  Lane::multipliers_ok / iterate (the per-axis `negative` tests, the tagged arg-min `worst`, `opt`, the polish band, the face code in
  the low bits) decides on (h, thr / 2) as it did on (2 h, thr), exact ties included.

An EMPTY build of a cold robot's first recalculation was weighed and not built (DESIGN 7 entry 26), so nothing restates it here.
"""
import itertools
from fractions import Fraction

import numpy as np

BIG = 1.0e300


# ----------------------------------------------------------------------------------------------------------------- SPD flag
def _six_compares(d):
    ok = True
    for x in d:
        ok = ok and bool(x > 0.0)
    return ok


def _vmin(a, b):
    """v_min_f64 on quiet NaNs: the other operand"""
    return np.fmin(np.float64(a), np.float64(b))


def _min_and_two_compares(d):
    m = np.float64(d[0])
    for k in range(1, 5):
        m = _vmin(m, d[k])
    return bool(m > 0.0) & bool(d[5] > 0.0)


def _one_compare_on_the_minimum_of_six(d):
    m = np.float64(d[0])
    for k in range(1, 6):
        m = _vmin(m, d[k])
    return bool(m > 0.0)


SPECIALS = (0.0, -0.0, -1.5, -1e-300, 5e-324, 1e-310, -5e-324, np.inf, -np.inf, np.nan)


def _nan_closure(d):
    """what the recurrence does to a pivot sequence: from the first NaN on, every pivot is NaN (test_ldlt_pivots_... shows it)"""
    d = np.array(d, np.float64)
    k = np.flatnonzero(np.isnan(d))
    if k.size:
        d[k[0]:] = np.nan
    return d


def test_minimum_and_two_compares_decide_as_six_compares_do():
    rng = np.random.default_rng(0x501D)
    seqs = []
    for _ in range(400):  # positive pivots over many decades, up to three specials planted anywhere
        d = np.exp(rng.uniform(-40.0, 40.0, 6))
        for _ in range(rng.integers(0, 4)):
            d[rng.integers(0, 6)] = SPECIALS[rng.integers(0, len(SPECIALS))]
        seqs.append(d)
    for s in SPECIALS:  # every special alone at every place
        for k in range(6):
            d = np.ones(6)
            d[k] = s
            seqs.append(d)
    for a, b in itertools.product(SPECIALS, SPECIALS):  # pairs next to each other, both orders, at the end of the sequence too
        for k in (0, 3, 4):
            d = np.full(6, 2.5)
            d[k], d[k + 1] = a, b
            seqs.append(d)
    seen = set()
    with np.errstate(all="ignore"):
        for d in seqs:
            d = _nan_closure(d)
            want = _six_compares(d)
            assert _min_and_two_compares(d) == want, d
            seen.add(want)
    assert seen == {True, False}
    # subnormal and inf pivots pass, as they pass `d > 0`
    assert _min_and_two_compares(np.array([5e-324, 1.0, np.inf, 1.0, 1e-310, np.inf]))


def test_one_compare_on_the_minimum_of_all_six_would_pass_a_nan_last_pivot():
    d = np.array([1.0, 2.0, 3.0, 4.0, 5.0, np.nan])
    assert not _six_compares(d)
    assert _one_compare_on_the_minimum_of_six(d)  # the dropped NaN: why the kernel keeps the last pivot's own compare
    assert not _min_and_two_compares(d)


def _rcp_nr(d):
    y = np.float64(1.0) / d
    for _ in range(2):
        e = np.float64(1.0) - d * y
        y = y + y * e
    return y


def _ldlt_pivots(A):
    """eqp_diagw's in-place L D L^T on the packed lower triangle, pivot by pivot (float64; the Newton steps without fma, which moves
    a last bit and no NaN)"""
    M = np.array(A, np.float64)
    piv = []
    for k in range(6):
        d = M[k, k]
        for m in range(k):
            w = M[k, m]
            M[k, m] = w * M[m, m]
            d = d - M[k, m] * w
        piv.append(d)
        M[k, k] = _rcp_nr(d)
        for r in range(k + 1, 6):
            t = M[r, k]
            for m in range(k):
                t = t - M[r, m] * M[k, m]
            M[r, k] = t
    return np.array(piv)


def test_ldlt_pivots_stay_nan_after_the_first_nan_and_both_forms_agree():
    rng = np.random.default_rng(0x1D17)
    seen = set()
    nan_runs = 0
    with np.errstate(all="ignore"):
        for case in range(300):
            B = rng.normal(size=(6, 6))
            A = B @ B.T + 0.5 * np.eye(6)
            if case % 3:  # plant a special on the diagonal or (symmetrically) off it
                r, c = rng.integers(0, 6), rng.integers(0, 6)
                A[r, c] = A[c, r] = SPECIALS[rng.integers(0, len(SPECIALS))]
            d = _ldlt_pivots(A)
            k = np.flatnonzero(np.isnan(d))
            if k.size:
                assert np.isnan(d[k[0]:]).all(), (case, d)
                nan_runs += 1
            want = _six_compares(d)
            assert _min_and_two_compares(d) == want, (case, d)
            seen.add(want)
    assert seen == {True, False} and nan_runs > 10


# -------------------------------------------------------------------------------------------------------- half the gradient
def _fma(a, b, c):
    """correctly rounded a * b + c of finite doubles"""
    return np.float64(float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))))


def _tag(x, code):
    """qc_device.hpp tag(): the face code in the five low mantissa bits"""
    b = np.float64(x).view(np.uint64)
    return ((b & np.uint64(0xFFFFFFFFFFFFFFE0)) | np.uint64(code)).view(np.float64)


def _decisions(g, thr, s, mu, foot):
    """Lane::multipliers_ok and the polish test of Lane::iterate for one foot: (neg x, neg y, neg z, opt, face code of `worst`,
    polish)"""
    sx, sy, sz = s
    lx = -np.float64(sx) * g[0]
    ly = -np.float64(sy) * g[1]
    lz = np.float64(sz) * _fma(mu, lx + ly, -g[2])
    c0 = 3 * foot
    cand = [_tag(lx if sx else BIG, c0), _tag(ly if sy else BIG, c0 + 1), _tag(lz if sz else BIG, c0 + 2)]
    neg = (bool(sx) and bool(lx < thr), bool(sy) and bool(ly < thr), bool(sz) and bool(lz < thr))
    worst = min(cand)
    opt = not bool(worst < thr)
    polish = (not opt) and bool(abs(worst) <= abs(thr))
    return neg + (opt, int(worst.view(np.uint64) & np.uint64(31)), polish)


def test_half_gradient_against_half_threshold_decides_as_the_doubled_value_does():
    rng = np.random.default_rng(0x6A1F)
    mu = 0.6
    states = [s for s in itertools.product((-1, 0, 1), repeat=3) if any(s)]
    cases = []
    for _ in range(600):
        tol = np.float64(10.0 ** rng.uniform(-12, -6)) * (1.0 if rng.random() < 0.5 else -1.0)  # signed: with / without the polish release
        gs = np.float64(max(0.25, abs(rng.normal()) * 10.0 ** rng.uniform(-2, 3)))
        h = rng.normal(size=3) * gs * 10.0 ** rng.uniform(-12, 0, 3)  # from inside the band to clearly outside
        cases.append((tol, gs, h))
    # exact ties: a multiplier equal to the bar, to its negative, and a tagged candidate equal to it bit for bit
    for sign in (1.0, -1.0):
        for gs in (0.25, 1.0, 3.0):
            tol = np.float64(sign * 3.3e-9)
            half_thr = (2.0 * tol) * gs
            for v in (half_thr, -half_thr, np.nextafter(half_thr, 1.0), np.nextafter(half_thr, -1.0)):
                cases.append((tol, np.float64(gs), np.array([v, -v, v])))
                cases.append((tol, np.float64(gs), np.array([-v, v, -v])))
    for code in range(12):
        t = _tag(-7.7e-9, code)
        cases.append((np.float64(t / 2.0), np.float64(1.0), np.array([t, t, t])))  # half_thr = tag(l): the arg-min's own tie
        cases.append((np.float64(-t / 2.0), np.float64(1.0), np.array([-t, -t, -t])))
    seen = set()
    n = 0
    for k, (tol, gs, h) in enumerate(cases):
        h = np.asarray(h, np.float64)
        thr_full = (4.0 * tol) * gs   # the lanes that keep the doubling: tol_s = kTolScale x tol
        thr_half = (2.0 * tol) * gs   # the ARITH lanes: tol_s = kTolScale / 2 x tol
        assert thr_full == 2.0 * thr_half
        g = 2.0 * h
        for s in (states if k % 7 == 0 or k >= 600 else [states[k % len(states)]]):
            foot = k % 4
            a = _decisions(g, thr_full, s, mu, foot)
            b = _decisions(h, thr_half, s, mu, foot)
            assert a == b, (tol, gs, h, s, a, b)
            seen.add(a[3:])
            n += 1
    assert n > 2000
    assert {x[0] for x in seen} == {True, False} and {x[2] for x in seen} == {True, False}
