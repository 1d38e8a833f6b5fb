"""No GPU: the ratio test and the multiplier test of Lane::iterate / Lane::multipliers_ok as DESIGN 7 entry 27 rewrote them,
restated on bit patterns and held against the forms they replace.

* The two Z faces of a foot as one candidate (step_cand_z) against the pair of step_cand calls: whenever the pair's minimum can
  block, the merged candidate is that minimum bit for bit (the same slack and the same |dz| reach the reciprocal - the stand-in
  below is a hash of its operand's bits, sign included, so any other operand would show); otherwise both carry +BIG's high word,
  and the low word of a ratio that does not block is never read (`blocked`, `beta` and the face code under `blocked` are compared
  on whole feet).
* The multiplier candidates with only their high word selected (big_unless) and `neg` compared on that selected value: `opt`, the
  face code of `worst`, the release masks (one field, or the drop-all strategy's negbits) applied to the working-set word, the
  polish flag, `neg` itself and negbits.  A bar of +inf (a non-finite scale; no tolerance produces it on finite data) is the one
  place where `neg` answers differently - an inactive face's 1e300 lies below it - and there the masks only name fields that are
  already free, so the word after the release is compared.
* The directions as the negated step operand: -(f - f^) against f^ - f.  Equal bits except for equal operands (-0 against +0), a
  zero direction with which no candidate can block; the candidates of whole feet are compared.  The step itself keeps f - f^: the
  last test shows the signed zero that fma(beta, -(f^ - f), f^) would change.

`can` keeps its two compares (one compare against max(slack, eps) was weighed and not taken), so nothing restates it here.
"""
import itertools
import struct

import numpy as np

BIG = 1.0e300
BIG_HI = 0x7E37E43C
M64 = (1 << 64) - 1
EPS = 1e-14


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def _val(b):
    return np.float64(struct.unpack("<d", struct.pack("<Q", b & M64))[0])


assert _bits(BIG) >> 32 == BIG_HI


def _rcp(x):
    """opaque stand-in for v_rcp_f64: about 1 / x, its low mantissa bits a hash of the operand's bit pattern"""
    with np.errstate(all="ignore"):
        r = np.float64(1.0) / np.float64(x)
    if not np.isfinite(r) or r == 0.0:
        return r
    h = (_bits(x) * 0x9E3779B97F4A7C15) & M64
    return _val(_bits(r) ^ ((h >> 40) & 0xFF))


def _vmin(a, b):
    """v_min_f64 on bit patterns: a quiet NaN operand is dropped"""
    fa, fb = _val(a), _val(b)
    if np.isnan(fa):
        return b
    if np.isnan(fb):
        return a
    return a if fa < fb else b


def _tree(c):
    """the min tree of iterate() / multipliers_ok()"""
    c = list(c)
    w = len(c)
    while w > 1:
        for k in range(w // 2):
            c[k] = _vmin(c[k], c[k + (w + 1) // 2])
        w = (w + 1) // 2
    return c[0]


def _step_cand(free, slack, nd, code):
    with np.errstate(all="ignore"):
        can = bool(free) and bool(nd > EPS) and bool(slack < nd)
        a = np.float64(slack) * _rcp(nd)
    b = _bits(a)
    hi = (b >> 32) if can else BIG_HI
    return (hi << 32) | (b & 0xFFFFFFE0) | code


def _z_pair(free, slack_lo, slack_hi, dz, c4):
    return _vmin(_step_cand(free, slack_lo, -np.float64(dz), c4), _step_cand(free, slack_hi, np.float64(dz), c4 + 1))


def _z_merged(free, slack_lo, slack_hi, dz, c4):
    up = bool(np.float64(dz) > 0.0)
    return _step_cand(free, slack_hi if up else slack_lo, np.abs(np.float64(dz)), c4 + 1 if up else c4)


def _same_to_every_reader(a, b):
    """two ratios (or multipliers) as their readers see them: both +BIG's high word (not blocking / not active: the low word is
    not read), or the same bits"""
    if a >> 32 == BIG_HI or b >> 32 == BIG_HI:
        return a >> 32 == b >> 32
    return a == b


DZ = (0.0, -0.0, 1e-14, -1e-14, 1e-15, -1e-15, 5e-324, -5e-324, 1e-310, -1e-310, np.inf, -np.inf, np.nan,
      np.nextafter(1e-14, 1.0), -np.nextafter(1e-14, 1.0), 0.37, -0.37, 12.5, -12.5, 1e200, -1e200)


def test_merged_z_candidate_is_the_pairs_minimum_wherever_it_is_read():
    rng = np.random.default_rng(0x27A710)
    cases = []
    for dz in DZ:
        a = abs(dz)
        slacks = [0.0, -0.0, -1e-9, -3.0, 0.25 * a if np.isfinite(a) else 1.0, a, np.nextafter(a, 0.0) if np.isfinite(a) else 7.0,
                  np.nextafter(a, np.inf) if np.isfinite(a) else 9.0, 2.0 * a if np.isfinite(a) else 1e300, np.nan, np.inf, 41.0]
        for sl, sh in itertools.product(slacks, repeat=2):
            cases.append((sl, sh, dz))
    for _ in range(3000):
        dz = rng.normal() * 10.0 ** rng.uniform(-16, 3)
        cases.append((rng.normal() * 10.0 ** rng.uniform(-16, 3) + 1.0, abs(rng.normal()) * 10.0 ** rng.uniform(-16, 3), dz))
    seen_codes, blocking = set(), 0
    for k, (sl, sh, dz) in enumerate(cases):
        if (np.isinf(sl) and sl < 0) or (np.isinf(sh) and sh < 0):
            continue  # -inf x rcp(inf) is a NaN ratio: an infinite force or bound, which no running robot holds
        for free in (True, False):
            c4 = 6 * (k % 4) + 4
            old, new = _z_pair(free, sl, sh, dz, c4), _z_merged(free, sl, sh, dz, c4)
            assert _same_to_every_reader(old, new), (sl, sh, dz, free, hex(old), hex(new))
            if new >> 32 != BIG_HI:
                assert free and abs(dz) > EPS
                blocking += 1
                seen_codes.add((new & 31) - c4)
                # the operand bits of the face that can block: its own slack and nd = |dz| > 0
                assert new == _step_cand(True, sh if dz > 0 else sl, abs(dz), c4 + (1 if dz > 0 else 0))
    assert seen_codes == {0, 1} and blocking > 500


def _foot_candidates(f, fh, mu, lo, hi, free, c0, merged, negated_operand):
    """iterate()'s candidates of one foot.  merged: step_cand_z, otherwise the pair; negated_operand: the directions as -(f - f^),
    otherwise f^ - f"""
    f, fh = np.asarray(f, np.float64), np.asarray(fh, np.float64)
    with np.errstate(all="ignore"):
        d = -(f - fh) if negated_operand else fh - f
        dx, dy, dz = d
        fx, fy, fz = f
        m, md = mu * fz, mu * dz
        xf, yf, zf = free
        c = [_step_cand(xf, m + fx, -dx - md, c0 + 0), _step_cand(xf, m - fx, dx - md, c0 + 1),
             _step_cand(yf, m + fy, -dy - md, c0 + 2), _step_cand(yf, m - fy, dy - md, c0 + 3)]
        if merged:
            c.append(_z_merged(zf, fz - lo, hi - fz, dz, c0 + 4))
        else:
            c += [_step_cand(zf, fz - lo, -dz, c0 + 4), _step_cand(zf, hi - fz, dz, c0 + 5)]
    return c


def _ratio_decisions(amin):
    """what iterate() takes from the reduced ratio: blocked, the face code under `blocked`, beta"""
    a = _val(amin)
    blocked = bool(a < 1.0e299)
    with np.errstate(all="ignore"):
        lo0 = np.fmax(a, 0.0)  # v_max_f64 / v_min_f64 drop a NaN
        beta = np.float64(1.0) - np.fmin(lo0, 1.0)
    return blocked, (amin & 31) if blocked else -1, _bits(beta)


def _feet(rng, n):
    for k in range(n):
        mu = 0.6 if k % 5 else 10.0 ** rng.uniform(-2, 0.3)
        lo, hi = (10.0, 160.0) if k % 3 else (0.0, 30.0)
        fz = rng.uniform(lo, hi) if k % 4 else (lo if k % 8 else hi)
        f = np.array([rng.uniform(-1, 1) * mu * fz, rng.uniform(-1, 1) * mu * fz, fz])
        fh = f + rng.normal(size=3) * 10.0 ** rng.uniform(-15, 2, 3)
        for j in range(3):  # components that do not move, zeros of either sign
            r = rng.random()
            if r < 0.15:
                fh[j] = f[j]
            elif r < 0.2:
                f[j], fh[j] = (0.0, -0.0) if rng.random() < 0.5 else (-0.0, -0.0)
        free = tuple(bool(rng.random() < 0.7) for _ in range(3))
        yield f, fh, mu, lo, hi, free, 6 * (k % 4)


def test_five_candidates_from_the_negated_operand_decide_as_the_six_did():
    rng = np.random.default_rng(0xF00727)
    seen, codes = set(), set()
    for f, fh, mu, lo, hi, free, c0 in _feet(rng, 4000):
        old = _ratio_decisions(_tree(_foot_candidates(f, fh, mu, lo, hi, free, c0, merged=False, negated_operand=False)))
        new = _ratio_decisions(_tree(_foot_candidates(f, fh, mu, lo, hi, free, c0, merged=True, negated_operand=True)))
        assert old == new, (f, fh, mu, free, old, new)
        seen.add(old[0])
        codes.add(old[1] - c0)
    assert seen == {True, False} and codes >= {0, 1, 2, 3, 4, 5}


def test_negated_step_operand_is_the_direction_except_for_the_sign_of_a_zero():
    rng = np.random.default_rng(0xA5171)
    vals = list(rng.normal(size=400) * 10.0 ** rng.uniform(-300, 300, 400)) + [0.0, -0.0, 5e-324, -5e-324, 1e-310, np.inf, -np.inf, np.nan, 1.0, -1.0]
    zeros = 0
    with np.errstate(all="ignore"):
        for a, b in itertools.product(vals[:40] + vals[400:], repeat=2):
            a, b = np.float64(a), np.float64(b)
            d, e = b - a, a - b
            if np.isnan(d):
                assert np.isnan(e)  # (its sign bit is not looked at: a NaN direction blocks nowhere)
            elif d == 0.0:
                assert e == 0.0  # equal operands: +0 both ways, so -e is -0 - no nd of it passes nd > eps
                zeros += 1
            else:
                assert _bits(-e) == _bits(d), (a, b)
    assert zeros > 40


def test_the_step_keeps_f_minus_fh_because_of_a_negative_zero_target():
    f, fh = np.float64(-0.0), np.float64(-0.0)
    for beta in (np.float64(0.0), np.float64(0.25), np.float64(1.0)):
        kept = beta * (f - fh) + fh        # fma(beta, f - f^, f^): the product is an exact zero, so the sum is the fma
        other = beta * -(fh - f) + fh      # fma(beta, -(f^ - f), f^)
        assert _bits(kept) == _bits(0.0) and _bits(other) == _bits(-0.0)


# ------------------------------------------------------------------------------------------------------------ multiplier test
def _tag(b, code):
    return (b & ~31 & M64) | code


def _big_unless(on, l):
    b = _bits(l)
    return ((b >> 32 if on else BIG_HI) << 32) | (b & 0xFFFFFFFF)


def _multipliers(states, g, mu, thr, new):
    """multipliers_ok over the four feet of a robot (one foot per lane, packed): worst, neg, negbits"""
    cand, neg, negbits = [], [], 0
    with np.errstate(all="ignore"):
        for foot, ((sx, sy, sz), gf) in enumerate(zip(states, g)):
            lx = -np.float64(sx) * gf[0]
            ly = -np.float64(sy) * gf[1]
            lz = np.float64(sz) * (mu * (lx + ly) - gf[2])
            lane = []
            for axis, (s, l) in enumerate(((sx, lx), (sy, ly), (sz, lz))):
                if new:
                    v = _big_unless(s != 0, l)
                    n = bool(_val(v) < thr)
                else:
                    v = _bits(l if s != 0 else BIG)
                    n = (s != 0) and bool(l < thr)
                lane.append(_tag(v, 3 * foot + axis))
                neg.append(n)
                negbits |= ((3 << (2 * axis)) << (6 * foot)) if n else 0
            cand.append(_tree(lane))
    return _tree(cand), neg, negbits  # (group_min: the same minimum whichever order the lanes meet in, NaNs aside)


def _word(states):
    w = 0
    for foot, s in enumerate(states):
        for axis, v in enumerate(s):
            w |= (v & 3) << (6 * foot + 2 * axis)
    return w


def _after_release(states, worst, negbits, thr):
    """iterate() at f = f^: opt, polish, and the working-set word after the release - one field, and the drop-all strategy's"""
    w = _word(states)
    with np.errstate(all="ignore"):
        opt = not bool(_val(worst) < thr)
        polish = (not opt) and bool(np.abs(_val(worst)) <= np.abs(thr))
    rel1 = 0 if opt else (3 << ((((worst & 31) << 1) & 31))) & 0xFFFFFFFF
    return opt, polish, w & ~rel1, w & ~negbits


def test_high_word_select_and_neg_on_the_selected_value_decide_as_before():
    rng = np.random.default_rng(0x3E6)
    mu = 0.6
    all_states = list(itertools.product((-1, 0, 1), repeat=3))
    cases = []
    for k in range(1500):
        states = [all_states[rng.integers(0, 27)] if rng.random() < 0.8 else (0, 0, 0) for _ in range(4)]
        g = rng.normal(size=(4, 3)) * 10.0 ** rng.uniform(-12, 2, (4, 3))
        thr = np.float64(10.0 ** rng.uniform(-12, -4)) * (1.0 if k % 2 else -1.0)
        if k % 4 == 0:  # a multiplier within a few ulps of the bar, on either side and on it
            foot, axis = rng.integers(0, 4), rng.integers(0, 2)
            s = states[foot][axis] or 1
            st = list(states[foot]); st[axis] = s; states[foot] = tuple(st)
            t = thr
            for _ in range(abs(k // 4 % 7 - 3)):
                t = np.nextafter(t, np.inf if k // 4 % 7 > 3 else -np.inf)
            g[foot, axis] = -t / s
        if k % 11 == 0:
            g[rng.integers(0, 4), rng.integers(0, 3)] = np.nan  # on whatever face is there, active or not
        if k % 13 == 0:
            g[rng.integers(0, 4), rng.integers(0, 3)] = np.inf
        cases.append((states, g, thr))
    for states, g, thr in list(cases[:200]):
        cases.append((states, g, np.float64(np.nan)))
        cases.append((states, g, np.float64(np.inf)))
    cases.append(([(0, 0, 0)] * 4, rng.normal(size=(4, 3)), np.float64(1e-9)))  # nothing active
    cases.append(([(0, 0, 0)] * 4, np.full((4, 3), np.nan), np.float64(-1e-9)))
    seen_opt, seen_polish, seen_neg = set(), set(), set()
    for states, g, thr in cases:
        wo, nego, nbo = _multipliers(states, g, mu, thr, new=False)
        wn, negn, nbn = _multipliers(states, g, mu, thr, new=True)
        old, new = _after_release(states, wo, nbo, thr), _after_release(states, wn, nbn, thr)
        assert old == new, (states, g, thr, old, new)
        if not np.isposinf(thr):
            assert nego == negn and nbo == nbn, (states, g, thr)
            assert _same_to_every_reader(wo, wn)
            if not old[0]:
                assert wo == wn  # read past `opt` (face code, release mask, polish): the winner is an active face, bit for bit
        seen_opt.add(old[0]); seen_polish.add(old[1]); seen_neg.add(any(nego))
    assert seen_opt == {True, False} and seen_polish == {True, False} and seen_neg == {True, False}


def test_neg_must_not_be_taken_from_the_tagged_value():
    """why the compare reads the selected value and not the candidate: the tag moves the low five bits across the bar"""
    thr = _val(_bits(-1e-9) | 16)
    l = _val(_bits(thr) + 3)  # a little below the bar (negative values: more bits = further down)
    assert bool(l < thr)
    assert not bool(_val(_tag(_bits(l), 2)) < thr)
