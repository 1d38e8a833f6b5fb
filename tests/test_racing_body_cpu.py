"""No GPU: the arithmetic of the strided 4-lane lanes' recalculation (Lane::kWord / kArith), restated in float64.

* foot_coef_arith against foot_coef<true>: the face coefficients a lane computes by arithmetic on its foot's states -1 / 0 / +1
  (ix, iy: fma(-|d|, iw, iw); fzfix: fma(max(dz, 0), hi, max(-dz, 0) lo)) equal the select forms BIT FOR BIT in all 27 cube
  states of a stance foot and of a swing foot, at several (mu, fzmin, fzmax, w).  iz stays a select in the kernel and is restated as
  one, so it is compared as well.  An fma with a factor in {-1, 0, 1} rounds nothing (the product is exact and the sum is x - x, x + 0
  or 0 + 0), so a float64 multiply-add restates it exactly; the quadratic through the three values of 1 / (1 + mu^2 k) that DESIGN
  7.21 weighed is shown NOT to be exact, which is why the kernel does not use it.
* the working-set word: encode_foot -> the lane's decode (v_bfe_i32 of two bits) is the identity, and the fields a lane reads back
  from a word it wrote at its own place are its own, whatever the other lanes' fields hold; a caller's word with the unused field
  value 2 is cleaned to "free" as dec2 reads it.
"""
import itertools

import numpy as np

STATES = (-1, 0, 1)


def _settings():
    from oracle import numpy_restatement as R

    P = R.cheetah_params(mu=0.6)
    w = float(np.asarray(P["W"], float).reshape(12, 12)[0, 0])
    out = [(float(P["mu"]), float(P["fzmin"]), float(P["fzmax"]), w)]
    # a second friction, a zero and a negative lower bound, weights far from the default's; the last one is the asymmetric model's
    # scale (tests/solved_batch_support.py: W = 1e-5 x U(0.5, 2)) with bounds that are no round numbers
    out += [(0.3, 0.0, 120.0, 1e-7), (1.0, 5.0, 250.0, 3.7e-4), (0.77, -3.25, 1e3 / 3.0, 1.0), (0.6, 10.0 / 3.0, 160.0 * 1.1, 1e-5 * 1.37)]
    return out


def _bits(x):
    return np.float64(x).view(np.uint64)


def _select_form(mu, fzmin, fzmax, w, sx, sy, sz, st):
    inv_w = 1.0 / w
    inv_bz = [1.0 / (w * (1.0 + mu * mu * k)) for k in range(3)]
    fzfix = (fzmax if sz > 0 else (fzmin if sz < 0 else 0.0)) if st else 0.0
    ix = inv_w if (st and sx == 0) else 0.0
    iy = inv_w if (st and sy == 0) else 0.0
    b1 = inv_bz[2] if sy != 0 else inv_bz[1]
    b0 = inv_bz[1] if sy != 0 else inv_bz[0]
    iz = (b1 if sx != 0 else b0) if (st and sz == 0) else 0.0
    return mu * float(sx), mu * float(sy), fzfix, ix, iy, iz


def _fma(a, b, c):
    # exact for the uses below: a in {-1, 0, 1} (or b an exact 0 / 1 switch), so a * b is exact and one rounding remains
    return np.float64(a) * np.float64(b) + np.float64(c)


def _arith_form(mu, fzmin, fzmax, w, sx, sy, sz, st):
    inv_w = 1.0 / w
    inv_bz = [1.0 / (w * (1.0 + mu * mu * k)) for k in range(3)]
    iw, lo, hi = (inv_w, fzmin, fzmax) if st else (0.0, 0.0, 0.0)  # FaceConst
    dx, dy, dz = np.float64(sx), np.float64(sy), np.float64(sz)
    fzfix = _fma(np.maximum(dz, 0.0), hi, np.maximum(-dz, 0.0) * np.float64(lo))
    ix = _fma(-np.abs(dx), iw, iw)
    iy = _fma(-np.abs(dy), iw, iw)
    b1 = inv_bz[2] if sy != 0 else inv_bz[1]
    b0 = inv_bz[1] if sy != 0 else inv_bz[0]
    iz = (b1 if sx != 0 else b0) if (st and sz == 0) else 0.0
    return mu * dx, mu * dy, fzfix, ix, iy, iz


def test_arithmetic_coefficients_equal_the_selects_bit_for_bit():
    n = 0
    for mu, fzmin, fzmax, w in _settings():
        for st in (True, False):
            for sx, sy, sz in itertools.product(STATES, STATES, STATES):
                a = _select_form(mu, fzmin, fzmax, w, sx, sy, sz, st)
                b = _arith_form(mu, fzmin, fzmax, w, sx, sy, sz, st)
                for name, x, y in zip(("mx", "my", "fzfix", "ix", "iy", "iz"), a, b):
                    assert _bits(x) == _bits(y), (name, mu, fzmin, fzmax, w, sx, sy, sz, st, x, y)
                n += 1
    assert n == 27 * 2 * len(_settings())


def test_quadratic_through_three_values_is_not_exact():
    """1 / (1 + mu^2 k) as r0 + k (r1 + k r2) misses at least one of its three values in some setting: not a bit-exact form."""
    miss = 0
    for mu, _, _, _ in _settings():
        r = [1.0 / (1.0 + mu * mu * k) for k in range(3)]
        c2 = 0.5 * (r[2] - 2.0 * r[1] + 1.0)
        c1 = r[1] - 1.0 - c2
        for k in range(3):
            miss += _bits(1.0 + k * (c1 + k * c2)) != _bits(r[k])
    assert miss > 0


def _encode_foot(sx, sy, sz):
    return (sx & 3) | ((sy & 3) << 2) | ((sz & 3) << 4)


def _sbfe2(word, pos):  # v_bfe_i32 of two bits
    v = (word >> pos) & 3
    return v - 4 if v & 2 else v


def _decode_lane(word, foot):
    return tuple(_sbfe2(word, 6 * foot + 2 * a) for a in range(3))


FOOT_STATES = tuple(itertools.product(STATES, STATES, STATES))


def _check_word(feet):
    word = 0
    for k, s in enumerate(feet):
        word |= _encode_foot(*s) << (6 * k)
    assert word < (1 << 24)
    for k, s in enumerate(feet):
        assert _decode_lane(word, k) == s, (feet, k)
        # what a lane carries: its field at its place, foreign fields arbitrary - the read-back and the output mask see only its own
        carried = (_encode_foot(*s) << (6 * k)) | (0xFFFFFF & ~(63 << (6 * k)))
        assert _decode_lane(carried, k) == s
        assert (carried >> (6 * k)) & 63 == _encode_foot(*s)


def test_word_encode_decode_is_the_identity():
    # every single-foot state with the other three feet all free / all at their lower bounds, for each foot ...
    for other in ((0, 0, 0), (-1, -1, -1)):
        for k in range(4):
            for s in FOOT_STATES:
                feet = [other] * 4
                feet[k] = s
                _check_word(feet)
    # ... and all 3^12 four-foot states through the vectorised form of the same two maps
    idx = np.arange(27 ** 4)
    S = np.empty((idx.size, 12), np.int64)
    for c in range(12):
        S[:, c] = (idx // 3 ** c) % 3 - 1
    word = np.zeros(idx.size, np.int64)
    for c in range(12):
        word |= (S[:, c] & 3) << (2 * c)
    for c in range(12):
        v = (word >> (2 * c)) & 3
        assert np.array_equal(np.where(v & 2, v - 4, v), S[:, c]), c
    assert len(np.unique(word)) == idx.size


def test_field_value_two_of_a_callers_word_reads_as_free():
    """load_from_stock keeps a field only if its bit 0 is set: 0 -> 0, 1 -> 1, 3 -> 3 and the unused 2 -> 0, which is how dec2
    reads the word in the lanes that decode to ints."""
    dec2 = {0: 0, 1: 1, 2: 0, 3: -1}
    for fb in range(64):
        b0 = fb & 0x15
        clean = fb & (b0 | (b0 << 1))
        for a in range(3):
            assert _sbfe2(clean, 2 * a) == dec2[(fb >> (2 * a)) & 3], (fb, a)
