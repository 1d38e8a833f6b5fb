"""-m gpu: the commander step of qc_tick_batch (commander_step, qc_balance.hip) at a few ulps and on its edges.

The closed-loop tests (tests/test_gpu_commander.py) hold the step to a float64 restatement at a flat 1e-12 with twists that keep
the increment angle inside (0, 1e-4).  Here ONE launch over robots that are all standing, running and holding a command leaves
the desired state in the qc_commander_state records, and every entry is held to the reference's formulas evaluated at 50 digits
(tests/device_math_reference.commander_apply_mp; long double on the bulk of the random sweep) with the bar

    |device - reference| <= count * EPS * condition sum

where the condition sum is sum |terms| of the expression that produces the entry and `count` the number of roundings on its
longest chain, both carried through the reference's own arithmetic (device_math_reference.Tr).  (The count of the longest chain
is applied to every term of an entry: for x_d = x + Rz tbb' the bar is 30 EPS (|x| + ...), so the robots with |x| near 1e6 m pin the
adjoint - xdot_d = R^T (v - x x w), where the large products are the terms - and not the translation; the translation is pinned by
the robots with small |x|, which the log-uniform draw keeps in the majority, and bit for bit by the edge sets.)  The counts (derived, not tuned;
test_commander_cpu pins them and shows that a plain double evaluation of the same formulas stays inside the bar):
  delta = w dt 1; |delta|^2 5; angle = sqrt 4; axis = delta / angle 6 (the division one rounding); sin, cos: sincos_joint's pinned
  2 EPS absolute plus the angle's own 4 roundings through |d sin| <= |d angle| - condition 1 + angle, count 4; 1 - cos 5;
  (1 - cos) a_i a_j 19; Rbb' 20; cy = R00 / h 3 (h^2 2, h 2, the division 1); Rwb_d rows 0 and 1: 25, row 2: 20;
  tbb' = (Rbb' v) dt 24; x_d = x + (cy t0 - sy t1): 30; almost-zero angle: Rwb_d 5, x_d 7; xdot_d = R^T (v - x x w): 6; w_d: 3.
Every lane layout of commander_support.CASES runs the same robots and must leave the same bits."""
import functools

import numpy as np
import pytest

from tests import device_math_reference as R
from tests.commander_support import CASES, DESIRED, MEAS, _base, _check_instantiation, _controller, _state_host, _to_dev
from tests.gpu_arrays import q  # noqa: F401

pytestmark = pytest.mark.gpu
EPS = R.EPS
FIELDS = ("Rwb_d", "x_d", "xdot_d", "w_d")
QC_SOLVED, QC_NOT_PD = 0, 3


@functools.lru_cache(maxsize=None)
def _cached_base(n):
    return _base(n)


def _tile(a, n):
    a = np.asarray(a)
    reps = -(-n // a.shape[0])
    return np.ascontiguousarray(np.concatenate([a] * reps, 0)[:n])


def _tick(q, ctl, n, st, Rwb, x, twist=None, fresh=None, carry=None, **scalars):
    """One qc_tick_batch over n robots: records `st` (host array [m], tiled to n), measured Rwb [m, 9] and x [m, 3] (tiled), the
    other measurements from the planned workload.  Returns (records [n], status [n], phase [n, 4], swing [n], carry)."""
    import torch

    base = _cached_base(n)
    if carry is None:
        carry = dict(phase=_to_dev(base["gait_phase"]), swing=_to_dev(q.new_swing_states(n).view(np.uint8)), dt=_to_dev(np.full(n, 1.0 / 300.0)),
                     meas={k: _to_dev(base[k]) for k in MEAS if k not in ("Rwb", "x")})
    d_state = _to_dev(_tile(st, n).view(np.uint8))
    command = dict(state=d_state, **scalars)
    if fresh is not None:
        command.update(twist=_to_dev(_tile(twist, n)), fresh=_to_dev(_tile(fresh, n).astype(np.uint8)))
    batch = dict(carry["meas"], Rwb=_to_dev(_tile(Rwb, n)), x=_to_dev(_tile(x, n)), gait_phase=carry["phase"], gait_dt=carry["dt"], swing_state=carry["swing"])
    out = ctl.tick_batch(batch, command)
    torch.cuda.synchronize()
    return (_state_host(q, d_state).copy(), out["status"].cpu().numpy(), carry["phase"].cpu().numpy(), carry["swing"].cpu().numpy().view(q.SWING_STATE_DTYPE).copy(),
            carry)


def _layouts(q):
    for case, (n, tune, lanes, mode, _) in CASES.items():
        _, ctl = _controller(q, tune)
        _check_instantiation(ctl, n, lanes, mode, case)
        yield case, n, ctl


def _applied_states(q, m, Vb):
    s = q.new_commander_states(m)
    s["standing"] = s["gait_running"] = s["cmd_pending"] = 1
    s["Vb"] = Vb
    return s


def _same_bits(a, b):
    return a.tobytes() == b.tobytes()


def _run_all_layouts(q, st, Rwb, x, **kw):
    """The same m robots on every lane layout: tiled to the layout's batch size where it is larger (every copy of a robot must hold
    the bits of the first - its step ran once, whatever wave, lane group or slot it sat in), in consecutive launches where it is
    smaller.  The layouts must leave the same bits in every field of every record.  Returns (records [m], status [m] of the first)."""
    m = st.shape[0]
    first = None
    for case, n, ctl in _layouts(q):
        rec_m, status_m = np.empty(m, st.dtype), np.empty(m, np.int32)
        for lo in range(0, m, n):
            idx = (lo + np.arange(n)) % m
            rec, status, _, _, _ = _tick(q, ctl, n, st[idx], Rwb[idx], x[idx], **kw)
            k = min(n, m - lo)
            rec_m[lo:lo + k], status_m[lo:lo + k] = rec[:k], status[:k]
            for t in range(m, n, m):
                kk = min(m, n - t)
                assert _same_bits(rec[t:t + kk], rec[:kk]), (case, t, [f for f in rec.dtype.names if not _same_bits(rec[f][t:t + kk], rec[f][:kk])])
        if first is None:
            first = (rec_m, status_m)
        else:
            assert _same_bits(rec_m, first[0]), (case, [f for f in rec_m.dtype.names if not _same_bits(rec_m[f], first[0][f])])
    return first


def _rot(yaw, pitch, roll):
    from scipy.spatial.transform import Rotation

    return Rotation.from_euler("ZYX", np.stack([yaw, pitch, roll], -1)).as_matrix().reshape(-1, 9)


def _sweep(rng, m, dt):
    """|w| |dt| log-uniform over [1e-14, pi] (80 %) and on to 50 rad; |v| up to 10 m/s; yaw on the circle, roll / pitch up to 1.5 rad;
    |x| log-uniform up to 1e6 m"""
    ang = np.where(rng.uniform(size=m) < 0.8, np.exp(rng.uniform(np.log(1e-14), np.log(np.pi), m)), rng.uniform(np.pi, 50.0, m))
    ax = rng.normal(size=(m, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ax[::7] = np.eye(3)[rng.integers(0, 3, ax[::7].shape[0])] * rng.choice([-1.0, 1.0], (ax[::7].shape[0], 1))  # coordinate axes: exact zeros in delta
    w = ax * (ang / abs(dt))[:, None]
    v = rng.normal(size=(m, 3))
    v *= (rng.uniform(0, 10.0, m) / np.linalg.norm(v, axis=1))[:, None]
    x = rng.normal(size=(m, 3))
    x *= (np.exp(rng.uniform(np.log(1e-3), np.log(1e6), m)) / np.linalg.norm(x, axis=1))[:, None]
    Rw = _rot(rng.uniform(-np.pi, np.pi, m), rng.uniform(-1.5, 1.5, m), rng.uniform(-1.5, 1.5, m))
    return Rw, x, np.concatenate([v, w], 1)


def _worst(rec, ref, sel=slice(None)):
    """max over fields and entries of |device - reference| / (count EPS condition sum); an exact reference entry (condition 0 or
    count 0) must be met exactly"""
    worst = {}
    for k in FIELDS:
        val, cond, cnt = ref[k]
        got = rec[k][sel]
        err = np.abs(got.astype(np.longdouble) - val)
        bar = cnt * EPS * cond
        exact = bar == 0
        assert np.array_equal(got[exact], np.asarray(val, np.float64)[exact]), k
        worst[k] = float(np.max(np.where(exact, 0.0, err / np.where(exact, 1.0, bar)), initial=0.0))
    return worst


@pytest.mark.parametrize("cmd_dt", [1e-3, 0.5, -0.25])
def test_commander_step_within_a_few_ulps(q, cmd_dt):
    """20 480 random robots over the whole range of the step (see _sweep) on every lane layout, the default cmd_dt, a large one and
    a NEGATIVE one (the validation accepts any finite cmd_dt; the formulas do not care: delta = w dt, angle = |delta|, the
    increment runs backwards - DESIGN.md section 5).  Bars: the module docstring's.  Long double on all robots, 50 digits on
    2 000 of them."""
    m = 20480
    rng = np.random.default_rng(0xED6E + int(abs(cmd_dt) * 1000))
    Rw, x, Vb = _sweep(rng, m, cmd_dt)
    rec, status = _run_all_layouts(q, _applied_states(q, m, Vb), Rw, x, cmd_dt=cmd_dt)
    assert (rec["cmd_pending"] == 0).all() and (rec["standing"] == 1).all() and (rec["gait_running"] == 1).all() and np.array_equal(rec["Vb"], Vb)
    ref = R.commander_apply_ld(Rw, x, Vb, cmd_dt, 0.26)
    assert ref["yaw_ok"].all() and (~ref["small"]).sum() > 15000 and ref["small"].sum() > 500
    worst = _worst(rec, ref)
    print(f"cmd_dt {cmd_dt}: worst error / bar over {m} robots (long double): {worst}")
    assert max(worst.values()) <= 1.0, worst
    sub = rng.choice(m, 2000, replace=False)
    worst_mp = dict.fromkeys(FIELDS, 0.0)
    for i in sub:
        o = R.commander_apply_mp(Rw[i], x[i], Vb[i], cmd_dt, 0.26)
        for k, v in _worst(rec, o, int(i)).items():
            worst_mp[k] = max(worst_mp[k], v)
    print(f"cmd_dt {cmd_dt}: worst error / bar over 2000 robots (50 digits): {worst_mp}")
    assert max(worst_mp.values()) <= 1.0, worst_mp


def test_zero_command_step(q):
    """cmd_dt = 0.0 and -0.0 with a twist that is anything but zero (random v up to 10 m/s, w up to 100 rad/s, yaw on the circle, tilted
    poses, one pose without a yaw), on every lane layout: delta = w * 0 = +-0, so the small-angle branch is taken and the reference's
    result is exact - Rwb_d = Rz(yaw) entry for entry (c = R00 / h, s = R10 / h, the zeros and the 1 exact), x_d(0:1) = x(0:1) bit for
    bit (the increment is +-0), x_d(2) = the stand height, the command consumed.  xdot_d and w_d do not read cmd_dt: bars as ever."""
    m = 256
    rng = np.random.default_rng(0xD70)
    Rw = _rot(rng.uniform(-np.pi, np.pi, m), rng.uniform(-1.5, 1.5, m), rng.uniform(-1.5, 1.5, m))
    Rw[7] = [0.0, 0.0, 1.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.0]
    x = rng.normal(size=(m, 3)) * np.exp(rng.uniform(np.log(1e-3), np.log(1e4), (m, 1)))
    Vb = np.concatenate([rng.uniform(-10, 10, (m, 3)), rng.uniform(-100, 100, (m, 3))], 1)
    for dt in (0.0, -0.0):
        rec, status = _run_all_layouts(q, _applied_states(q, m, Vb), Rw, x, cmd_dt=dt)
        assert (rec["cmd_pending"] == 0).all() and np.array_equal(rec["Vb"], Vb)
        h = np.sqrt(Rw[:, 0] * Rw[:, 0] + Rw[:, 3] * Rw[:, 3])
        c, s = Rw[:, 0] / np.where(h > 0, h, 1.0), Rw[:, 3] / np.where(h > 0, h, 1.0)
        c[h == 0], s[h == 0] = 1.0, 0.0
        z, o = np.zeros(m), np.ones(m)
        Rz = np.stack([c, -s, z, s, c, z, z, z, o], 1)
        got = rec["Rwb_d"]
        for k in (2, 5, 6, 7, 8):
            assert np.array_equal(got[:, k], Rz[:, k]), k
        # c and s: one division of exact inputs by h, h within 2 roundings (count 3 in the reference's terms); the device's own h may
        # sit an ulp from numpy's, so the non-trivial entries are held to the reference's bar, the pattern (c, -s; s, c) bit for bit
        assert np.array_equal(got[:, 0], got[:, 4]) and np.array_equal(got[:, 1], -got[:, 3])
        assert np.array_equal(rec["x_d"][:, :2], x[:, :2]) and (rec["x_d"][:, 2] == 0.26).all(), dt
        ref = R.commander_apply_ld(Rw, x, Vb, dt, 0.26)
        assert ref["small"].all() and (~ref["yaw_ok"]).sum() == 1
        assert np.array_equal(got[7], np.eye(3).reshape(9))
        worst = _worst(rec, ref)
        assert max(worst.values()) <= 1.0, (dt, worst)


def _edge(x, Vb, Rw=None):
    return (np.eye(3).reshape(9) if Rw is None else np.asarray(Rw, float).reshape(9)), np.asarray(x, float), np.asarray(Vb, float)


def test_increment_angle_edges(q):
    """|w| dt = 0, -0, 9.9e-13, the last double below 1e-12, 1e-12 itself, the next one, 1e-9 and 1e-8 (where 1 - cos rounds to 0),
    about each coordinate axis, with cmd_dt = 2^-10 (so w dt is exact) and x = (0, 0, z), yaw 0.  Below the threshold the reference's
    result is exact: Rwb_d = I and x_d - x = v dt UNROTATED, bit for bit.  From it on: the 50-digit reference within the bars, and
    the translation is rotated (x_d differs from v dt where the rotation moves it by more than an ulp)."""
    dt = 2.0 ** -10
    v = np.array([3.0, -5.0, 7.0])
    rows, small = [], []
    for ang, sm in ((0.0, True), (-0.0, True), (9.9e-13, True), (np.nextafter(1e-12, 0), True), (1e-12, False), (np.nextafter(1e-12, 1), False), (1e-9, False), (1e-8, False)):
        for axis in range(3):
            w = np.zeros(3)
            w[axis] = ang / dt
            assert w[axis] * dt == ang
            rows.append(_edge([0.0, 0.0, 0.31], np.concatenate([v, w])))
            small.append(sm)
    Rw, x, Vb = (np.array(c) for c in zip(*rows))
    rec, _ = _run_all_layouts(q, _applied_states(q, len(rows), Vb), Rw, x, cmd_dt=dt)
    small = np.array(small)
    assert (rec["cmd_pending"] == 0).all()
    for i in np.nonzero(small)[0]:
        assert np.array_equal(rec["Rwb_d"][i], np.eye(3).reshape(9)), (i, rec["Rwb_d"][i])
        assert np.array_equal(rec["x_d"][i], [v[0] * dt, v[1] * dt, 0.26]), (i, rec["x_d"][i])
    for i in range(len(rows)):
        o = R.commander_apply_mp(Rw[i], x[i], Vb[i], dt, 0.26)
        assert o["small"] == small[i]
        worst = _worst(rec, o, int(i))
        assert max(worst.values()) <= 1.0, (i, worst)
    for i in np.nonzero(~small)[0]:  # Rbb' is not the identity: its sine shows, and so does the rotated translation at 1e-9 and 1e-8
        ang = np.linalg.norm(Vb[i, 3:]) * dt
        assert np.abs(rec["Rwb_d"][i]).reshape(3, 3)[~np.eye(3, dtype=bool)].max() == np.sin(ang), i
        if ang >= 1e-9:
            assert not np.array_equal(rec["x_d"][i, :2], [v[0] * dt, v[1] * dt]), i


def test_yaw_extraction_edges(q):
    """Yaw 0, +-pi/2, pi built with exact zeros and +-1 in R00 / R10: Rz(yaw) must be exact (a signed permutation), in every
    quadrant.  No yaw to extract - R00 = R10 = 0 (pitch = +-pi/2), |R00|, |R10| = 1e-163 (their squares underflow to 0), a NaN or an
    Inf in R00 or R10: yaw 0 is taken, as INTEGRATION.md says, the rest of the record is what the formulas give with Rz = I (xdot_d, w_d
    read Rwb itself: NaN where the non-finite entry reaches them, and only there).  |R00|, |R10| = 1e-160: h^2 is subnormal with 12
    significant bits, so Rz is a rotation to 2^-10 only."""
    dt = 1e-3
    Vb = np.array([0.5, -0.25, 0.125, 0.0, 0.0, 40.0])  # a yaw increment of 0.04 rad
    x0 = [0.0, 0.0, 0.3]
    cases = []
    for c, s in ((1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (-1.0, 0.0), (-1.0, -0.0)):
        cases.append(("quadrant", np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]), (c, s)))
    for sgn in (1.0, -1.0):
        cases.append(("lock", np.array([[0.0, 0.0, sgn], [0.0, 1.0, 0.0], [-sgn, 0.0, 0.0]]), (1.0, 0.0)))
    for r00, r10 in ((1e-163, -1e-163), (np.nan, 0.5), (0.5, np.nan), (np.inf, 0.0), (0.25, -np.inf)):
        M = np.array([[r00, 0.0, 1.0], [r10, 1.0, 0.0], [-1.0, 0.0, 0.0]])
        cases.append(("lock", M, (1.0, 0.0)))
    cases.append(("subnormal", np.array([[1e-160, 0.0, 1.0], [1e-160, 1.0, 0.0], [-1.0, 0.0, 0.0]]), None))
    Rw = np.array([c[1].reshape(9) for c in cases])
    m = len(cases)
    rec, status = _run_all_layouts(q, _applied_states(q, m, np.tile(Vb, (m, 1))), Rw, np.tile(x0, (m, 1)), cmd_dt=dt)
    Rb = R.commander_apply_mp(np.eye(3), x0, Vb, dt, 0.26)  # yaw 0: Rwb_d = Rbb', x_d = tbb'
    for i, (kind, M, cs) in enumerate(cases):
        got = rec["Rwb_d"][i].reshape(3, 3)
        if kind == "subnormal":
            Rz = got @ np.linalg.inv(Rb["Rwb_d"][0].reshape(3, 3))
            assert np.isfinite(got).all() and abs(np.linalg.det(Rz) - 1.0) < 2.0 ** -10 and abs(Rz[0, 0] - np.sqrt(0.5)) < 2.0 ** -10 and abs(Rz[2, 2] - 1.0) < 1e-12
            continue
        o = R.commander_apply_mp(M, x0, Vb, dt, 0.26)
        assert o["yaw_ok"] == (kind == "quadrant")
        if kind == "lock":
            assert np.array_equal(rec["Rwb_d"][i], rec["Rwb_d"][0]) and np.array_equal(rec["x_d"][i], rec["x_d"][0]), (i, M)
        else:  # Rz is an exact signed permutation: the device's entries are Rbb' entries moved and negated, bit for bit
            c, s = cs
            want = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ rec["Rwb_d"][0].reshape(3, 3)
            assert np.array_equal(got, want), (i, got, want)
        fin = np.isfinite(M).all()
        assert (status[i] == QC_NOT_PD) == (not fin), (i, status[i])
        if fin:
            assert max(_worst(rec, o, int(i)).values()) <= 1.0, i
        else:  # xdot_d = Rwb^T u, w_d = Rwb^T w: entry 0 reads column 0 of Rwb, where the non-finite value sits - and only entry 0
            for k in ("xdot_d", "w_d"):
                val, cond, cnt = o[k]
                assert not np.isfinite(rec[k][i, 0]), (i, k)
                assert np.all(np.abs(rec[k][i, 1:] - val[1:]) <= (cnt * EPS * cond)[1:]), (i, k)


def _latch_expected(z, h, tol):
    with np.errstate(invalid="ignore"):
        return (np.abs(z - h) < tol).astype(np.int32)  # the reference's almost_equal in double (commander_node.cpp:386-391)


@pytest.mark.parametrize("h,tol", [(0.26, 0.005), (0.3, 0.017), (0.26, 0.0)])
def test_stand_latch_edges(q, h, tol):
    """Heights at h +- tol, a few ulps inside and outside, for the defaults, for a pair whose h + tol is not representable, and
    for stand_tol = 0 (never latches, not even at x2 == h): the flag is the double expression fabs(x2 - h) < tol, strictly.  NaN and
    +-Inf heights never latch a robot that is not standing; a standing, running robot keeps running on them (its flags do not move,
    its tick reports the non-finite input)."""
    zs = []
    for edge in (h + tol, h - tol):
        z = edge
        walk = [z]
        up = dn = z
        for _ in range(3):
            up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
            walk += [up, dn]
        zs += walk
    zs += [h, np.nextafter(h, 1), np.nextafter(h, 0), h + 0.5 * tol, h - 0.999 * tol, h + 2 * tol + 1e-3, 0.0, np.nan, np.inf, -np.inf]
    zs = np.array(zs)
    m = 2 * len(zs)
    z2 = np.concatenate([zs, zs])
    st = q.new_commander_states(m, x_stand=(0.0, 0.0, h))
    st["standing"][len(zs):] = 1  # second half: already standing and running
    st["gait_running"][len(zs):] = 1
    x = np.stack([np.zeros(m), np.zeros(m), z2], 1)
    for case, n, ctl in _layouts(q):
        rec, status, phase, swing, carry = _tick(q, ctl, n, st, np.tile(np.eye(3).reshape(9), (m, 1)), x, stand_height=h, stand_tol=tol)
        base = _cached_base(n)
        for lo in range(0, n - m + 1, max(m, (n // m // 3) * m)):
            r = rec[lo:lo + m]
            want = _latch_expected(zs, h, tol)
            assert np.array_equal(r["standing"][:len(zs)], want), (case, lo, zs[r["standing"][:len(zs)] != want])
            assert np.array_equal(r["gait_running"][:len(zs)], want), case  # the tick it stands up is the tick its gait starts ...
            assert np.array_equal(phase[lo:lo + len(zs)], base["gait_phase"][lo:lo + len(zs)]), case  # ... and no clock moves on either
            assert (r["standing"][len(zs):] == 1).all() and (r["gait_running"][len(zs):] == 1).all(), case
            assert (phase[lo + len(zs):lo + m] != base["gait_phase"][lo + len(zs):lo + m]).any(axis=1).all(), case  # running robots ran
            bad = ~np.isfinite(z2)
            assert (status[lo:lo + m][bad] == QC_NOT_PD).all() and (status[lo:lo + m][~bad] != QC_NOT_PD).all(), (case, status[lo:lo + m])
            for k in DESIRED:
                assert _same_bits(r[k], st[k]), (case, k)
        if tol == 0.0:
            assert (rec["standing"][:len(zs)] == 0).all()
    want = _latch_expected(zs, h, tol)
    if tol > 0:
        assert want.sum() >= 8 and (want == 0).sum() >= 8  # both sides of both edges are in the set


def test_command_life_cycle(q):
    """One robot's commander over consecutive ticks on every lane layout (the other robots of the batch are copies), hand-checked as
    tests/test_commander_cpu.py::test_command_held_until_the_gait_runs: a fresh command before standing is held; a second one
    replaces it; the stand-up tick starts the gait and applies nothing (phases held, all-stance, planner state untouched); the first
    running tick applies the command; a tick with fresh = 0 and junk in `twist` moves nothing; fresh = 2 and 255 count as fresh."""
    tw1 = np.array([[0.2, 0.05, 0.0, 0.01, 0.0, 0.04]])
    tw2 = np.array([[-0.3, 0.1, 0.0, 0.0, 0.02, -0.5]])
    junk = np.full((1, 6), 7.0)
    low, stand = np.array([[0.0, 0.0, 0.20]]), np.array([[0.01, 0.02, 0.258]])
    I = np.eye(3).reshape(1, 9)
    for case, n, ctl in _layouts(q):
        base = _cached_base(n)
        swing0 = q.new_swing_states(n)
        st = q.new_commander_states(1)
        init = st.copy()
        # tick 0: held
        rec, status, phase, swing, carry = _tick(q, ctl, n, st, I, low, tw1, np.array([1]))
        assert (rec["standing"] == 0).all() and (rec["gait_running"] == 0).all() and (rec["cmd_pending"] == 1).all() and (rec["Vb"] == tw1).all(), case
        assert all(_same_bits(rec[k], _tile(init[k], n)) for k in DESIRED)
        # tick 1: a second command (fresh = 255) replaces the first
        rec, *_ = _tick(q, ctl, n, rec[:1], I, low, tw2, np.array([255]), carry)
        assert (rec["cmd_pending"] == 1).all() and (rec["Vb"] == tw2).all() and (rec["standing"] == 0).all(), case
        # tick 2: the stand height is reached: standing, the gait starts, nothing else
        rec, status, phase, swing, _ = _tick(q, ctl, n, rec[:1], I, stand, junk, np.array([0]), carry)
        assert (rec["standing"] == 1).all() and (rec["gait_running"] == 1).all() and (rec["cmd_pending"] == 1).all() and (rec["Vb"] == tw2).all(), case
        assert all(_same_bits(rec[k], _tile(init[k], n)) for k in DESIRED)
        assert np.array_equal(phase, base["gait_phase"]) and _same_bits(swing, swing0), case
        # tick 3: the gait runs and the held command becomes the desired state
        rec, status, phase, swing, _ = _tick(q, ctl, n, rec[:1], I, stand, junk, np.array([0]), carry)
        assert (rec["cmd_pending"] == 0).all() and (rec["Vb"] == tw2).all(), case
        o = R.commander_apply_mp(I[0], stand[0], tw2[0], 1e-3, 0.26)
        assert max(_worst(rec, o, 0).values()) <= 1.0 and rec["x_d"][0, 2] == 0.26, case
        assert _same_bits(rec[1:], rec[:-1]) and (phase != base["gait_phase"]).any(axis=1).all(), case
        assert (swing["leg_state"] >= 0).all(), case  # the planner ran: its state is no longer "nothing yet"
        # tick 4: fresh = 0 with junk behind it: nothing moves
        keep = rec.copy()
        rec, *_ = _tick(q, ctl, n, rec[:1], I, stand + 0.001, junk, np.array([0]), carry)
        assert _same_bits(rec, keep), case
        # tick 5: fresh = 2 is a command: applied in the same tick, since the gait runs
        rec, *_ = _tick(q, ctl, n, rec[:1], I, stand, tw1, np.array([2]), carry)
        assert (rec["cmd_pending"] == 0).all() and (rec["Vb"] == tw1).all(), case
        o = R.commander_apply_mp(I[0], stand[0], tw1[0], 1e-3, 0.26)
        assert max(_worst(rec, o, 0).values()) <= 1.0, case


def test_a_poisoned_robot_stays_alone(q):
    """A NaN twist on one robot in the middle of a wave (and an Inf on another): its record holds what the reference's arithmetic
    gives - NaN wherever the poisoned component reaches, x_d(2) = the stand height, cmd_pending back to 0 - its status is the tick's
    non-finite-input status - on that tick and on every later tick without a new command - and EVERY OTHER robot of the batch, records, forces, torques, clock and planner state, is bit-identical
    to the same launch without the poison (on the racing and MFMA layouts every lane takes part in every reduction).  A later fresh
    finite command restores the robot."""
    import torch

    for case, n, ctl in _layouts(q):
        base = _cached_base(n)
        rng = np.random.default_rng(77)
        x = base["x"].copy()
        x[:, 2] = 0.26 + rng.uniform(-0.004, 0.004, n)
        Vb = rng.uniform(-0.05, 0.05, (n, 6))
        victims = {min(n - 1, 37): np.nan, min(n - 2, n // 2 + 5): np.inf}
        res = {}
        for poisoned in (False, True):
            V = Vb.copy()
            if poisoned:
                for i, bad in victims.items():
                    V[i, 5 if np.isnan(bad) else 0] = bad
            carry = dict(phase=_to_dev(base["gait_phase"]), swing=_to_dev(q.new_swing_states(n).view(np.uint8)), dt=_to_dev(np.full(n, 1.0 / 300.0)),
                         meas={k: _to_dev(base[k]) for k in MEAS if k not in ("Rwb", "x")})
            d_state = _to_dev(_applied_states(q, n, np.zeros((n, 6))).view(np.uint8))
            batch = dict(carry["meas"], Rwb=_to_dev(base["Rwb"]), x=_to_dev(x), gait_phase=carry["phase"], gait_dt=carry["dt"], swing_state=carry["swing"])
            out = ctl.tick_batch(batch, dict(state=d_state, twist=_to_dev(V), fresh=_to_dev(np.ones(n, np.uint8))))
            torch.cuda.synchronize()
            res[poisoned] = dict(rec=_state_host(q, d_state).copy(), phase=carry["phase"].cpu().numpy(), swing=carry["swing"].cpu().numpy().view(q.SWING_STATE_DTYPE).copy(),
                                 **{k: v.cpu().numpy() for k, v in out.items()}, d_state=d_state, carry=carry, batch=batch)
        clean, dirty = res[False], res[True]
        others = np.ones(n, bool)
        others[list(victims)] = False
        for k in ("rec", "phase", "swing", "grf_body", "joint_tau", "status"):
            assert _same_bits(np.ascontiguousarray(clean[k][others]), np.ascontiguousarray(dirty[k][others])), (case, k)
        for i, bad in victims.items():
            r = dirty["rec"][i]
            assert dirty["status"][i] == QC_NOT_PD and clean["status"][i] != QC_NOT_PD, (case, i)
            assert r["cmd_pending"] == 0 and r["x_d"][2] == 0.26 and r["standing"] == 1 and r["gait_running"] == 1
            if np.isnan(bad):  # w_z = NaN: the angle, Rbb', tbb' are NaN; xdot_d = R^T (v - x x w) and w_d = R^T w too (R is full)
                assert np.isnan(r["Rwb_d"]).all() and np.isnan(r["x_d"][:2]).all() and np.isnan(r["xdot_d"]).all() and np.isnan(r["w_d"]).all(), (case, r)
            else:  # v_x = Inf: the rotation is finite and right, the translation and R^T v are not
                assert np.array_equal(r["Rwb_d"], clean["rec"][i]["Rwb_d"]) and np.array_equal(r["w_d"], clean["rec"][i]["w_d"]), (case, r)
                assert not np.isfinite(r["x_d"][:2]).any() and not np.isfinite(r["xdot_d"]).any(), (case, r)
        # ticks in between, no new command: the poisoned robots keep their non-finite desired state untouched, keep running (their
        # clocks advance) and keep reporting the non-finite input; nobody else turns bad
        for _ in range(2):
            before, ph0 = _state_host(q, dirty["d_state"]).copy(), dirty["carry"]["phase"].cpu().numpy()
            out = ctl.tick_batch(dirty["batch"], dict(state=dirty["d_state"], twist=_to_dev(Vb), fresh=_to_dev(np.zeros(n, np.uint8))))
            torch.cuda.synchronize()
            assert _same_bits(_state_host(q, dirty["d_state"]), before), case
            st, ph1 = out["status"].cpu().numpy(), dirty["carry"]["phase"].cpu().numpy()
            assert (st[list(victims)] == QC_NOT_PD).all() and (st[others] != QC_NOT_PD).all(), case
            assert (ph1[list(victims)] != ph0[list(victims)]).any(axis=1).all(), case
        # the next tick brings fresh finite commands: the poisoned robots are ordinary robots again
        out = ctl.tick_batch(dirty["batch"], dict(state=dirty["d_state"], twist=_to_dev(Vb), fresh=_to_dev(np.ones(n, np.uint8))))
        torch.cuda.synchronize()
        rec = _state_host(q, dirty["d_state"])
        st = out["status"].cpu().numpy()
        for i in victims:
            assert st[i] != QC_NOT_PD and all(np.isfinite(rec[k][i]).all() for k in FIELDS), (case, i)
            o = R.commander_apply_mp(base["Rwb"][i], x[i], Vb[i], 1e-3, 0.26)
            assert max(_worst(rec, o, int(i)).values()) <= 1.0, (case, i)


def test_increment_beyond_the_sine_range(q):
    """|w| dt >= 2^30 rad: sincos_joint returns NaN there (test_sincos_joint), the reference's std::sin does not.  The documented
    behaviour (commander section): Rwb_d and x_d(0:1) become NaN, x_d(2), xdot_d and w_d are the reference's, the
    command is consumed and the tick reports QC_NOT_PD for that robot until a new command arrives; one ulp below 2^30 the step is
    the reference's within the bars.  (A range reduction for such an increment - 170 000 revolutions in one command step - would
    cost every robot's fill for no robot's benefit.)"""
    dt = 1.0
    below = np.nextafter(2.0 ** 30, 0.0)
    angs = [below, 2.0 ** 30, 2.0 ** 30 * 1.5, 1e12, 1e300]
    m = len(angs)
    Vb = np.array([[0.5, -0.25, 0.125, 0.0, 0.0, a] for a in angs])
    x = np.tile([0.25, -0.5, 0.3], (m, 1))
    Rw = np.tile(_rot(np.array([0.4]), np.array([0.1]), np.array([-0.2])), (m, 1))
    rec, status = _run_all_layouts(q, _applied_states(q, m, Vb), Rw, x, cmd_dt=dt)
    o = R.commander_apply_mp(Rw[0], x[0], Vb[0], dt, 0.26)
    assert max(_worst(rec, o, 0).values()) <= 1.0 and status[0] != QC_NOT_PD
    for i in range(1, m):
        r = rec[i]
        assert np.isnan(r["Rwb_d"]).all() and np.isnan(r["x_d"][:2]).all() and r["x_d"][2] == 0.26 and r["cmd_pending"] == 0, (i, r)
        ow = R.commander_apply_mp(Rw[i], x[i], Vb[i], dt, 0.26)  # (xdot_d and w_d do not go through the sine)
        for k in ("xdot_d", "w_d"):
            val, cond, cnt = ow[k]
            assert np.all(np.abs(r[k] - val) <= cnt * EPS * cond), (i, k)
        assert np.isfinite(r["xdot_d"]).all() and np.isfinite(r["w_d"]).all()
        assert status[i] == QC_NOT_PD, (i, status[i])
