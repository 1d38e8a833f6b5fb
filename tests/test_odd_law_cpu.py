"""CPU: the four restatements of the balance QP's derivative kernels (tests/sensitivity_restatement.py,
tests/sensitivity_rotation_restatement.py, tests/sensitivity_params_restatement.py, tests/tangent_restatement.py) OFF the cheetah's
control law - solved_batch_support.odd_law (three distinct gains per axis, six non-zero kff, dense Ib and S, another mass) on
solved_batch_support.odd_states (general w_d, xdot_d and Rwb_d) - where every index of the PD law b(state; gains) is visible:
  a. each restatement against its own 50-digit variant on EVERY robot of the 130-robot placed-force batches;
  b. b_tan and the reverse outputs against central differences (h = 1e-25) of the forward wrench written as tests/kkt_batch.wrench_data
     states it, evaluated at 50 digits - no derivative formula on that side;
  c. the list of index confusions (a gain vector rolled by an axis, two kff swapped, Ib replaced by its diagonal or its transpose):
     bit-invisible at the cheetah's law on config3's states, more than 100 device bars at the odd law - the proof that
     tests/test_gpu_odd_law.py could fail;
  d. the rotation-log branch sweep in forward mode: tangent() against tangent_mp() on every case of RR.branch_sweep.
The 50-digit passes are made once per (law, source) and shared."""
import functools

import mpmath as mp
import numpy as np
import pytest

import quadruped_control_amd as q
from tests import device_math_reference as DMR
from tests import sensitivity_params_restatement as PR
from tests import sensitivity_restatement as SR
from tests import sensitivity_rotation_restatement as RR
from tests import tangent_restatement as TR
from tests.kkt_batch import wrench_data
from tests.kkt_certificate_restatement import distance
from tests.solved_batch_support import EPS, inputs, odd_law, odd_states
from tests.tangent_restatement import C_DOT_ODD, C_TAN_ALL, C_TAN_ODD, dot_gap

N = 130
ODD_SEED = 5  # (the first seed tried: 2c's 90 % holds with it)
KIN = (DMR.HIP.reshape(-1), DMR.LINKS.reshape(-1))


def law(name):
    return q.cheetah_params(mu=0.6) if name == "cheetah" else odd_law()


@functools.lru_cache(maxsize=None)
def batch(name, source):
    b, grf = inputs(N, source)
    return (b if name == "cheetah" else odd_states(b, ODD_SEED)), grf


# ------------------------------------------------------------------ a. against 50 digits, every robot
def _c_tan(name, K):
    P, worst = law(name), {}
    for source in ("feet", "joint_q"):
        b, grf = batch(name, source)
        tans = TR.random_tangents(N, K, 50, joint_q=source != "feet")
        t = TR.tangent(P, b, grf, tans, log_formation=name == "odd")
        assert (t["flags"] == 0).all() and np.abs(t["grf_tan"]).max() > 0
        memo = {}
        for i in range(N):
            for k in range(K):
                ref = TR.tangent_mp(P, b, grf, tans, i, k, t["active"][i], memo=memo)
                for out, sums in (("grf_tan", "grf_sum"), ("b_tan", "b_sum")):
                    d, c = distance(t[out][k, i], ref[out]), t[sums][k, i].reshape(-1)
                    assert np.all(d[c == 0] == 0), (source, i, k, out)
                    if (c > 0).any():
                        worst[source, out] = max(worst.get((source, out), 0.0), float((d[c > 0] / (EPS * c[c > 0])).max()))
    return worst


def test_tangent_restatement_against_50_digits_on_every_robot():
    """test_tangent_cpu.py::test_restatement_against_50_digits' measure on ALL 130 robots, not every eighth (both sources, its two
    directions): the worst is C_TAN_ALL (measured: b_tan 3.06, grf_tan 0.66 from `feet`, 0.77 from joint_q)."""
    worst = _c_tan("cheetah", 2)
    print("C_TAN_ALL measured", worst)
    assert max(worst.values()) <= C_TAN_ALL, worst


def test_tangent_restatement_against_50_digits_at_the_odd_law():
    """The same on odd_states at odd_law, every robot, one direction: the worst here is b_tan 1.14, grf_tan 0.80 / 0.92; C_TAN_ODD, the
    unit of tests/test_gpu_odd_law.py's bar, also covers the one-input-alone draws of the next test."""
    worst = _c_tan("odd", 1)
    print("C_TAN_ODD measured", worst)
    assert max(worst.values()) <= C_TAN_ODD, worst


def test_tangent_restatement_against_50_digits_one_input_alone():
    """tests/test_gpu_odd_law.py::test_tangent_one_input_alone's draws (n = 65, one input with the three unit-axis seeds) for the
    three inputs whose lines are longest - the two rotation tangents, which go through the log's Jacobian, and w_d_tan: with one
    input alone the condition sum holds that input's terms only, nothing covers a line's rounding but its own terms, and the worst
    is larger than with every input at once.  It belongs to C_TAN_ODD (measured: b_tan 1.81 Rwb_d_rot_tan, 1.53 Rwb_rot_tan, 1.44
    w_d_tan; w_tan 1.13 and xdot_d_tan 0.94 measured once, not asserted here).  Two repairs of the reference stand behind these
    figures: ds / dn of the log's Jacobian is formed in long double (sensitivity_rotation_restatement._log_factors; in double
    Rwb_d_rot_tan alone stood at 7.7), and the sums take the Jacobian's own formation (log_formation=True; with |J| it stood at 2.45)."""
    P, n = odd_law(), 65
    b, grf = inputs(n, "feet")
    b = odd_states(b, ODD_SEED)
    memo, worst = {}, {}
    for name in ("Rwb_d_rot_tan", "Rwb_rot_tan", "w_d_tan"):
        tans = {name: np.broadcast_to(np.eye(3)[:, None, :], (3, n, 3)).copy()}
        t = TR.tangent(P, b, grf, tans, log_formation=True)
        for i in range(n):
            for k in range(3):
                ref = TR.tangent_mp(P, b, grf, tans, i, k, t["active"][i], memo=memo)
                for out, sums in (("grf_tan", "grf_sum"), ("b_tan", "b_sum")):
                    d, c = distance(t[out][k, i], ref[out]), t[sums][k, i].reshape(-1)
                    assert np.all(d[c == 0] == 0), (name, i, k, out)
                    if (c > 0).any():
                        worst[name, out] = max(worst.get((name, out), 0.0), float((d[c > 0] / (EPS * c[c > 0])).max()))
    print("C_TAN_ODD measured, one input alone", worst)
    assert max(worst.values()) <= C_TAN_ODD, worst


@pytest.mark.parametrize("source", ["feet", "joint_q"])
def test_reverse_restatements_against_50_digits_at_the_odd_law(source):
    """sensitivity(), rotation_cotangents() and param_cotangents() against their _mp variants on every robot of odd_states at
    odd_law.  Bars: one evaluation's share of the device bars, which do not depend on the law - the adjoint's (16 cond + 32) EPS of
    the output's largest entry (tests/test_gpu_sensitivity.py: each evaluation may be that far from the true value), and half the
    chain-length constants, 80 / 88 EPS `terms` for the 160 / 176 of the rotation cotangents and the parameter rows."""
    P = odd_law()
    b, grf = batch("odd", source)
    kin = KIN if source != "feet" else None
    gbar = np.random.default_rng(2).normal(0.0, 1.0, (N, 12))
    s = SR.sensitivity(P, b, grf, gbar)
    r = RR.rotation_cotangents(P, b, grf, gbar, s["b_bar"], s["feet_bar"])
    p = PR.param_cotangents(P, b, grf, gbar, s["adjoint"])
    assert (s["flags"] == 0).all() and (np.abs(r["qw"]) > 0.95).all()
    c = 80.0 if source == "feet" else 88.0
    worst = dict(adjoint=0.0, rotation=0.0, params=0.0)
    for i in range(N):
        cond = SR.reduced_condition(P, b, s["active"], i)
        ref = SR.sensitivity_mp(P, b, grf, gbar, i, s["active"][i], kin=kin)
        for k in SR.OUTPUTS:
            d, bar = SR.distance(s[k][i], ref[k]), (16 * cond + 32) * EPS * SR.magnitude(ref[k])
            worst["adjoint"] = max(worst["adjoint"], float(d.max() / max(bar, 1e-300)))
            assert np.all(d <= bar), (i, k, float(d.max()), bar)
        ref = RR.rotation_cotangents_mp(P, b, grf, gbar, s["b_bar"], s["feet_bar"], i, kin=kin)
        for k in RR.OUTPUTS:
            d, bar = RR.distance(r[k][i], ref[k]), c * EPS * r["terms"][k][i]
            worst["rotation"] = max(worst["rotation"], float((d / np.maximum(bar, 1e-300)).max()))
            assert np.all(d <= bar), (i, k, float(d.max()))
        ref = PR.param_cotangents_mp(P, b, grf, gbar, s["adjoint"], i, s["active"][i], kin=kin)
        d, bar = PR.distance(p["rows"][i], ref), c * EPS * p["terms"][i]
        worst["params"] = max(worst["params"], float((d / np.maximum(bar, 1e-300)).max()))
        assert np.all(d <= bar), (i, int(np.argmax(d / np.maximum(bar, 1e-300))))
    print(source, "worst error / bar", worst)


def test_dot_product_identity_at_the_odd_law():
    """test_tangent_cpu.py's two identity tests (every input at once, two directions; one input at a time) at the odd law: the worst
    gap is C_DOT_ODD (measured: 0.94 at once; alone 0.61 ... 1.39: w_d_tan 1.39, Rwb_d_rot_tan 1.27)."""
    P = odd_law()
    b, grf = batch("odd", "feet")
    gbar = np.random.default_rng(2).normal(0.0, 1.0, (N, 12))
    s = SR.sensitivity(P, b, grf, gbar)
    r = RR.rotation_cotangents(P, b, grf, gbar, s["b_bar"], s["feet_bar"])
    worst = {}
    tans = TR.random_tangents(N, 2, 1)
    t = TR.tangent(P, b, grf, tans)
    ok = t["flags"] == 0
    assert np.array_equal(t["flags"], s["flags"]) and ok.mean() > 0.9
    worst["all"] = max(float(dot_gap(gbar, t["grf_tan"], s, r, tans, k, t["cond"])[0][ok].max()) for k in range(2))
    for name in TR.TANGENTS:
        if name == "joint_q_tan":
            continue
        tans = TR.random_tangents(N, 1, 4, names=(name,))
        t = TR.tangent(P, b, grf, tans)
        gap, lhs = dot_gap(gbar, t["grf_tan"], s, r, tans, 0, t["cond"])
        assert (np.abs(lhs[ok]) > 0).mean() > 0.75, name
        worst[name] = float(gap[ok].max())
    print("C_DOT_ODD measured", worst)
    assert max(worst.values()) <= C_DOT_ODD, worst


# ------------------------------------------------------------------ b. against central differences of the forward wrench at 50 digits
def _wrench_mp(P, st, case, negative):
    """b [6] as tests/kkt_batch.wrench_data states it, on 50-digit inputs (st: mp matrices R, Rd [3,3], x, x_d, xdot, xdot_d, w, w_d
    [3]); the log on the branch held (RR._log_mp_on_branch)"""
    V = lambda k: mp.matrix([DMR.mpf(float(v)) for v in np.asarray(P[k], float).reshape(-1)])
    kff, kp_p, kd_p, kp_w, kd_w = (V(k) for k in ("kff", "kp_p", "kd_p", "kp_w", "kd_w"))
    m, g = DMR.mpf(float(P["mass"])), DMR.mpf(9.81)
    Ib = mp.matrix(3, 3)
    for j, v in enumerate(V("Ib")):
        Ib[j // 3, j % 3] = v
    a = [kp_p[k] * (st["x_d"][k] - st["x"][k]) + kd_p[k] * (st["xdot_d"][k] - st["xdot"][k]) for k in range(3)]
    a[0] += kff[0] * st["xdot_d"][0]
    a[1] += kff[1] * st["xdot_d"][1]
    a[2] += kff[2] * m * g
    e = RR._log_mp_on_branch(st["Rd"] * st["R"].T, case, negative)
    wd = st["w_d"]
    al = mp.matrix([kp_w[k] * e[k] + kd_w[k] * (wd[k] - st["w"][k]) for k in range(3)])
    al[0] += kff[3] * wd[0]
    al[1] += kff[4] * wd[1] + kff[5] * wd[2]  # sic: index 1
    Iw = st["R"] * Ib * st["R"].T
    Iwd = Iw * wd
    cr = mp.matrix([wd[1] * Iwd[2] - wd[2] * Iwd[1], wd[2] * Iwd[0] - wd[0] * Iwd[2], wd[0] * Iwd[1] - wd[1] * Iwd[0]])
    ba = Iw * al + cr
    return mp.matrix([m * a[0], m * a[1], m * (a[2] - g)] + [ba[k] for k in range(3)])


_B_KEYS = (("x", "x_tan"), ("x_d", "x_d_tan"), ("xdot", "xdot_tan"), ("xdot_d", "xdot_d_tan"), ("w", "w_tan"), ("w_d", "w_d_tan"))


def _state_mp(b, i, tans, k, step):
    """robot i's state at 50 digits, moved by `step` along direction k of `tans`: the vectors entrywise, Rwb <- (I + step [delta]x) Rwb
    (the tangent of exp(step [delta]x) Rwb: a central difference sees nothing of the second order) and Rwb_d likewise"""
    lift = lambda a: mp.matrix([DMR.mpf(float(v)) for v in np.asarray(a, float).reshape(-1)])
    st = {key: lift(b[key][i]) + step * lift(tans[name][k, i]) for key, name in _B_KEYS}
    for key, src, name in (("R", "Rwb", "Rwb_rot_tan"), ("Rd", "Rwb_d", "Rwb_d_rot_tan")):
        X = mp.matrix(3, 3)
        for j, v in enumerate(lift(b[src][i])):
            X[j // 3, j % 3] = v
        d = lift(tans[name][k, i])
        st[key] = X + step * (mp.matrix([[0, -d[2], d[1]], [d[2], 0, -d[0]], [-d[1], d[0], 0]]) * X)
    return st


@pytest.mark.parametrize("name", ["cheetah", "odd"])
def test_wrench_derivatives_against_differences_of_the_forward_wrench(name):
    """Per robot, one random direction u in every b-type input and both rotation tangents at once; FD = (b(+h u) - b(-h u)) / 2h of the
    50-digit forward wrench, h = 1e-25 (sensitivity_rotation_restatement.log_jacobian_mp's scheme: exact to ~25 digits, the log's
    branch held).  The forward wrench at h = 0 is first held to wrench_data itself.  Then
      * b_tan of tangent() is within C EPS b_sum of FD entry by entry, C = C_TAN_ALL / C_TAN_ODD of the law;
      * <b_bar, FD> + <grf_bar, d grf_body> + <r_bar, d r> = the pairing of u with x_bar ... w_d_bar of sensitivity() and Rwb_rot_bar,
        Rwb_d_rot_bar of rotation_cotangents() - the last two terms, the output transform grf_body = -Rwb^T f and the lever arms
        r = Rwb p, differentiated here directly at 50 digits - within (64 + 16 / |qw|) EPS of the sum of the magnitudes of all terms
        on both sides: the bar of tests/test_sensitivity_rotation_cpu.py's 50-digit test, whose reasoning (chains of < 40 rounded
        operations; the rounding of Re through the log's second derivative) covers the pull-back through the PD law as well.
    A kff line or the sic line in the wrong row of a restatement moves either side by 1e-5 ... 1e-3 of its terms at the odd law."""
    P = law(name)
    b, grf = batch(name, "feet")
    names = tuple(t for _, t in _B_KEYS) + ("Rwb_rot_tan", "Rwb_d_rot_tan")
    tans = TR.random_tangents(N, 1, 71, names=names)
    gbar = np.random.default_rng(72).normal(0.0, 1.0, (N, 12))
    t = TR.tangent(P, b, grf, tans, log_formation=name == "odd")
    s = SR.sensitivity(P, b, grf, gbar)
    r = RR.rotation_cotangents(P, b, grf, gbar, s["b_bar"], s["feet_bar"])
    _, bv = wrench_data(P, b)
    c_tan = C_TAN_ALL if name == "cheetah" else C_TAN_ODD
    worst = dict(b_tan=0.0, pairing=0.0)
    with mp.workdps(DMR.DPS):
        h = mp.mpf(10) ** -25
        lift = lambda a: mp.matrix([DMR.mpf(float(v)) for v in np.asarray(a, float).reshape(-1)])
        for i in range(N):
            st0 = _state_mp(b, i, tans, 0, 0)
            Re = st0["Rd"] * st0["R"].T
            case = DMR.eigen_case(np.array([[float(Re[a, c]) for c in range(3)] for a in range(3)]))
            assert case == -1  # (error angles of at most 0.6 rad)
            b0 = _wrench_mp(P, st0, case, False)
            assert np.all(distance(bv[i], [b0[c] for c in range(6)]) <= 64 * EPS * np.abs(bv[i]).max()), i  # it IS wrench_data's wrench
            sp, sm = _state_mp(b, i, tans, 0, h), _state_mp(b, i, tans, 0, -h)
            bp, bm = _wrench_mp(P, sp, case, False), _wrench_mp(P, sm, case, False)
            fd = [(bp[c] - bm[c]) / (2 * h) for c in range(6)]
            d, c = distance(t["b_tan"][0, i], fd), t["b_sum"][0, i]
            worst["b_tan"] = max(worst["b_tan"], float((d / (EPS * c)).max()))
            assert np.all(d <= c_tan * EPS * c), (i, (d / (EPS * c)).tolist())
            # the reverse side
            bb = lift(s["b_bar"][i])
            lhs = sum(bb[c] * fd[c] for c in range(6))
            mag = float(np.abs(s["b_bar"][i]) @ t["b_sum"][0, i])
            dR = (sp["R"] - sm["R"]) / (2 * h)
            gb, gbr, fbar, p = (np.asarray(a[i], float).reshape(4, 3) for a in (grf, gbar, s["feet_bar"], b["feet"]))
            aR, adR = np.abs(b["Rwb"][i].reshape(3, 3)), np.abs(np.array([[float(dR[a, c]) for c in range(3)] for a in range(3)]))
            for l in range(4):
                f = -(st0["R"] * lift(gb[l]))
                lhs += (lift(gbr[l]).T * (-(dR.T * f)))[0] + ((st0["R"] * lift(fbar[l])).T * (dR * lift(p[l])))[0]
                mag += float(np.abs(gbr[l]) @ (adR.T @ (aR @ np.abs(gb[l]))) + (aR @ np.abs(fbar[l])) @ (adR @ np.abs(p[l])))
            rhs, rmag = 0.0, 0.0
            for src, out, tan in [(s, key + "_bar", tn) for key, tn in _B_KEYS] + [(r, "Rwb_rot_bar", "Rwb_rot_tan"), (r, "Rwb_d_rot_bar", "Rwb_d_rot_tan")]:
                prod = src[out][i] * tans[tan][0, i]
                rhs, rmag = rhs + prod.sum(), rmag + np.abs(prod).sum()
            bar = (64 + 16 / abs(r["qw"][i])) * EPS * (mag + rmag)
            gap = float(abs(lhs - DMR.mpf(float(rhs))))
            worst["pairing"] = max(worst["pairing"], gap / max(bar, 1e-300))
            assert gap <= bar and (i % 16 == 0 or mag + rmag > 0), (i, gap, bar)
    print(name, "worst error / bar", worst)
    assert (np.abs(s["b_bar"]).max(axis=1) > 0).mean() > 0.75  # (not vacuous: most robots have a face that moves)


# ------------------------------------------------------------------ c. the confusions
def _roll(k):
    return lambda P: dict(P, **{k: np.roll(np.asarray(P[k], float), 1)})


def _swap(i, j):
    def f(P):
        kff = np.asarray(P["kff"], float).copy()
        kff[[i, j]] = kff[[j, i]]
        return dict(P, kff=kff)
    return f


_ANTI = 1e-3 * np.array([[0.0, 1.0, -2.0], [-1.0, 0.0, 1.5], [2.0, -1.5, 0.0]])  # the antisymmetric part that makes a transposed Ib visible
# name -> (transform, the restatements that read the transformed parameter, a change of the law made on both sides first)
CONFUSIONS = {
    "roll kp_p": (_roll("kp_p"), ("SR", "TR", "PR"), None),
    "roll kd_p": (_roll("kd_p"), ("SR", "TR", "PR"), None),
    "roll kp_w": (_roll("kp_w"), ("SR", "RR", "TR", "PR"), None),
    "roll kd_w": (_roll("kd_w"), ("SR", "RR", "TR", "PR"), None),
    "kff 0 <-> 1": (_swap(0, 1), ("SR", "TR", "PR"), None),
    "kff 3 <-> 4": (_swap(3, 4), ("SR", "RR", "TR", "PR"), None),
    "kff 4 <-> 5": (_swap(4, 5), ("SR", "RR", "TR", "PR"), None),
    "Ib -> diag": (lambda P: dict(P, Ib=np.diag(np.diag(np.asarray(P["Ib"], float)))), ("SR", "RR", "TR", "PR"), None),
    "Ib -> Ib^T": (lambda P: dict(P, Ib=np.asarray(P["Ib"], float).T.copy()), ("SR", "RR", "TR", "PR"), lambda P: dict(P, Ib=np.asarray(P["Ib"], float) + _ANTI)),
}


def _all_four(P, b, grf, fixed=None):
    """every output of the four restatements with its device bar (tests/test_gpu_sensitivity.py, test_gpu_sensitivity_rotation.py,
    test_gpu_sensitivity_params.py, test_gpu_odd_law.py), per robot: {restatement: [(value [n, m], bar [n, m])]}.  The kernels
    downstream of the adjoint are fed FIXED b_bar, feet_bar and adjoint (`fixed`: those of the untransformed law), as the GPU tests
    feed both sides the device's own."""
    tans = TR.random_tangents(N, 1, 81)
    gbar = np.random.default_rng(82).normal(0.0, 1.0, (N, 12))
    s = SR.sensitivity(P, b, grf, gbar)
    fixed = {k: s[k] for k in ("b_bar", "feet_bar", "adjoint")} if fixed is None else fixed
    r = RR.rotation_cotangents(P, b, grf, gbar, fixed["b_bar"], fixed["feet_bar"])
    p = PR.param_cotangents(P, b, grf, gbar, fixed["adjoint"], active=s["active"])
    t = TR.tangent(P, b, grf, tans, log_formation=True)
    cond = np.array([SR.reduced_condition(P, b, s["active"], i) for i in range(N)])
    flat = lambda a: np.asarray(a).reshape(N, -1)
    out = dict(SR=[(flat(s[k]), (2 * (16 * cond + 32) * EPS * np.abs(flat(s[k])).max(axis=1))[:, None] * np.ones_like(flat(s[k]))) for k in SR.OUTPUTS],
               RR=[(r[k], 160.0 * EPS * r["terms"][k]) for k in RR.OUTPUTS], PR=[(p["rows"], 160.0 * EPS * p["terms"])],
               TR=[(flat(t[k][0]), 4 * C_TAN_ODD * EPS * flat(t[m][0])) for k, m in (("grf_tan", "grf_sum"), ("b_tan", "b_sum"))])
    return out, fixed


@functools.lru_cache(maxsize=None)
def _base(name, pre):
    P = law(name)
    if pre is not None:
        P = CONFUSIONS[pre][2](P)
    return _all_four(P, *batch(name, "feet")), P


@pytest.mark.parametrize("what", list(CONFUSIONS))
def test_confusions_are_visible_at_the_odd_law_and_invisible_at_the_cheetahs(what):
    """Each transform of the law stands for an index mistake in a kernel's hand-written copy of the PD law.  At odd_law on odd_states
    every restatement that reads the transformed parameter moves at least one output by more than 100 x that output's device bar on
    at least 90 % of the robots with a stance foot; at the cheetah's law on config3's states every output of every restatement is
    bit-equal (the two Ib transforms are vacuous there: Ib is diagonal).  A restatement that does not read the parameter - the
    rotation cotangents, fed a fixed b_bar and feet_bar, read nothing of the linear half of the law - is bit-equal at both laws."""
    transform, reads, pre = CONFUSIONS[what]
    stance = np.arange(N) % 16 != 0
    for name in ("cheetah", "odd"):
        (ref, fixed), P = _base(name, what if pre is not None and name == "odd" else None)
        Pt = transform(P)
        if what.startswith("Ib") and name == "cheetah":
            assert np.array_equal(Pt["Ib"], P["Ib"])  # vacuous
        got, _ = _all_four(Pt, *batch(name, "feet"), fixed=fixed)
        for which in ("SR", "RR", "TR", "PR"):
            same = all(np.array_equal(a, c) for (a, _), (c, _) in zip(got[which], ref[which]))
            if name == "cheetah" or which not in reads:
                assert same, (what, name, which)
                continue
            moved = np.zeros(N, bool)
            for (a, _), (c, bar) in zip(got[which], ref[which]):
                moved |= (np.abs(a - c) > 100 * bar).any(axis=1)
            print(what, which, "robots with a stance foot that move by > 100 bars:", float(moved[stance].mean()))
            assert moved[stance].mean() >= 0.9, (what, which, float(moved[stance].mean()))


# ------------------------------------------------------------------ d. the branch sweep in forward mode
def sweep_laws():
    """RR.branch_sweep's own law (kp_w = 20) and the odd law with kp_w = 20 x (0.7, 1.0, 1.3)"""
    return {"sweep": dict(q.cheetah_params(mu=0.6), kp_w=np.full(3, 20.0)), "odd": dict(odd_law(), kp_w=20.0 * np.array([0.7, 1.0, 1.3]))}


def sweep_tangents(n):
    """K = 3 unit seeds, then K = 3 random, in Rwb_rot_tan and Rwb_d_rot_tan only"""
    unit = np.broadcast_to(np.eye(3)[:, None, :], (3, n, 3)).copy()
    rnd = TR.random_tangents(n, 3, 91, names=("Rwb_rot_tan", "Rwb_d_rot_tan"))
    return {"unit": {"Rwb_rot_tan": unit, "Rwb_d_rot_tan": unit.copy()}, "random": rnd}


@functools.lru_cache(maxsize=None)
def sweep_reference(name, seeds):
    """(P, batch with stance, forces, tangents, tangent(), [per robot tangent_mp() of direction 0; None for the unit seeds]) of the
    sweep: shared with tests/test_gpu_odd_law.py.  (A 50-digit pass costs 30 ms: one direction of the random seeds on all 181 cases is
    six seconds per law, all six directions would be forty.)  Every foot stands and the forces are interior (fz = 40 ... 80, |fx|, |fy| < 0.3 mu fz in the world
    frame), so all twelve coordinates are free and grf_tan sees db through the full solve."""
    P = sweep_laws()[name]
    b, *_ = RR.branch_sweep()
    n = b["x"].shape[0]
    b = dict(b, stance=np.ones((n, 4), np.uint8))
    rng = np.random.default_rng(92)
    fw = np.zeros((n, 4, 3))
    fw[..., 2] = rng.uniform(40.0, 80.0, (n, 4))
    fw[..., :2] = rng.uniform(-0.3, 0.3, (n, 4, 2)) * P["mu"] * fw[..., 2:]
    grf = np.ascontiguousarray(-np.einsum("nji,nkj->nki", b["Rwb"].reshape(n, 3, 3), fw).reshape(n, 12))
    tans = sweep_tangents(n)[seeds]
    t = TR.tangent(P, b, grf, tans, log_formation=True)
    refs = [TR.tangent_mp(P, b, grf, tans, i, 0, t["active"][i]) for i in range(n)] if seeds == "random" else None
    return P, b, grf, tans, t, refs


@pytest.mark.parametrize("name", ["sweep", "odd"])
def test_branch_sweep_in_forward_mode(name, seeds="random"):
    """tangent() against tangent_mp() on every case of the sweep (nine axes x angles 0 ... pi - 1e-7 x both signs, Rwb = Rwb_d = I),
    with only the two rotation tangents given (direction 0 of the random seeds): finite, flags 0, and inside C_TAN_ODD EPS x the
    condition sum on EVERY case, pi - 1e-7 included (measured: 1.02 under the sweep's law, 0.53 under the odd one) - the sum carries
    |J| of the log on the branch taken and grows with it towards pi, which is enough: nothing had to be added to it."""
    P, b, grf, tans, t, refs = sweep_reference(name, seeds)
    n = b["x"].shape[0]
    assert (t["flags"] == 0).all() and np.isfinite(t["grf_tan"]).all() and np.isfinite(t["b_tan"]).all()
    qw = np.array([RR.log_jacobian(b["Rwb_d"][i].reshape(3, 3) @ b["Rwb"][i].reshape(3, 3).T)[3] for i in range(n)])
    assert np.abs(qw).min() < 1e-7 and (qw < 0).any() and qw[-1] == 1.0  # (the cases near pi and the identity robot are in it)
    worst = 0.0
    for i in range(n):
        for k in range(1):
            for out, sums in (("grf_tan", "grf_sum"), ("b_tan", "b_sum")):
                d, c = distance(t[out][k, i], refs[i][out]), t[sums][k, i].reshape(-1)
                assert np.all(d[c == 0] == 0), (i, k, out)
                unit = C_TAN_ODD * EPS * c
                if (c > 0).any():
                    worst = max(worst, float((d[c > 0] / unit[c > 0]).max()))
                assert np.all(d <= unit), (i, k, out, float(qw[i]), (d / np.maximum(unit, 1e-300)).max())
    print(name, seeds, "worst error / bar", worst)
