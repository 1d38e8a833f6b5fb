"""GPU: qc_sensitivity_batch (csrc/qc_sensitivity.hpp) against the numpy restatement (tests/sensitivity_restatement.py), against the
same definitions at 50 digits on a fixed subset, and against central differences of control_batch itself.

Batch sizes 1, 63, 64, 65 and 130: tail lanes, one wave +- 1 (a workgroup is one wave), more than one workgroup.  Robot i of
every batch has contact pattern i % 16.  The placed forces and the three handles are solved_batch_support's: every component
exactly on a face or well inside, so the device and numpy classify alike.

Bars.  `flags` is compared exactly.  Floating-point outputs of a robot: the device solves the padded 12 x 12 system by LDL^T, the
restatement the explicit Z^T H Z by Cholesky.  Both are backward stable: the forward error of either is c n eps cond(Z^T H Z) with
n = 12 and c of order one, so each may be 16 eps cond from the true value; outside the solve every output is a chain of up to ~30 rounded products
and sums (the assembly of H and of v, the Iw pull-back), 32 eps of the output's scale, which is all there is on a face with one free
coordinate.  The two evaluations may be 2 x (16 cond + 32) eps max|output| apart.  The bar
is per robot and scaled by its own condition number, not one measured figure, because the faces of one batch range from a single
free coordinate (cond 1) to twelve (cond ~ 1e6 at the reference's weights): the relative error measured on a subset
(test_device_and_restatement_against_50_digits: ~2e-11 at cond ~ 4e5, i.e. 0.2 eps cond) would be loose for the first and false for
the last.  In the 50-digit test the device may be 8 x as far from the 50-digit value as the numpy restatement is at its worst (FMA
contraction, another elimination order), with a floor of 64 eps max|output|; both measured values are printed and recorded in
profiles/sensitivity.md."""
import ctypes
import functools

import numpy as np
import pytest

from tests import sensitivity_restatement as SR
from tests import solved_batch_support as SB
from tests.solved_batch_support import EPS, FORMS, SENTINEL, STATE_KEYS, assert_raw_refusals, batch_in, ctls, inputs, params, q, run  # noqa: F401

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 130)
WANT_ALL = SR.OUTPUTS + ("flags",)


_gbar = functools.partial(SB.gbar, 4000)


def _run(q, ctl, b, grf, gbar, want=WANT_ALL, **kw):
    return run(q, ctl.sensitivity_batch, b, grf, gbar, want=want, **kw)[0]


def _assert_close(P, b, got, ref, what):
    n = ref["flags"].shape[0]
    assert np.array_equal(got["flags"], ref["flags"]), what
    for i in range(n):
        cond = SR.reduced_condition(P, b, ref["active"], i)
        for k in SR.OUTPUTS:
            r, g = ref[k][i].reshape(-1), got[k][i].reshape(-1)
            bar = 2 * (16 * cond + 32) * EPS * np.abs(r).max()
            assert np.all(np.abs(g - r) <= bar), (what, i, k, float(np.abs(g - r).max()), bar)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("source", ["feet", "joint_q", "duty"])
def test_every_output_against_the_restatement(q, ctls, n, source):
    """Placed forces; `feet` with stance bytes, joint_q with the phase rule (the handle's duty, and gait_duty); all 16 contact
    masks once n >= 16; the all-swing mask gives all zeros."""
    P = params(q, "uniform")
    b, grf = inputs(n, source)
    gbar = _gbar(n)
    got = _run(q, ctls["uniform"], b, grf, gbar)
    ref = SR.sensitivity(P, b, grf, gbar)
    _assert_close(P, b, got, ref, (n, source))
    for i in range(0, n, 16):  # contact pattern 0: every foot swings
        assert got["flags"][i] == 0 and all(not got[k][i].any() for k in SR.OUTPUTS)
    if n >= 16:
        assert np.abs(got["adjoint"]).max() > 0 and (ref["flags"] == 0).all()


@pytest.fixture(scope="module")
def odd_ctl(q):
    """this module's own handle at ODD_KIN's hip and links"""
    c = SB.odd_handle(q)
    yield c
    c.close()


def test_joint_q_source_at_the_odd_model(q, odd_ctl):
    """test_every_output_against_the_restatement's joint_q case on a handle at ODD_KIN, n = 65: the restatement gets the feet of
    ODD_KIN's forward kinematics; the same bar."""
    P = params(q, "uniform")
    n = 65
    b, b_ref, grf, _ = SB.odd_inputs(n)
    gbar = _gbar(n)
    got = _run(q, odd_ctl, b, grf, gbar)
    ref = SR.sensitivity(P, b_ref, grf, gbar)
    _assert_close(P, b_ref, got, ref, (n, "joint_q at the odd model"))
    assert np.abs(got["adjoint"]).max() > 0 and (ref["flags"] == 0).all()
    wrong = SR.sensitivity(P, b, grf, gbar)  # the default model on the same angles: far outside the bar
    assert np.abs(wrong["feet_bar"] - ref["feet_bar"]).max() > 1e-6 * np.abs(ref["feet_bar"]).max()


def test_all_stance_without_stance_or_phase(q, ctls):
    P = params(q, "uniform")
    b = {k: v for k, v in inputs(64, "feet")[0].items() if k != "stance"}
    fw = np.tile([[2.0, -1.0, 30.0], [0.6 * 40.0, 3.0, 40.0], [-4.0, 5.0, 120.0], [1.0, 1.0, 10.0]], (64, 1, 1))  # interior, tied, fzmax, fzmin
    grf = -np.einsum("nji,nkj->nki", b["Rwb"].reshape(64, 3, 3), fw).reshape(64, 12)
    gbar = _gbar(64, 1)
    got = _run(q, ctls["uniform"], b, grf, gbar)
    ref = SR.sensitivity(P, b, grf, gbar)
    _assert_close(P, b, got, ref, "all stance")
    assert np.count_nonzero(got["adjoint"]) > 64 * 6


@pytest.fixture(scope="module")
def solved(q, ctls):
    """130 robots solved by control_batch on each formulation (race 0), and the restatement on those forces"""
    import torch
    from quadruped_control_amd import workloads

    n = 130
    b = dict(workloads.config3(n=n))
    b["stance"] = ((np.arange(n)[:, None] % 15 + 1 >> np.arange(4)[None, :]) & 1).astype(np.uint8)
    b = {k: np.ascontiguousarray(v) for k, v in b.items()}
    gbar = _gbar(n, 2)
    out = {}
    for kind, ctl in ctls.items():
        ctl.set_tuning(race=0)
        dev = q.to_device(b)
        o = ctl.control_batch(dev)
        torch.cuda.synchronize()
        assert int((o["status"] != 0).sum()) == 0
        grf = o["grf_body"].cpu().numpy()
        s = ctl.sensitivity_batch(dev, o["grf_body"], torch.from_numpy(gbar).cuda(), want=WANT_ALL)
        torch.cuda.synchronize()
        P = params(q, kind)
        out[kind] = dict(P=P, b=b, grf=grf, gbar=gbar, got={k: v.cpu().numpy() for k, v in s.items()}, ref=SR.sensitivity(P, b, grf, gbar))
    return out


@pytest.mark.parametrize("kind", list(FORMS))
def test_solved_points_of_each_formulation(solved, kind):
    """The kernel uses the handle's full S and W whatever form solved the batch."""
    c = solved[kind]
    _assert_close(c["P"], c["b"], c["got"], c["ref"], kind)
    assert (c["ref"]["flags"] == 0).mean() > 0.9 and np.abs(c["got"]["adjoint"]).max() > 0


def test_device_and_restatement_against_50_digits(solved):
    """Every eighth solved robot of the uniform and the dense handle at 50 digits: the device's and the numpy restatement's distance,
    relative to the output's largest entry, worst over the robots.  The device may be 8 x as far as numpy, floor 64 eps."""
    for kind in ("uniform", "dense"):
        c = solved[kind]
        worst = {k: [0.0, 0.0] for k in SR.OUTPUTS}
        for i in range(0, 130, 8):
            ref = SR.sensitivity_mp(c["P"], c["b"], c["grf"], c["gbar"], i, c["ref"]["active"][i])
            for k in SR.OUTPUTS:
                mag = max(SR.magnitude(ref[k]), 1e-300)
                worst[k][0] = max(worst[k][0], float(SR.distance(c["got"][k][i], ref[k]).max()) / mag)
                worst[k][1] = max(worst[k][1], float(SR.distance(c["ref"][k][i], ref[k]).max()) / mag)
        for k, (dev, host) in worst.items():
            print(f"50-digit {kind} {k}: device {dev:.3e} numpy {host:.3e}")
        for k, (dev, host) in worst.items():
            assert dev <= 8 * max(host, 8 * EPS), (kind, k, dev, host)


@pytest.mark.parametrize("law", ["cheetah", "odd"])
def test_finite_differences_of_control_batch(q, ctls, law):
    """<theta_bar, d> against control_batch itself at theta +- h d, 128 robots, race = 0, for a direction in the b-type inputs
    (exactly linear on a fixed face: h = 1e-3).  Kept: solved and the same want_active_set word at -h, 0, +h, flags 0.  Bar: the 6x6
    forms' forces carry an absolute error of eps (S / w) |b| ~ 1e-8 N at the reference's weights (csrc/qc_host.hpp), so the quotient
    carries 1e-8 / h = 1e-5 on derivatives of |theta_bar| |d| ~ 5e3: 2e-9 relative; the bar is 1e-6 |theta_bar| |d|.  law = "odd": the same h, bar and keep rule on a handle of the test's own at
    solved_batch_support.odd_law with odd_states of the batch; there the kept share must be at least one half, and is printed."""
    import torch
    from quadruped_control_amd import workloads

    ctl = ctls["uniform"] if law == "cheetah" else q.BalanceController.from_params(SB.odd_law(), device=0)
    try:
        _finite_differences(q, ctl, law, torch, workloads)
    finally:
        if law == "odd":
            ctl.close()


def _finite_differences(q, ctl, law, torch, workloads):
    ctl.set_tuning(race=0)
    n, h = 128, 1e-3
    b = dict(workloads.config3(n=n))
    b["stance"] = ((np.arange(n)[:, None] % 15 + 1 >> np.arange(4)[None, :]) & 1).astype(np.uint8)
    if law == "odd":
        b = SB.odd_states({k: np.ascontiguousarray(v) for k, v in b.items()}, 5)
    rng = np.random.default_rng(9)
    keys = ("x", "xdot", "w", "x_d", "xdot_d", "w_d")
    d = {k: rng.normal(0.0, 1.0, (n, 3)) for k in keys}
    gbar = _gbar(n, 3)

    def solve(step):
        bb = {k: np.ascontiguousarray(v + step * d[k] if k in d else v) for k, v in b.items()}
        dev = q.to_device(bb)
        o = ctl.control_batch(dev, want_active_set=True)
        torch.cuda.synchronize()
        return dev, o

    dev0, o0 = solve(0.0)
    (_, op), (_, om) = solve(h), solve(-h)
    s = ctl.sensitivity_batch(dev0, o0["grf_body"], torch.from_numpy(gbar).cuda(), want=tuple(k + "_bar" for k in keys) + ("flags",))
    torch.cuda.synchronize()
    s = {k: v.cpu().numpy() for k, v in s.items()}
    st = [o["status"].cpu().numpy() for o in (o0, op, om)]
    ws = [o["active_set"].cpu().numpy() for o in (o0, op, om)]
    keep = (st[0] == 0) & (st[1] == 0) & (st[2] == 0) & (ws[0] == ws[1]) & (ws[0] == ws[2]) & (s["flags"] == 0)
    assert keep.mean() >= (0.75 if law == "cheetah" else 0.5), keep.mean()
    fd = (gbar * (op["grf_body"].cpu().numpy() - om["grf_body"].cpu().numpy())).sum(axis=1) / (2 * h)
    an = sum((s[k + "_bar"] * d[k]).sum(axis=1) for k in keys)
    scale = np.sqrt(sum((s[k + "_bar"] ** 2).sum(axis=1) for k in keys)) * np.sqrt(sum((d[k] ** 2).sum(axis=1) for k in keys))
    err = np.abs(fd - an)
    print(law, "kept", keep.mean(), "worst relative error", float((err[keep] / np.maximum(scale[keep], 1e-300)).max()))
    assert (scale[keep] > 0).mean() > (0.9 if law == "cheetah" else 0.75)  # (odd states keep more robots whose face is pinned throughout: 0.85 measured)
    assert np.all(err[keep] <= 1e-6 * scale[keep])


def test_feet_finite_differences_of_control_batch(q, ctls):
    """feet_bar against control_batch itself for a random direction in `feet`: the only output that goes through v = S (A f - b),
    the r_bar cross products and the Rwb^T pull-back, and the direction that moves A and with it the Hessian.  128 robots, race = 0,
    h = 1e-4 (tests/test_sensitivity_cpu.py's sweep: truncation falls as h^2 down to there), solves at 0, +-h and +-2h.  Kept:
    solved and the same want_active_set word at all five points, flags 0.  The truncation is estimated per robot from the solver
    alone, t = |FD(h) - FD(2h)| (three times the h^2 term of FD(h)).  Bar: t + 1e-5 |feet_bar| |d| - the forces' absolute error of
    ~1e-8 N (csrc/qc_host.hpp) over h is 1e-4 on derivatives of |feet_bar| |d| ~ 7e2, 1.4e-7 relative; 1e-5 is the b-type test's
    rounding term scaled by its 1 / h."""
    import torch
    from quadruped_control_amd import workloads

    ctl = ctls["uniform"]
    ctl.set_tuning(race=0)
    n, h = 128, 1e-4
    b = dict(workloads.config3(n=n))
    b["stance"] = ((np.arange(n)[:, None] % 15 + 1 >> np.arange(4)[None, :]) & 1).astype(np.uint8)
    d = np.random.default_rng(10).normal(0.0, 1.0, (n, 12))
    gbar = _gbar(n, 6)

    def solve(step):
        bb = {k: np.ascontiguousarray(v + step * d if k == "feet" else v) for k, v in b.items()}
        dev = q.to_device(bb)
        o = ctl.control_batch(dev, want_active_set=True)
        torch.cuda.synchronize()
        return dev, o

    dev0, o0 = solve(0.0)
    pts = {k: solve(k * h)[1] for k in (-2, -1, 1, 2)}
    s = ctl.sensitivity_batch(dev0, o0["grf_body"], torch.from_numpy(gbar).cuda(), want=("feet_bar", "flags"))
    torch.cuda.synchronize()
    fbar, flags = s["feet_bar"].cpu().numpy().reshape(n, 12), s["flags"].cpu().numpy()
    w0 = o0["active_set"].cpu().numpy()
    keep = (o0["status"].cpu().numpy() == 0) & (flags == 0)
    for o in pts.values():
        keep &= (o["status"].cpu().numpy() == 0) & (o["active_set"].cpu().numpy() == w0)
    F = {k: o["grf_body"].cpu().numpy() for k, o in pts.items()}
    assert keep.mean() >= 0.75, keep.mean()
    fd1 = (gbar * (F[1] - F[-1])).sum(axis=1) / (2 * h)
    fd2 = (gbar * (F[2] - F[-2])).sum(axis=1) / (4 * h)
    an = (fbar * d).sum(axis=1)
    scale = np.linalg.norm(fbar, axis=1) * np.linalg.norm(d, axis=1)
    err, t = np.abs(fd1 - an), np.abs(fd1 - fd2)
    rel = lambda v: float((v[keep] / np.maximum(scale[keep], 1e-300)).max())
    print("kept", keep.mean(), "worst relative error", rel(err), "worst t", rel(t), "worst error beyond t", rel(np.maximum(err - t, 0.0)))
    assert (scale[keep] > 0).mean() > 0.9
    assert np.median(t[keep] / np.maximum(scale[keep], 1e-300)) < 1e-6  # (the estimate itself is small: the bar is tight)
    assert np.all(err[keep] <= t[keep] + 1e-5 * scale[keep])


@pytest.mark.parametrize("source", ["feet", "joint_q"])
def test_bad_pivot_sets_bit_1_and_poisons_the_robot(q, ctls, source):
    """A non-finite foot position (or joint angle) of a stance foot under given, finite forces: the face is read from the forces and
    has free coordinates, the reduced matrix is not finite, so the pivot check sets bit 1 and every output of that robot is NaN - on
    the device as in the restatement - and the robots next to it are untouched."""
    P = params(q, "uniform")
    n = 65
    b, grf = inputs(n, source)
    b = {k: v.copy() for k, v in b.items()}
    bad = [15, 47]  # contact pattern 15: four stance feet
    for i in bad:
        b["feet" if source == "feet" else "joint_q"][i, 4] = np.nan if i == 15 or source == "joint_q" else np.inf  # (an infinite angle has no sine)
    gbar = _gbar(n, 7)
    got = _run(q, ctls["uniform"], b, grf, gbar)
    ref = SR.sensitivity(P, b, grf, gbar)
    assert np.array_equal(got["flags"], ref["flags"])
    assert [int(got["flags"][i]) for i in bad] == [2, 2] and int(np.count_nonzero(got["flags"] & 2)) == 2
    for k in SR.OUTPUTS:
        assert np.isnan(got[k][bad]).all() and np.isnan(ref[k][bad]).all(), k
    good = np.setdiff1d(np.arange(n), bad)
    clean = {k: v[good] for k, v in b.items()}
    _assert_close(P, clean, {k: v[good] for k, v in got.items()}, SR.sensitivity(P, clean, grf[good], gbar[good]), ("bad pivot", source))


@pytest.mark.parametrize("source", ["feet", "joint_q"])
def test_second_round_of_the_grid_stride(q, ctls, source):
    """n = 4096 x 64 + 65 = 262 209 robots: the grid is capped at 4096 one-wave workgroups, so workgroup 0 walks a full second round
    and workgroup 1 has one live lane and 63 tail lanes in its second.  The batch is inputs(130) - placed forces, all 16 contact
    masks - with robot 15 poisoned by a NaN foot (bit 1, every output NaN) and robot 31 failed (all-zero forces: bit 0), tiled on the device
    (index = arange(n) % 130).  Robot i of the large launch equals robot i % 130 of the n = 130 launch of the same kernel - the launch
    test_every_output_against_the_restatement holds to the restatement - in every output, bit for bit, NaN positions included: a
    robot's arithmetic reads no other lane.  Both sources of the lever arms (feet; joint_q through the forward kinematics)."""
    import torch

    n, p = 4096 * 64 + 65, 130
    b, grf = inputs(p, source)
    b, grf = {k: v.copy() for k, v in b.items()}, grf.copy()
    b["feet" if source == "feet" else "joint_q"][15, 4] = np.nan
    grf[31] = 0.0
    dev = q.to_device(b)
    g, gb = SB.to_cuda(grf, _gbar(p))
    small = ctls["uniform"].sensitivity_batch(dev, g, gb, want=WANT_ALL)
    torch.cuda.synchronize()
    flags = small["flags"].cpu().numpy()
    print("flags of the period:", np.flatnonzero(flags).tolist(), flags[flags != 0].tolist())
    assert flags[15] == 2 and all(bool(torch.isnan(small[k][15]).all()) for k in SR.OUTPUTS)
    assert flags[31] & 1 and np.flatnonzero(flags).tolist() == [15, 31]  # the failed robot (all-zero forces under four stance feet): bit 0
    index = torch.arange(n, device="cuda") % p
    tile = lambda v: v.index_select(0, index).contiguous()
    big = ctls["uniform"].sensitivity_batch({k: tile(v) for k, v in dev.items()}, tile(g), tile(gb), want=WANT_ALL)
    torch.cuda.synchronize()
    for k in WANT_ALL:
        bits = lambda t: t.contiguous() if t.dtype != torch.float64 else t.contiguous().view(torch.int64)
        want, got = tile(bits(small[k])), bits(big[k])
        assert got.shape == want.shape and torch.equal(got, want), (k, int((got != want).reshape(n, -1).any(dim=1).nonzero()[0]))
    del big, small, index, dev, g, gb
    torch.cuda.empty_cache()


def test_flagged_robots(q, ctls):
    """A failed robot (non-finite input: all-zero forces) has adjoint 0 and bit 0; fzmin = fzmax sets bit 0 on every robot."""
    import torch
    from quadruped_control_amd import workloads

    n = 65
    b = {k: np.ascontiguousarray(v) for k, v in workloads.config3(n=n).items()}
    b["stance"] = np.ones((n, 4), np.uint8)
    b["x"][3, 0] = np.nan
    dev = q.to_device(b)
    ctl = ctls["uniform"]
    o = ctl.control_batch(dev)
    s = ctl.sensitivity_batch(dev, o["grf_body"], torch.from_numpy(_gbar(n, 4)).cuda(), want=("adjoint", "flags"))
    torch.cuda.synchronize()
    assert int(o["status"][3]) != 0 and not bool(o["grf_body"][3].any())
    assert int(s["flags"][3]) == 1 and not bool(s["adjoint"][3].any())
    assert int((s["flags"] & 2).sum()) == 0
    b["x"][3, 0] = 0.0
    ctl2 = q.BalanceController.from_params(dict(q.cheetah_params(mu=0.6), fzmin=35.0, fzmax=35.0), device=0)
    try:
        dev = q.to_device(b)
        o = ctl2.control_batch(dev)
        s = ctl2.sensitivity_batch(dev, o["grf_body"], torch.from_numpy(_gbar(n, 4)).cuda(), want=("adjoint", "flags"))
        torch.cuda.synchronize()
        assert bool((s["flags"] == 1).all()) and not bool(s["adjoint"].any())
    finally:
        ctl2.close()


def test_inputs_untouched_repeatable_and_capturable(q, ctls):
    """The inputs are left bit-identical, a second call repeats the first bit for bit, and the call captured into a graph on one
    stream (no parallel branches) and replayed gives the same bits."""
    import torch

    n = 130
    b, grf = inputs(n, "feet")
    dev = q.to_device(b)
    before = {k: v.clone() for k, v in dev.items()}
    g, gb = torch.from_numpy(grf).cuda(), torch.from_numpy(_gbar(n, 5)).cuda()
    g0, gb0 = g.clone(), gb.clone()
    ctl = ctls["dense"]
    first = ctl.sensitivity_batch(dev, g, gb, want=WANT_ALL)
    second = ctl.sensitivity_batch(dev, g, gb, want=WANT_ALL)
    torch.cuda.synchronize()
    assert all(torch.equal(dev[k], before[k]) for k in before) and torch.equal(g, g0) and torch.equal(gb, gb0)
    for k in WANT_ALL:
        assert torch.equal(first[k], second[k]), k
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        launch, out = ctl.plan_sensitivity(dev, g, gb, want=WANT_ALL, stream=stream)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            launch()
    for v in out.values():
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in WANT_ALL:
        assert torch.equal(out[k], first[k]), k


def test_refusals_raise_and_launch_nothing(q, ctls):
    """Each refusal of qc_sensitivity_batch raises ValueError with the library's message and launches nothing: the output tensor
    keeps its sentinel."""
    import torch
    from quadruped_control_amd import _lib

    ctl = ctls["uniform"]
    n = 65
    b, grf = inputs(n, "feet")
    dev = q.to_device(b)
    g, gb = torch.from_numpy(grf).cuda(), torch.from_numpy(_gbar(n)).cuda()
    out = {"adjoint": torch.full((n, 12), SENTINEL, dtype=torch.float64, device="cuda")}

    def refused(batch, grf_body, grf_bar, **kw):
        with pytest.raises(ValueError, match=r"^qc_sensitivity_batch:"):
            ctl.sensitivity_batch(batch, grf_body, grf_bar, want=kw.pop("want", ("adjoint",)), out=kw.pop("out", out), **kw)

    refused(dev, None, gb)
    refused(dev, g, None)
    for k in STATE_KEYS:
        refused({a: v for a, v in dev.items() if a != k}, g, gb)
    refused({a: v for a, v in dev.items() if a != "feet"}, g, gb)
    for bad in (-1e-9, float("nan"), float("inf")):
        refused(dev, g, gb, act_tol=bad)
    refused(dev, g, gb, want=(), out=None)
    lib = _lib.load()
    io = _lib.QcSensitivityIo()
    lib.qc_default_sensitivity(ctypes.byref(io))
    io.grf_body, io.grf_bar, io.adjoint = g.data_ptr(), gb.data_ptr(), out["adjoint"].data_ptr()
    bi = batch_in(dev, STATE_KEYS + ("feet", "stance"))
    assert_raw_refusals(lib.qc_sensitivity_batch, lambda: (ctl._h, n, bi, io), "qc_sensitivity_io", 112, 104, [(out["adjoint"], SENTINEL, True)])
