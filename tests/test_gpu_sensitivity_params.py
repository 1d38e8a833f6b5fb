"""GPU: qc_sensitivity_param_batch (csrc/qc_sensitivity_params.hpp) against the numpy restatement
(tests/sensitivity_params_restatement.py), its batch sum against its own rows, central differences of control_batch on handles built
at perturbed parameter sets, and the `params` leaf of the torch.autograd wrappers.

Rows: batch sizes 1, 63, 64, 65 and 130 (tail lanes, one wave +- 1, more than one workgroup); the placed forces and the handles are
solved_batch_support's.  Both sides are fed the SAME adjoint: the device's own, from sensitivity_batch.  The bar per entry is
C eps `terms`, `terms` being the restatement's sum of the magnitudes of the entry's contributions (every factor absolute).  C from
the longest rounded chain, mu_bar's: the lever arms r = R p 5; A z (a cross product 3, four feet and the sum 5) 8; q = S A z 11;
H z's row (cross product and sum 5, the 12-term row of W 23, the sum and the factor 2) 30; f_bar 5 and rho 1; the tie 3, its product
with f_z 1, the column term 5, four feet 8: 77 per evaluation, and the two evaluations may be twice that apart: C = 160.  With
joint_q the foot positions come from two forward kinematics (8 per evaluation): C = 176.

Sum: the kernel adds a workgroup's robots in index order into per-lane accumulators that live across the grid stride (at most
ceil(ceil(n / 64) / 1024) * 64 additions), the finisher's 16 waves each add every 16th partial in rising order and thread e adds the
16 wave sums: depth(n) below, read from csrc/qc_sensitivity_params.hpp.  The finisher strides over the partials by its WAVES, not its
threads, and the grid is capped at its thread count (1024), so "one partial more than the finisher's stride" is 17 partials (n = 1025)
and "one workgroup more than the cap" is n = 65537, where workgroup 0 walks a second round of the grid stride; both are in SUM_SIZES."""
import ctypes
import functools
import math

import numpy as np
import pytest

from tests import sensitivity_params_restatement as PR
from tests import solved_batch_support as SB
from tests.fd_support import GROUPS, fd_batch
from tests.solved_batch_support import EPS, FORMS, SENTINEL, STATE_KEYS, assert_raw_refusals, batch_in, ctls, inputs, params, q  # noqa: F401

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 130)
SUM_SIZES = (130, 1000, 1025, 65537)
HANDLES = tuple(FORMS)
FD_N = 480


@pytest.fixture(scope="module")
def ctl(ctls):
    return ctls["uniform"]


_gbar = functools.partial(SB.gbar, 7000)


def _guarded(n, rows=True, total=True):
    """output tensors with a sentinel row behind each: (out dict for the call, the full tensors)"""
    import torch

    full, out = {}, {}
    if rows:
        full["param_bar_rows"] = torch.full((n + 1, 211), SENTINEL, dtype=torch.float64, device="cuda")
        out["param_bar_rows"] = full["param_bar_rows"][:n]
    if total:
        full["param_bar"] = torch.full((2, 211), SENTINEL, dtype=torch.float64, device="cuda")
        out["param_bar"] = full["param_bar"][0]
    return out, full


def _sentinels_intact(full):
    return all(bool((t[-1] == SENTINEL).all()) for t in full.values())


def _adjoint(ctl, dev, g, gb):
    return ctl.sensitivity_batch(dev, g, gb, want=("adjoint", "flags"))


def depth(n):
    """additions on the longest path of the sum's tree (csrc/qc_sensitivity_params.hpp): a lane's accumulator over the robots of its
    workgroup's rounds of the grid stride, a finisher wave over every 16th partial, the 16 wave sums"""
    blocks = min((n + 63) // 64, 1024)
    rounds = ((n + 63) // 64 + blocks - 1) // blocks
    return rounds * 64 + (blocks + 15) // 16 + 16


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("source", ["feet", "joint_q", "duty"])
@pytest.mark.parametrize("handle", HANDLES)
def test_rows_against_the_restatement(q, ctls, n, source, handle):
    """Placed forces; `feet` with stance bytes, joint_q with the phase rule (the handle's duty, and gait_duty); all 16 contact masks
    once n >= 16; the all-swing mask gives exact zero rows.  A sentinel row sits behind the rows and behind the sum."""
    import torch

    P, c = params(q, handle), ctls[handle]
    b, grf = inputs(n, source)
    gbar = _gbar(n)
    dev = q.to_device(b)
    g, gb = torch.from_numpy(grf).cuda(), torch.from_numpy(gbar).cuda()
    s = _adjoint(c, dev, g, gb)
    out, full = _guarded(n)
    got = c.sensitivity_params_batch(dev, g, gb, s["adjoint"], want=("param_bar", "param_bar_rows"), out=out)
    torch.cuda.synchronize()
    assert _sentinels_intact(full)
    rows, z = got["param_bar_rows"].cpu().numpy(), s["adjoint"].cpu().numpy()
    ref = PR.param_cotangents(P, b, grf, gbar, z)
    bar = (160.0 if source == "feet" else 176.0) * EPS * ref["terms"]
    err = np.abs(rows - ref["rows"])
    worst = float((err / np.maximum(bar, 1e-300)).max())
    print((n, source, handle), "worst error / bar", worst)
    assert np.all(err <= bar), worst
    for i in range(0, n, 16):  # contact pattern 0: every foot swings
        assert not rows[i].any()
    if n >= 16:
        for k in PR.LAYOUT:
            assert np.abs(rows[:, PR.LAYOUT[k][0]]).max() > 0, k
        assert (s["flags"].cpu().numpy() == 0).all()


def test_joint_q_source_at_the_odd_model(q):
    """test_rows_against_the_restatement's joint_q case on a handle of this test's own at ODD_KIN, n = 65: the restatement gets the
    feet of ODD_KIN's forward kinematics; the same bar (176 EPS terms)."""
    import torch

    P, n = params(q, "uniform"), 65
    b, b_ref, grf, _ = SB.odd_inputs(n)
    gbar = _gbar(n)
    dev = q.to_device(b)
    g, gb = torch.from_numpy(grf).cuda(), torch.from_numpy(gbar).cuda()
    c = SB.odd_handle(q)
    try:
        s = _adjoint(c, dev, g, gb)
        got = c.sensitivity_params_batch(dev, g, gb, s["adjoint"], want=("param_bar_rows",))
        torch.cuda.synchronize()
    finally:
        c.close()
    rows, z = got["param_bar_rows"].cpu().numpy(), s["adjoint"].cpu().numpy()
    ref = PR.param_cotangents(P, b_ref, grf, gbar, z)
    bar = 176.0 * EPS * ref["terms"]
    err = np.abs(rows - ref["rows"])
    print("joint_q at the odd model: worst error / bar", float((err / np.maximum(bar, 1e-300)).max()))
    assert np.all(err <= bar)
    for k in PR.LAYOUT:
        assert np.abs(rows[:, PR.LAYOUT[k][0]]).max() > 0, k
    assert (s["flags"].cpu().numpy() == 0).all()


@pytest.mark.parametrize("n", SUM_SIZES)
def test_sum_is_reproducible_and_is_the_sum_of_the_rows(q, ctl, n):
    """Two calls give bit-equal sums; a call on another batch in between does not change the bits; the sum is the same whether the
    rows are asked for or not; against a float64 sum of the device's own rows the error is at most depth(n) eps sum_i |row_i|."""
    import torch

    b, grf = inputs(n, "feet")
    other_b, other_grf = inputs(130 if n != 130 else 65, "feet")
    dev, other = q.to_device(b), q.to_device(other_b)
    g, gb = torch.from_numpy(grf).cuda(), torch.from_numpy(_gbar(n, 1)).cuda()
    og, ogb = torch.from_numpy(other_grf).cuda(), torch.from_numpy(_gbar(other_grf.shape[0], 2)).cuda()
    z, oz = _adjoint(ctl, dev, g, gb)["adjoint"], _adjoint(ctl, other, og, ogb)["adjoint"]
    out, full = _guarded(n)
    first = ctl.sensitivity_params_batch(dev, g, gb, z, want=("param_bar", "param_bar_rows"), out=out)
    s1 = first["param_bar"].clone()
    ctl.sensitivity_params_batch(other, og, ogb, oz, want=("param_bar",))
    out2, full2 = _guarded(n, rows=False)
    s2 = ctl.sensitivity_params_batch(dev, g, gb, z, want=("param_bar",), out=out2)["param_bar"]
    s3 = ctl.sensitivity_params_batch(dev, g, gb, z, want=("param_bar",))["param_bar"]
    torch.cuda.synchronize()
    assert _sentinels_intact(full) and _sentinels_intact(full2)
    assert torch.equal(s1, s2) and torch.equal(s1, s3)
    rows = first["param_bar_rows"].cpu().numpy()
    ref, mag = np.array([math.fsum(col) for col in rows.T]), np.abs(rows).sum(axis=0)  # (fsum: the exactly rounded sum)
    err = np.abs(s1.cpu().numpy() - ref)
    bar = depth(n) * EPS * mag
    print(n, "depth", depth(n), "worst error / bar", float((err / np.maximum(bar, 1e-300)).max()))
    assert np.all(err <= bar) and np.abs(ref).max() > 0


@pytest.fixture(scope="module")
def fd_handles(q):
    made = []

    def make(P):
        c = q.BalanceController.from_params(P, device=0)
        c.set_tuning(race=0)
        made.append(c)
        return c

    yield make
    for c in made:
        c.close()


@pytest.mark.parametrize("group", list(GROUPS))
def test_central_differences_of_control_batch(q, fd_handles, group):
    """One direction per parameter group (the CPU test's, its h and its parameter sets): control_batch on handles built at
    theta + k h d, k = +-1, +-2, 480 robots.  Kept: solved and the same want_active_set word at all five points, flags 0; at least
    0.75.  The SUM over the kept robots of <row, d> against the summed quotient; the bar is the sum of the per-robot bars of the CPU
    test's quotient_check, made of the solver's own quotients (t = |FD(h) - FD(2h)|, N the fourth difference), with 1e-5 |row| |d| as
    the rounding term - test_gpu_sensitivity_rotation's, for the same reason: the forces' absolute error of ~1e-8 N over h."""
    import torch

    changes, h, _ = GROUPS[group]
    P = dict(q.cheetah_params(mu=0.6), **changes)
    d = PR.direction(np.random.default_rng(11), group, P)
    b = fd_batch(FD_N)
    dev = q.to_device(b)
    gbar = _gbar(FD_N, 3)

    def solve(k):
        c = fd_handles(PR.unpack(PR.pack(P) + k * h * d, P))
        o = c.control_batch(dev, want_active_set=True)
        torch.cuda.synchronize()
        return c, {a: v.cpu().numpy() for a, v in o.items()}, o

    c0, o0, dev_out = solve(0)
    pts = {k: solve(k)[1] for k in (-2, -1, 1, 2)}
    gb = torch.from_numpy(gbar).cuda()
    s = _adjoint(c0, dev, dev_out["grf_body"], gb)
    rows = c0.sensitivity_params_batch(dev, dev_out["grf_body"], gb, s["adjoint"], want=("param_bar_rows",))["param_bar_rows"].cpu().numpy()
    keep = (o0["status"] == 0) & (s["flags"].cpu().numpy() == 0)
    for o in pts.values():
        keep &= (o["status"] == 0) & (o["active_set"] == o0["active_set"])
    F = {k: o["grf_body"] for k, o in pts.items()}
    fd1 = (gbar * (F[1] - F[-1])).sum(axis=1) / (2 * h)
    fd2 = (gbar * (F[2] - F[-2])).sum(axis=1) / (4 * h)
    d4 = (gbar * (F[-2] - 4 * F[-1] + 6 * o0["grf_body"] - 4 * F[1] + F[2])).sum(axis=1) / (2 * h)
    an = rows @ d
    scale = np.linalg.norm(rows * (d != 0), axis=1) * np.linalg.norm(d)
    bar = np.abs(fd1 - fd2) + 3 * np.abs(d4) + 1e-5 * scale
    err_sum, bar_sum, scale_sum = abs(float((fd1 - an)[keep].sum())), float(bar[keep].sum()), float(scale[keep].sum())
    print(group, "kept", keep.mean(), "summed error / summed |row| |d|", err_sum / scale_sum, "summed bar / summed |row| |d|", bar_sum / scale_sum,
          "worst single error / bar", float((np.abs(fd1 - an)[keep] / np.maximum(bar[keep], 1e-300)).max()))
    assert keep.mean() >= 0.75, keep.mean()
    assert (an[keep] != 0).mean() >= (GROUPS[group][2] or 0.9)
    assert bar_sum <= 1e-3 * scale_sum  # (the bar is tight)
    assert err_sum <= bar_sum


def test_nan_adjoint_gives_a_nan_row_and_a_nan_sum(q, ctl):
    import torch

    n = 65
    b, grf = inputs(n, "feet")
    dev = q.to_device(b)
    g, gb = torch.from_numpy(grf).cuda(), torch.from_numpy(_gbar(n, 4)).cuda()
    z = _adjoint(ctl, dev, g, gb)["adjoint"]
    clean = ctl.sensitivity_params_batch(dev, g, gb, z, want=("param_bar_rows",))["param_bar_rows"].clone()
    z[16] = float("nan")  # an all-swing robot: the codes alone would leave its face entries at zero
    z[47] = float("nan")
    got = ctl.sensitivity_params_batch(dev, g, gb, z, want=("param_bar", "param_bar_rows"))
    torch.cuda.synchronize()
    rows = got["param_bar_rows"]
    assert bool(torch.isnan(rows[[16, 47]]).all()) and bool(torch.isnan(got["param_bar"]).all())
    good = [i for i in range(n) if i not in (16, 47)]
    assert torch.equal(rows[good], clean[good])


def test_inputs_untouched_and_capturable_behind_the_adjoint(q, ctl):
    """The inputs are left bit-identical, and sensitivity -> sensitivity_params captured into one graph on one stream and replayed
    gives the same bits."""
    import torch

    n = 130
    b, grf = inputs(n, "feet")
    dev = q.to_device(b)
    before = {k: v.clone() for k, v in dev.items()}
    g, gb = torch.from_numpy(grf).cuda(), torch.from_numpy(_gbar(n, 5)).cuda()
    z = _adjoint(ctl, dev, g, gb)["adjoint"]
    kept = [t.clone() for t in (g, gb, z)]
    first = ctl.sensitivity_params_batch(dev, g, gb, z, want=("param_bar", "param_bar_rows"))
    torch.cuda.synchronize()
    assert all(torch.equal(dev[k], before[k]) for k in before)
    assert all(torch.equal(a, c) for a, c in zip((g, gb, z), kept))
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        l1, s2 = ctl.plan_sensitivity(dev, g, gb, want=("adjoint",), stream=stream)
        l2, out = ctl.plan_sensitivity_params(dev, g, gb, s2["adjoint"], want=("param_bar", "param_bar_rows"), stream=stream)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            l1()
            l2()
    for v in list(out.values()) + list(s2.values()):
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in first:
        assert torch.equal(out[k], first[k]), k


def test_refusals_raise_and_launch_nothing(q, ctl):
    """Each refusal of qc_sensitivity_param_batch raises ValueError with the library's message and launches nothing: the outputs keep
    their sentinels."""
    import torch
    from quadruped_control_amd import _lib

    n = 65
    b, grf = inputs(n, "feet")
    dev = q.to_device(b)
    g, gb = torch.from_numpy(grf).cuda(), torch.from_numpy(_gbar(n)).cuda()
    z = torch.zeros((n, 12), dtype=torch.float64, device="cuda")
    out, full = _guarded(n)

    def refused(batch, *inputs, **kw):
        with pytest.raises(ValueError, match=r"^qc_sensitivity_param_batch:"):
            ctl.sensitivity_params_batch(batch, *inputs, want=kw.pop("want", ("param_bar", "param_bar_rows")), out=kw.pop("out", out), **kw)

    for m in range(3):
        refused(dev, *[None if k == m else t for k, t in enumerate((g, gb, z))])
    for k in STATE_KEYS:
        refused({a: v for a, v in dev.items() if a != k}, g, gb, z)
    refused({a: v for a, v in dev.items() if a not in ("Rwb_d", "x_d", "xdot_d", "w_d")}, g, gb, z)  # a commander-mode batch
    refused({a: v for a, v in dev.items() if a != "feet"}, g, gb, z)
    refused(dev, g, gb, z, want=(), out=None)
    for tol in (-1.0, float("nan"), float("inf")):
        refused(dev, g, gb, z, act_tol=tol)
    with pytest.raises(ValueError, match="unknown output"):
        ctl.sensitivity_params_batch(dev, g, gb, z, want=("param_bar", "S_bar"))
    lib = _lib.load()
    io = _lib.QcSensitivityParamIo()
    lib.qc_default_sensitivity_param(ctypes.byref(io))
    io.grf_body, io.grf_bar, io.adjoint = g.data_ptr(), gb.data_ptr(), z.data_ptr()
    io.param_bar_rows, io.param_bar = out["param_bar_rows"].data_ptr(), out["param_bar"].data_ptr()
    bi = batch_in(dev, STATE_KEYS + ("feet",))

    def rows_behind(what="the valid call"):
        assert _sentinels_intact(full), what

    assert_raw_refusals(lib.qc_sensitivity_param_batch, lambda: (ctl._h, n, bi, io), "qc_sensitivity_param_io", 56, 48,
                        [(out["param_bar_rows"], SENTINEL, True), (out["param_bar"], SENTINEL, True)], untouched=rows_behind, launched=rows_behind)


# ------------------------------------------------------------------ the autograd wrappers
def test_parameter_tensor_is_the_handles_own(q, ctl):
    theta = ctl.parameter_tensor()
    assert theta.shape == (211,) and theta.is_cuda and str(theta.dtype) == "torch.float64"
    assert np.array_equal(theta.cpu().numpy(), PR.pack(params(q, "uniform")))
    P = q.unpack_param_bar(theta)
    assert P["mu"] == 0.6 and np.array_equal(P["S"], np.asarray(params(q, "uniform")["S"], float)) and list(q.PARAM_LAYOUT) == list(PR.LAYOUT)


def test_autograd_params_grad_equals_the_direct_sum_bit_for_bit(q, ctl):
    import torch

    ctl.set_tuning(race=0)
    n = 130
    b = fd_batch(n)
    dev = q.to_device(b)
    o = ctl.control_batch(dev)
    gb = torch.from_numpy(_gbar(n, 9)).cuda()
    s = ctl.sensitivity_batch(dev, o["grf_body"], gb, want=("adjoint", "x_bar"))
    direct = ctl.sensitivity_params_batch(dev, o["grf_body"], gb, s["adjoint"])["param_bar"].clone()
    theta = ctl.parameter_tensor().requires_grad_(True)
    poisoned = torch.full_like(theta, float("nan")).requires_grad_(True)  # forward never reads the values
    for leaf in (theta, poisoned):
        grf, status = ctl.control_batch_autograd(q.to_device(b), params=leaf)
        assert grf.grad_fn is not None and not status.requires_grad and torch.equal(grf.detach(), o["grf_body"])
        (grad,) = torch.autograd.grad(grf, [leaf], gb)
        torch.cuda.synchronize()
        assert grad.shape == (211,) and torch.equal(grad, direct)
    assert float(direct.abs().max()) > 0
    # next to a state leaf: both gradients, each the direct call's
    dev2 = q.to_device(b)
    dev2["x"].requires_grad_(True)
    grf, _ = ctl.control_batch_autograd(dev2, params=theta)
    gx, gt = torch.autograd.grad(grf, [dev2["x"], theta], gb)
    assert torch.equal(gt, direct) and torch.equal(gx, s["x_bar"])
    with pytest.raises(ValueError, match="params"):
        ctl.control_batch_autograd(dev, params=torch.zeros(210, dtype=torch.float64, device="cuda"))


def test_autograd_without_params_is_the_parents(q, ctl, monkeypatch):
    """params=None (and a params leaf that does not require grad): no grad_fn where nothing requires grad, the results are
    control_batch's, and the parameter kernel is never launched."""
    import torch

    n = 65
    b = fd_batch(n)
    dev = q.to_device(b)
    o = ctl.control_batch(dev)
    monkeypatch.setattr(type(ctl), "sensitivity_params_batch", lambda *a, **k: pytest.fail("the parameter kernel was launched"))
    grf, status = ctl.control_batch_autograd(dev)
    assert grf.grad_fn is None and torch.equal(grf, o["grf_body"]) and torch.equal(status, o["status"])
    grf, _ = ctl.control_batch_autograd(dev, params=ctl.parameter_tensor())
    assert grf.grad_fn is None
    dev["x"].requires_grad_(True)
    gb = torch.from_numpy(_gbar(n, 8)).cuda()
    direct = ctl.sensitivity_batch({k: v.detach() for k, v in dev.items()}, o["grf_body"], gb, want=("x_bar",))["x_bar"]
    for kw in ({}, {"params": ctl.parameter_tensor()}):
        grf, _ = ctl.control_batch_autograd(dev, **kw)
        assert type(grf.grad_fn).__name__ == "_ControlBatchBackward"
        (gx,) = torch.autograd.grad(grf, [dev["x"]], gb)
        assert torch.equal(gx, direct)


@pytest.mark.parametrize("group", list(GROUPS))
def test_rollout_params_grad_against_a_two_handle_loop(q, fd_handles, group):
    """rollout_autograd(..., params=theta), 3 steps, 64 robots, against central differences of a hand-written loop with TWO handles:
    control_batch on the handle built at theta + k h d, plant_step on the BASE handle - the plant's use of mass and Ib is held fixed,
    which is what params.grad is documented to mean.  One direction per group (the CPU test's, with its h).  Kept: every solve of
    every loop solved with the base loop's active_set words; the loss is a fixed random linear functional of the kept robots' final
    x, xdot, w and Rwb, so that params.grad is the sum over exactly those robots.  Bar: the loop's own quotients (t = |FD(h) - FD(2h)|
    and the fourth difference N, summed per robot) and 1e-5 of the summed quotient as the rounding term; the gradient must also be non-zero.
    Measured on the committed seeds: kept 0.67 (mass, h = 1e-2) ... 1.0, |grad . d - quotient| / |quotient| 5e-7 ... 1e-3 (W diag),
    bar / |quotient| 1e-5 ... 0.2 (W: the final state barely depends on W, the quotient is 7e-5 against the loop's rounding)."""
    import torch

    changes, h, _ = GROUPS[group]
    P = dict(q.cheetah_params(mu=0.6), **changes)
    d = PR.direction(np.random.default_rng(11), group, P)
    n, steps, dt = 64, 3, 1.0 / 300.0
    b = fd_batch(n)
    R = b["Rwb"].reshape(n, 3, 3)
    fw = np.ascontiguousarray((b["x"][:, None, :] + np.einsum("nij,nlj->nli", R, b["feet"].reshape(n, 4, 3))).reshape(n, 12))
    rng = np.random.default_rng(21)
    wts = {k: rng.normal(0.0, 1.0, b[k].shape) for k in ("Rwb", "x", "xdot", "w")}
    base = fd_handles(P)

    def loop(k):
        c = base if k == 0 else fd_handles(PR.unpack(PR.pack(P) + k * h * d, P))
        dev = q.to_device(b)
        foot_world = torch.from_numpy(fw).cuda()
        words, ok = [], np.ones(n, bool)
        for _ in range(steps):
            o = c.control_batch(dev, want_active_set=True)
            words.append(o["active_set"].cpu().numpy().copy())
            ok &= o["status"].cpu().numpy() == 0
            feet = torch.empty_like(foot_world)
            base.plant_step(dev, o["grf_body"], foot_world, dt, feet=feet)
            dev["feet"] = feet
        torch.cuda.synchronize()
        loss = sum((wts[a] * dev[a].cpu().numpy()).reshape(n, -1).sum(axis=1) for a in wts)
        return loss, words, ok

    L0, w0, keep = loop(0)
    L = {}
    for k in (-2, -1, 1, 2):
        L[k], wk, ok = loop(k)
        keep = keep & ok & np.all([a == c for a, c in zip(wk, w0)], axis=0)
    fd1, fd2 = (L[1] - L[-1]) / (2 * h), (L[2] - L[-2]) / (4 * h)
    d4 = (L[-2] - 4 * L[-1] + 6 * L0 - 4 * L[1] + L[2]) / (2 * h)

    theta = base.parameter_tensor().requires_grad_(True)
    state, _ = base.rollout_autograd(q.to_device(b), torch.from_numpy(fw).cuda(), steps, dt, warm=False, params=theta)
    kept = torch.from_numpy(keep.astype(np.float64)).cuda()
    loss = sum((torch.from_numpy(wts[a]).cuda() * state[a]).reshape(n, -1).sum(dim=1) for a in wts)
    assert np.allclose(loss.detach().cpu().numpy(), L0, rtol=0, atol=1e-9 * np.abs(L0).max())  # the functional loop is the hand-written one
    (loss * kept).sum().backward()
    torch.cuda.synchronize()
    an = float(theta.grad.cpu().numpy() @ d)
    fd = float(fd1[keep].sum())
    bar = float((np.abs(fd1 - fd2) + 3 * np.abs(d4))[keep].sum()) + 1e-5 * abs(fd)
    print(group, "kept", keep.mean(), "grad . d", an, "quotient", fd, "error", abs(an - fd), "bar", bar)
    assert keep.mean() >= 0.5 and an != 0.0  # (a robot must hold its working sets at 15 solves here, not 5: the share is lower than one solve's)
    assert bar <= 0.5 * abs(fd)  # (a bar beyond half the quotient would let a wrong factor 2 pass)
    assert abs(an - fd) <= bar
