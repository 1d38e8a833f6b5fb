"""GPU: qc_sensitivity_kin_batch (csrc/qc_sensitivity_kin.hpp) against the numpy restatement (tests/sensitivity_kinematics_restatement.py),
against the same definitions at 50 digits, its halves and in-place forms against each other, and fused_tick_autograd
(quadruped_control_amd/autograd.py) against central differences of control_batch(want_torques=True) itself, against the chain of direct
calls and against control_batch_autograd.

Batch sizes 1, 15, 16, 17 and 40: the kernel gives every lane one (robot, leg) row and a workgroup is one wave, so 16 robots fill a
wave - tail lanes, one wave +- 1 robot, more than one workgroup (three, the last one partly filled).  The inputs are
sensitivity_kinematics_restatement.case(): solved_batch_support's placed forces over workloads.with_joint_angles, all 16 contact
masks once n >= 16, robots 5, 12, 19, ... failed through the status array, both mask sources, and a handle whose torque limits
(-2.5, 9 N m) clamp about half of the stance torque components.

The bar against the restatement, per output entry: C EPS `terms`, `terms` the restatement's sum of the magnitudes of the entry's
contributions with the absolute values of all factors.  C from the longest rounded chain, a monomial link * f(q0) * f(q1 + q2) of
the second derivatives inside joint_q_bar:  the device's sines and cosines are within 2 EPS of 1 (sincos_joint's pinned bar), its
s23 = s2 c3 + c2 s3 and c23 two such products and a sum, 7.2 EPS absolute - 27 EPS of a |sin(q1 + q2)| or |cos(q1 + q2)| >= 0.26
(asserted on the angles used); the factor of q0 or q1 4.1 EPS (|c1|, |s2|, |c2| >= 0.49 asserted: with_joint_angles keeps q1 within
0.8 +- 0.25, cos 1.05 = 0.4976; s1 is small but relatively exact: no reduction below pi/4); the monomial's two products 1;
a = l2 c2 + l3 c23 1/2; v = g1 s1 - g2 c1 and G00 = a v - l1 u 3; G s three products and two sums 2; the sum onto joint_q_bar_in
and J^T feet_bar 1: 39 for the device (measured against 50 digits: 1.4), 16 at most for the restatement
(tests/test_sensitivity_kinematics_cpu.py holds it to that; measured 1.0), and the two may be that far apart: C = 64.
Against 50 digits the device may be 4 x as far from the 50-digit value as the numpy restatement at its worst, floor 64 EPS of the
leg's largest entry (test_gpu_sensitivity's floor); both are printed and recorded in profiles/sensitivity_kinematics.md."""
import ctypes

import numpy as np
import pytest

from tests import device_math_reference as DMR
from tests import sensitivity_kinematics_restatement as KN
from tests import sensitivity_rotation_restatement as RR
from tests.fd_support import FD_H
from tests.solved_batch_support import EPS, SENTINEL, STATE_KEYS, assert_raw_refusals, batch_in, params, q  # noqa: F401

pytestmark = pytest.mark.gpu
SIZES = (1, 15, 16, 17, 40)
C_BAR = 64.0
COT = ("joint_tau_bar", "feet_bar", "grf_bar_in", "joint_q_bar_in")


@pytest.fixture(scope="module")
def ctl(q):
    c = q.BalanceController.from_params(params(q, "uniform"), device=0)
    c.set_kinematics(tau_min=KN.TAU_MIN, tau_max=KN.TAU_MAX)
    yield c
    c.close()


@pytest.fixture(scope="module")
def odd_ctl(q):
    """a handle of this module's own with ODD_KIN's hip and links and the limits the odd-model tests use (KN.ODD_TAU_MIN, ODD_TAU_MAX)"""
    c = q.BalanceController.from_params(params(q, "uniform"), device=0)
    c.set_kinematics(**dict(DMR.ODD_KIN.handle_arguments(), tau_min=KN.ODD_TAU_MIN, tau_max=KN.ODD_TAU_MAX))
    yield c
    c.close()


@pytest.fixture(scope="module")
def fd_ctl(q):
    c = q.BalanceController.from_params(params(q, "uniform"), device=0)
    c.set_kinematics(tau_min=KN.FD_TAU_MIN, tau_max=KN.FD_TAU_MAX)
    c.set_tuning(race=0)
    yield c
    c.close()


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(n):
    """an output of n rows with two sentinel rows behind it: (whole tensor, the view of the first n rows)"""
    import torch

    whole = torch.full((n + 2, 4, 3), SENTINEL, dtype=torch.float64, device="cuda")
    return whole, whole[:n]


def _run(q, ctl, b, grf, status, cot, want=KN.OUTPUTS, out=None):
    import torch

    dev = q.to_device(b)
    r = ctl.sensitivity_kinematics_batch(dev, None if grf is None else _cuda(grf), None if status is None else _cuda(status),
                                         **{k: _cuda(v) for k, v in cot.items()}, want=want, out=out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("source", ["stance", "phase"])
def test_every_output_against_the_restatement(q, ctl, n, source):
    """Both halves in one call with all four cotangents; stance bytes and the phase rule; contact pattern 0 and the failed robots
    give exact zeros in grf_bar - grf_bar_in and in the torque part of joint_q_bar; the rows behind row n keep their sentinel."""
    _every_output_against_the_restatement(q, ctl, n, source, None, KN.TAU_MIN, KN.TAU_MAX)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("source", ["stance", "phase"])
def test_every_output_against_the_restatement_at_the_odd_model(q, odd_ctl, n, source):
    """The same body on a handle at ODD_KIN's hip and links, the restatement evaluated under the model; the bar C EPS terms is the
    same expression (its assertions on the angles hold: the angles are the same)."""
    _every_output_against_the_restatement(q, odd_ctl, n, source, DMR.ODD_KIN, KN.ODD_TAU_MIN, KN.ODD_TAU_MAX)


def _every_output_against_the_restatement(q, ctl, n, source, kin, lo, hi):
    b, grf, status, cot = KN.case(n, source)
    ref = KN.kin_cotangents(b, grf, status, lo, hi, kin=kin, **cot)
    qq = b["joint_q"].reshape(n, 4, 3)
    a23 = qq[..., 1] + qq[..., 2]
    assert min(np.abs(np.sin(a23)).min(), np.abs(np.cos(a23)).min()) >= 0.26
    assert min(np.abs(np.cos(qq[..., 0])).min(), np.abs(np.sin(qq[..., 1])).min(), np.abs(np.cos(qq[..., 1])).min()) >= 0.49
    assert np.abs(np.abs(ref["tau_raw"] - lo)).min() > 1e-9 and np.abs(ref["tau_raw"] - hi).min() > 1e-9  # no torque on a limit
    if n >= 16:
        share = 1.0 - ref["mask"][ref["emit"]].mean()
        print((n, source), "clamped share of the stance torque components", share)
        assert 0.1 <= share <= 0.9
    guards = {k: _guarded(n) for k in KN.OUTPUTS}
    got = _run(q, ctl, b, grf, status, cot, out={k: v[1] for k, v in guards.items()})
    for k in KN.OUTPUTS:
        bar = C_BAR * EPS * ref["terms"][k]
        err = np.abs(got[k] - ref[k])
        worst = float((err / np.maximum(bar, 1e-300)).max())
        print((n, source), k, "worst error / bar", worst)
        assert np.all(err <= bar), (n, source, k, worst)
        assert bool((guards[k][0][n:] == SENTINEL).all()), k
    dead = ~ref["emit"]
    assert dead[0].all() and (n < 6 or dead[5].all())
    assert np.array_equal(got["grf_bar"][dead], cot["grf_bar_in"].reshape(n, 4, 3)[dead])
    torque_only = _run(q, ctl, b, grf, status, {"joint_tau_bar": cot["joint_tau_bar"]})
    assert not torque_only["grf_bar"][dead].any() and not torque_only["joint_q_bar"][dead].any()
    if n >= 16:
        assert np.abs(torque_only["grf_bar"][~dead]).max() > 0 and np.abs(torque_only["joint_q_bar"][~dead]).max() > 0


def test_against_50_digits(q, ctl):
    """Every leg of the 40-robot case at 50 digits: the device's and the numpy restatement's distance relative to the leg's largest
    entry.  The device may be 4 x as far as numpy at its worst, floor 64 EPS."""
    n = 40
    b, grf, status, cot = KN.case(n, "stance")
    ref = KN.kin_cotangents(b, grf, status, KN.TAU_MIN, KN.TAU_MAX, **cot)
    got = _run(q, ctl, b, grf, status, cot)
    dev_terms, dev = KN.worst_against_50_digits(b, grf, ref, got, **cot)
    host_terms, host = KN.worst_against_50_digits(b, grf, ref, ref, **cot)
    for k in KN.OUTPUTS:
        print(f"50-digit {k}: device {dev[k]:.3e} numpy {host[k]:.3e} of the largest entry; device {dev_terms[k]:.2f} numpy {host_terms[k]:.2f} EPS terms")
    for k in KN.OUTPUTS:
        assert dev[k] <= 4 * max(host[k], 16 * EPS), (k, dev[k], host[k])


def test_against_50_digits_at_the_odd_model(q, odd_ctl):
    """Every leg of the 40-robot case at 50 digits under ODD_KIN: the device's distance relative to the leg's largest entry within
    4 x max(C_KIN_ODD, 16) EPS - C_KIN_ODD the float64 restatement's own distance, measured on the CPU
    (tests/test_sensitivity_kinematics_cpu.py), never on the device; 16 EPS the default test's floor."""
    n, K = 40, DMR.ODD_KIN
    b, grf, status, cot = KN.case(n, "stance")
    ref = KN.kin_cotangents(b, grf, status, KN.ODD_TAU_MIN, KN.ODD_TAU_MAX, kin=K, **cot)
    got = _run(q, odd_ctl, b, grf, status, cot)
    dev_terms, dev = KN.worst_against_50_digits(b, grf, ref, got, kin=K, **cot)
    for k in KN.OUTPUTS:
        print(f"odd model 50-digit {k}: device {dev[k] / EPS:.2f} EPS of the largest entry (C_KIN_ODD {KN.C_KIN_ODD[k]}); {dev_terms[k]:.2f} EPS terms")
        assert dev[k] <= 4 * max(KN.C_KIN_ODD[k], 16.0) * EPS, (k, dev[k])


def test_second_round_of_the_grid_stride(q, ctl):
    """n = 65 536 + 17 robots, 262 212 (robot, leg) rows: the grid is capped at 4096 one-wave workgroups of 16 robots, so workgroup 0
    walks a full second round and workgroup 1 has four live rows in its second.  The batch is case(130) - all 16 contact masks, the
    failed robots 5, 12, 19, ..., about half of the torques clamped - with one robot's forces and another's joint angles poisoned
    with NaN, tiled on the device (index = arange(n) % 130).  Robot i of the large launch equals robot i % 130 of the n = 130 launch
    of the same kernel - the launch the tests above hold to the restatement and to 50 digits - in both outputs, bit for bit, NaN
    positions included: a row's arithmetic reads no other lane."""
    import torch

    n, p = 65536 + 17, 130
    b, grf, status, cot = KN.case(p, "stance")
    b, grf = {k: v.copy() for k, v in b.items()}, grf.copy()
    grf[33, 4] = np.nan
    b["joint_q"][34, 7] = np.nan
    assert (status != 0).any() and len({tuple(r) for r in b["stance"].tolist()}) == 16
    dev, t = q.to_device(b), {k: _cuda(v) for k, v in cot.items()}
    small = ctl.sensitivity_kinematics_batch(dev, _cuda(grf), _cuda(status), **t, want=KN.OUTPUTS)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(small[k][33:35]).any()) and bool(torch.isfinite(small[k][:33]).all()) for k in KN.OUTPUTS)
    index = torch.arange(n, device="cuda") % p
    tile = lambda v: v.index_select(0, index).contiguous()
    big = ctl.sensitivity_kinematics_batch({k: tile(v) for k, v in dev.items()}, tile(_cuda(grf)), tile(_cuda(status)),
                                           **{k: tile(v) for k, v in t.items()}, want=KN.OUTPUTS)
    torch.cuda.synchronize()
    for k in KN.OUTPUTS:
        want, got = tile(small[k].contiguous().view(torch.int64)), big[k].contiguous().view(torch.int64)
        assert got.shape == want.shape and torch.equal(got, want), (k, int((got != want).reshape(n, -1).any(dim=1).nonzero()[0]))
    del big, small, index, dev, t
    torch.cuda.empty_cache()


def test_halves_and_aliasing(q, ctl):
    """The torque half alone, the kinematics half alone and both in one call: grf_bar is the torque half's bit for bit; joint_q_bar of
    the one call equals the kinematics half run in place over the torque half's, and (joint_q_bar_in + the torque half's) + the
    kinematics half's summed on the host in that order, bit for bit - the kernel adds in that order and neither add is fused.
    Outputs written over grf_bar_in / joint_q_bar_in equal the out-of-place result bit for bit."""
    import torch

    n = 40
    b, grf, status, cot = KN.case(n, "stance")
    both = _run(q, ctl, b, grf, status, cot)
    torque = _run(q, ctl, b, grf, status, {k: cot[k] for k in ("joint_tau_bar", "grf_bar_in", "joint_q_bar_in")})
    assert np.array_equal(torque["grf_bar"], both["grf_bar"])
    chained = _run(q, ctl, b, None, None, {"feet_bar": cot["feet_bar"], "joint_q_bar_in": torque["joint_q_bar"]}, want=("joint_q_bar",))
    assert np.array_equal(chained["joint_q_bar"], both["joint_q_bar"])
    bare_torque = _run(q, ctl, b, grf, status, {"joint_tau_bar": cot["joint_tau_bar"]})
    bare_fk = _run(q, ctl, b, None, None, {"feet_bar": cot["feet_bar"]}, want=("joint_q_bar",))
    assert np.array_equal(bare_torque["joint_q_bar"] + bare_fk["joint_q_bar"],
                          _run(q, ctl, b, grf, status, {k: cot[k] for k in ("joint_tau_bar", "feet_bar")})["joint_q_bar"])
    copy = _run(q, ctl, b, None, None, {"joint_q_bar_in": cot["joint_q_bar_in"]}, want=("joint_q_bar",))
    assert np.array_equal(copy["joint_q_bar"].reshape(n, 12), cot["joint_q_bar_in"])
    # in place
    dev = q.to_device(b)
    t = {k: _cuda(v) for k, v in cot.items()}
    before = {k: v.clone() for k, v in dev.items()}
    r = ctl.sensitivity_kinematics_batch(dev, _cuda(grf), _cuda(status), **t, want=KN.OUTPUTS, out={"grf_bar": t["grf_bar_in"], "joint_q_bar": t["joint_q_bar_in"]})
    torch.cuda.synchronize()
    assert r["grf_bar"] is t["grf_bar_in"] and r["joint_q_bar"] is t["joint_q_bar_in"]
    assert np.array_equal(r["grf_bar"].cpu().numpy().reshape(n, 4, 3), both["grf_bar"])
    assert np.array_equal(r["joint_q_bar"].cpu().numpy().reshape(n, 4, 3), both["joint_q_bar"])
    assert all(torch.equal(dev[k], before[k]) for k in before)  # `in` is never written


def test_refusals_raise_and_launch_nothing(q, ctl):
    """The refusals of qc_sensitivity_kin_batch raise ValueError with the library's message and launch nothing: the output keeps its
    sentinel; then the raw C call through assert_raw_refusals."""
    import torch
    from quadruped_control_amd import _lib

    n = 17
    b, grf, status, cot = KN.case(n, "stance")
    dev = q.to_device(b)
    g, st = _cuda(grf), _cuda(status)
    t = {k: _cuda(v) for k, v in cot.items()}
    out = {"joint_q_bar": torch.full((n, 4, 3), SENTINEL, dtype=torch.float64, device="cuda"), "grf_bar": torch.full((n, 4, 3), SENTINEL, dtype=torch.float64, device="cuda")}

    def refused(batch, grf_body, status, want, **cots):
        with pytest.raises(ValueError, match=r"^qc_sensitivity_kin_batch:"):
            ctl.sensitivity_kinematics_batch(batch, grf_body, status, want=want, out={k: out[k] for k in want}, **cots)

    refused({k: v for k, v in dev.items() if k != "joint_q"}, g, st, ("joint_q_bar",), joint_tau_bar=t["joint_tau_bar"])
    refused(dev, None, st, ("joint_q_bar",), joint_tau_bar=t["joint_tau_bar"])
    refused(dev, g, None, ("joint_q_bar",), joint_tau_bar=t["joint_tau_bar"])
    refused(dev, g, st, ("grf_bar",), feet_bar=t["feet_bar"])
    refused(dev, g, st, ("joint_q_bar",), grf_bar_in=t["grf_bar_in"])
    refused(dev, g, st, (), joint_tau_bar=t["joint_tau_bar"])
    torch.cuda.synchronize()
    assert all(bool((v == SENTINEL).all()) for v in out.values())
    lib = _lib.load()
    io = _lib.QcSensitivityKinIo()
    lib.qc_default_sensitivity_kin(ctypes.byref(io))
    io.grf_body, io.status, io.joint_tau_bar, io.feet_bar = g.data_ptr(), st.data_ptr(), t["joint_tau_bar"].data_ptr(), t["feet_bar"].data_ptr()
    io.grf_bar, io.joint_q_bar = out["grf_bar"].data_ptr(), out["joint_q_bar"].data_ptr()
    bi = batch_in(dev, ("joint_q", "stance"))
    live = torch.from_numpy(np.repeat(KN.contact_mask(n, b["stance"]) & (status == 0)[:, None], 3).reshape(n, 4, 3)).cuda()
    assert_raw_refusals(lib.qc_sensitivity_kin_batch, lambda: (ctl._h, n, bi, io), "qc_sensitivity_kin_io", 72, 64,
                        [(out["joint_q_bar"], SENTINEL, True), (out["grf_bar"], SENTINEL, True)])
    assert bool((out["grf_bar"][~live] == 0).all())


def test_symbols_are_exported(q):
    from quadruped_control_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, name) and name in _lib.EXPORTS for name in ("qc_sensitivity_kin_batch", "qc_default_sensitivity_kin"))


# ------------------------------------------------------------------ fused_tick_autograd
def _leaves(q, b, requires):
    dev = q.to_device(b)
    for k in requires:
        dev[k].requires_grad_(True)
    return dev


def test_finite_differences_of_the_fused_tick(q, fd_ctl):
    """<joint_q.grad, dq> + <x.grad, dx> of fused_tick_autograd under the loss <c_tau, joint_tau> + <c_g, grf_body> against central
    differences of control_batch(want_torques=True) itself at joint_q + k h dq, x + k h dx, k = +-1, +-2: the 480 robots of
    sensitivity_kinematics_restatement.fd_case (fd_support.fd_batch with joint angles), committed directions and coefficients,
    h = FD_H, race = 0, torque limits (-4, 12 N m).  Kept: solved with the same want_active_set word and the same clamp mask (read off
    the torques the device wrote: on a limit or not) at all five points, flags 0; at least 0.75 with all 15 contact patterns among
    them (tests/test_sensitivity_kinematics_cpu.py holds the oracle's tick to the same rule at this h).
    Bar per robot, in the manner of fd_support.fd_bar: the truncation from the differences alone, t = |FD(h) - FD(2h)|; the rounding of
    the quotient, delta / h with delta = 1e-8 N (the forces' absolute error, csrc/qc_host.hpp) carried into each loss - sum |c_g| and,
    through tau = J^T g, sum_c |c_tau_c| sum_r |J_rc|; and the analytic side's own bar, C EPS sum terms |dq| of the kinematics kernel
    plus 1e-7 of |gradient| |direction| for the adjoint behind it (test_gpu_sensitivity_rotation's rounding term is 1e-5 of that)."""
    import torch

    ctl = fd_ctl
    n, h = 480, FD_H
    b, d = KN.fd_case(n)
    c_tau, c_g = _cuda(d["c_tau"]), _cuda(d["c_g"])

    def solve(k):
        bb = dict(b, joint_q=np.ascontiguousarray(b["joint_q"] + k * h * d["dq"]), x=np.ascontiguousarray(b["x"] + k * h * d["dx"]))
        o = ctl.control_batch(q.to_device(bb), want_active_set=True, want_torques=True)
        torch.cuda.synchronize()
        tau = o["joint_tau"].cpu().numpy()
        loss = (d["c_tau"] * tau).sum(axis=1) + (d["c_g"] * o["grf_body"].cpu().numpy()).sum(axis=1)
        return o["status"].cpu().numpy(), o["active_set"].cpu().numpy(), (tau == KN.FD_TAU_MIN) | (tau == KN.FD_TAU_MAX), loss

    dev = _leaves(q, b, ("joint_q", "x"))
    flags = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    tau, grf, status = ctl.fused_tick_autograd(dev, flags=flags, want_active_set=False)
    ((c_tau * tau).sum() + (c_g * grf).sum()).backward()
    torch.cuda.synchronize()
    gq, gx = dev["joint_q"].grad.cpu().numpy(), dev["x"].grad.cpu().numpy()
    st0, w0, m0, _ = solve(0)
    assert np.array_equal(st0, status.cpu().numpy())
    keep = (st0 == 0) & (flags.cpu().numpy() == 0)
    pts = {}
    for k in (-2, -1, 1, 2):
        st, w, m, pts[k] = solve(k)
        keep &= (st == 0) & (w == w0) & (m == m0).all(axis=1)
    fd1, fd2 = (pts[1] - pts[-1]) / (2 * h), (pts[2] - pts[-2]) / (4 * h)
    an = (gq * d["dq"]).sum(axis=1) + (gx * d["dx"]).sum(axis=1)
    geo = KN.geometry(b["joint_q"])
    delta = 1e-8 * (np.abs(d["c_g"]).sum(axis=1) + np.einsum("nlc,nlrc->n", np.abs(d["c_tau"]).reshape(n, 4, 3), geo["aJ"]))
    ref = KN.kin_cotangents(b, grf.detach().cpu().numpy(), st0, KN.FD_TAU_MIN, KN.FD_TAU_MAX, joint_tau_bar=d["c_tau"], feet_bar=None)
    scale = np.sqrt((gq ** 2).sum(axis=1) + (gx ** 2).sum(axis=1)) * np.sqrt((d["dq"] ** 2).sum(axis=1) + (d["dx"] ** 2).sum(axis=1))
    analytic = C_BAR * EPS * (ref["terms"]["joint_q_bar"].reshape(n, 12) * np.abs(d["dq"])).sum(axis=1) + 1e-7 * scale
    err, t = np.abs(fd1 - an), np.abs(fd1 - fd2)
    bar = t + delta / h + analytic
    rel = lambda v: float((v[keep] / np.maximum(scale[keep], 1e-300)).max())
    print("kept", keep.mean(), "clamped share", m0[(b["stance"] != 0).repeat(3, axis=1) & (st0 == 0)[:, None]].mean(), "worst relative error", rel(err),
          "worst t", rel(t), "worst error / bar", float((err[keep] / bar[keep]).max()), "median error / bar", float(np.median(err[keep] / bar[keep])))
    assert keep.mean() >= 0.75, keep.mean()
    pats = set((b["stance"][keep].astype(int) * [1, 2, 4, 8]).sum(axis=1).tolist())
    assert pats == set(range(1, 16)), sorted(pats)
    assert m0.any() and (scale[keep] > 0).mean() > 0.9
    assert np.median(t[keep] / np.maximum(scale[keep], 1e-300)) < 1e-6  # (the estimate itself is small: the bar is tight)
    assert np.all(err[keep] <= bar[keep]), float((err[keep] / bar[keep]).max())


@pytest.fixture(scope="module")
def solved_tick(q, fd_ctl):
    """130 robots of fd_case through control_batch(want_torques=True), and the chain of direct calls for one pair of cotangents"""
    import torch

    ctl = fd_ctl
    n = 130
    b, d = KN.fd_case(n)
    dev = q.to_device(b)
    o = ctl.control_batch(dev, want_torques=True)
    tb, gb = _cuda(d["c_tau"]), _cuda(d["c_g"])
    k = ctl.sensitivity_kinematics_batch(dev, o["grf_body"], o["status"], joint_tau_bar=tb, grf_bar_in=gb, want=("grf_bar", "joint_q_bar"))
    total = k["grf_bar"].view(n, 12)
    s = ctl.sensitivity_batch(dev, o["grf_body"], total, want=tuple(x + "_bar" for x in STATE_KEYS[2:]) + ("feet_bar", "b_bar", "adjoint", "flags"))
    s.update(ctl.sensitivity_rotation_batch(dev, o["grf_body"], total, s["b_bar"], s["feet_bar"], want=("Rwb_bar", "Rwb_d_bar")))
    s.update(ctl.sensitivity_params_batch(dev, o["grf_body"], total, s["adjoint"], want=("param_bar",)))
    first = k["joint_q_bar"].clone()
    s["joint_q_bar"] = ctl.sensitivity_kinematics_batch(dev, feet_bar=s["feet_bar"], joint_q_bar_in=k["joint_q_bar"], want=("joint_q_bar",),
                                                        out={"joint_q_bar": k["joint_q_bar"]})["joint_q_bar"]
    torch.cuda.synchronize()
    return dict(b=b, out=o, tau_bar=tb, grf_bar=gb, direct=s, first=first)


def test_autograd_equals_the_direct_calls_bit_for_bit(q, fd_ctl, solved_tick):
    import torch

    c, ctl = solved_tick, fd_ctl
    names = STATE_KEYS + ("joint_q",)
    dev = _leaves(q, c["b"], names)
    P = ctl.parameter_tensor().requires_grad_(True)
    flags = torch.full((130,), -1, dtype=torch.int32, device="cuda")
    tau, grf, status = ctl.fused_tick_autograd(dev, flags=flags, params=P)
    assert tau.grad_fn is not None and grf.grad_fn is not None and not status.requires_grad
    assert all(torch.equal(a.detach(), c["out"][k]) for a, k in ((tau, "joint_tau"), (grf, "grf_body"), (status, "status")))  # forward is control_batch
    grads = torch.autograd.grad([tau, grf], [dev[k] for k in names] + [P], [c["tau_bar"], c["grf_bar"]])
    torch.cuda.synchronize()
    for k, g in zip(names + ("param",), grads):
        assert (k == "param" or g.shape == dev[k].shape) and torch.equal(g.reshape(-1), c["direct"][k + "_bar"].reshape(-1)), k
    assert torch.equal(flags, c["direct"]["flags"])
    assert float(grads[-2].abs().max()) > 0 and not torch.equal(c["first"], c["direct"]["joint_q_bar"])  # both halves reached joint_q


def _device_feet(joint_q):
    """[n,12] body-frame feet: leg_fk of csrc/qc_device.hpp on joint_q [n,12], through the device-math probe (the library's flags)"""
    import __graft_entry__ as g

    g.build_device_probe()
    from tests import device_probe as D

    _, basis = DMR.sextic_basis_mp()
    D.set_params(DMR.HIP, DMR.LINKS, DMR.JC_KFF, DMR.JC_KP, DMR.JC_KD, basis, 0.18, 0.8, 0.08)
    n = joint_q.shape[0]
    _, p, _, _ = D.leg(np.tile(np.arange(4, dtype=np.int32), n), joint_q.reshape(-1, 3), np.zeros((4 * n, 3)))
    return np.ascontiguousarray(p.reshape(n, 12))


def test_an_output_the_loss_never_reached(q, fd_ctl, solved_tick, monkeypatch):
    """A loss on joint_tau alone or on grf_body alone: the missing cotangent arrives as None and becomes a missing pointer - the
    torque half is not launched at all without a cotangent on joint_tau -, and a loss on grf_body alone gives the state gradients
    of control_batch_autograd on the same batch with `feet` the forward kinematics of joint_q: the rotations' to the rotation
    test's joint_q bar (176 EPS of sensitivity_rotation_restatement's terms), the six vectors' to 176 EPS of the sum of the
    magnitudes of the robot's gradient entries.
    `feet` are the forward kinematics AS THE LIBRARY EVALUATES IT - leg_fk of csrc/qc_device.hpp through the device-math probe, built
    with the library's own flags; asserted to lie within 8 EPS of the leg's reach of the double restatement's -, so that the two
    forward passes solve the same problem.  With feet that numpy's sines made, a few EPS away, the two solves' forces come out
    3.5e-9 N apart and the gradients 1e-11 relative (measured: 262 - 650 of this bar, Rwb 2.4e6): that compares two inputs, not
    two code paths.  The forces' distance is printed."""
    import torch

    from tests import kkt_certificate_restatement as KC

    c, ctl = solved_tick, fd_ctl
    calls = []
    real = ctl.sensitivity_kinematics_batch

    def spy(*a, **kw):
        calls.append((kw.get("joint_tau_bar") is not None, kw.get("grf_bar_in") is not None, kw.get("feet_bar") is not None))
        return real(*a, **kw)

    monkeypatch.setattr(ctl, "sensitivity_kinematics_batch", spy)
    dev = _leaves(q, c["b"], STATE_KEYS + ("joint_q",))
    tau, grf, _ = ctl.fused_tick_autograd(dev)
    got = torch.autograd.grad([grf], [dev[k] for k in STATE_KEYS + ("joint_q",)], [c["grf_bar"]])
    torch.cuda.synchronize()
    assert calls == [(False, False, True)]
    calls.clear()
    dev2 = _leaves(q, c["b"], ("joint_q",))
    tau, grf, _ = ctl.fused_tick_autograd(dev2)
    torch.autograd.grad([tau], [dev2["joint_q"]], [c["tau_bar"]])
    torch.cuda.synchronize()
    assert calls == [(True, False, False), (False, False, True)]
    bf = {k: v for k, v in c["b"].items() if k != "joint_q"}
    bf["feet"] = _device_feet(c["b"]["joint_q"])
    theirs = KC.with_feet(c["b"])["feet"]
    reach = np.abs(DMR.LINKS).sum(axis=1) + np.abs(DMR.HIP).max(axis=1)
    assert np.all(np.abs(bf["feet"] - theirs).reshape(130, 4, 3) <= 8 * EPS * reach[None, :, None])
    devf = _leaves(q, bf, STATE_KEYS)
    grf_f, _ = ctl.control_batch_autograd(devf)
    ref = torch.autograd.grad(grf_f, [devf[k] for k in STATE_KEYS], c["grf_bar"])
    s = ctl.sensitivity_batch(devf, grf_f.detach(), c["grf_bar"], want=("b_bar", "feet_bar"))
    torch.cuda.synchronize()
    terms = RR.rotation_cotangents(params(q, "uniform"), bf, grf_f.detach().cpu().numpy(), c["grf_bar"].cpu().numpy(), s["b_bar"].cpu().numpy(),
                                   s["feet_bar"].cpu().numpy())["terms"]
    worst = {}
    for k, a, r in zip(STATE_KEYS, got, ref):
        a, r = a.cpu().numpy().reshape(130, -1), r.cpu().numpy().reshape(130, -1)
        scale = terms[k + "_bar"] if k in ("Rwb", "Rwb_d") else np.abs(r).sum(axis=1, keepdims=True)
        worst[k] = float((np.abs(a - r) / np.maximum(176.0 * EPS * scale, 1e-300)).max())
    print("the two forward solves' forces are apart by", float((grf.detach() - grf_f.detach()).abs().max()), "N")
    print("grf_body alone against control_batch_autograd on the feet, worst error / bar:", worst)
    assert all(v <= 1.0 for v in worst.values()), worst


def test_refused_batches(q, fd_ctl, solved_tick):
    """feet, swing_pos, swing_state and gait_dt in the batch are refused with ValueError; control_batch_autograd keeps its refusal of
    joint_q.requires_grad; a second backward raises."""
    import torch

    c, ctl = solved_tick, fd_ctl
    dev = _leaves(q, c["b"], ("joint_q",))
    for k in ("feet", "swing_pos", "swing_state", "gait_dt"):
        with pytest.raises(ValueError, match=k):
            ctl.fused_tick_autograd(dict(dev, **{k: torch.zeros((130, 12), dtype=torch.float64, device="cuda")}))
    with pytest.raises(ValueError, match="joint_q"):
        ctl.control_batch_autograd(dev)
    tau, _, _ = ctl.fused_tick_autograd(dev)
    tau.backward(c["tau_bar"])
    with pytest.raises(RuntimeError, match="backward through the graph a second time"):
        tau.backward(c["tau_bar"])
    torch.cuda.synchronize()
