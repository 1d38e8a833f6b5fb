"""GPU: qc_certify_batch (csrc/qc_certify.hpp) and certify_every of the rollouts against the numpy restatement
(tests/kkt_certificate_restatement.py) and, on a fixed subset, against the same formulas at 50 digits.

Batch sizes 1, 63, 64, 65, 257 and 1000: tail lanes, one wave +- 1 (a workgroup is one wave), several workgroups + a tail for
the summary.  Robot i of every batch has contact pattern i % 16.  All references are computed once per module.

Bars.  `active`, `flags` and the summary's counts and indices are compared exactly.  The test forces make that meaningful: every
component is exactly on a face (fx ASSIGNED as mu * fz, fz as fzmin / fzmax) or at least 0.1 mu fz / 1 N inside, and the on-face
components sit on robots with Rwb = I, where f_w = -grf_body exactly - the device evaluates the row tests without contraction,
so such a slack is exactly 0 on both sides and the worst primal residual (0.0, many ties, lowest index) is the same robot.
Floating-point outputs: in the 50-digit test the device may be 8 x as far from the 50-digit value as the numpy restatement is
(FMA contraction, another summation order), with a floor of 16 * 2^-53 times the sum of |terms| of the expression
(device_math_reference.Tr's condition sums; stationarity: on the scale 1 + |grad|).  The sweeps over sizes and handles use
_sweep_bars: both evaluations round sums of ~30 terms, so they differ by at most 2 * 32 * 2^-53 times the sum of |terms|
T = 2 (|A|^T |S| (|A| |f| + |b| + 1e3) + |W| |f|) - 1e3 N / N m bounding the terms of b itself for these parameters
(m kp |dx| ~ 11 * 100 * 1, |Iw| kp_w pi ~ 0.043 * 5000 * 3.2) - taken x 4 for the chain through f_w, r and b."""
import ctypes
import functools

import numpy as np
import pytest

from tests import device_math_reference as DMR
from tests import kkt_certificate_restatement as KR
from tests.kkt_batch import wrench_data
from tests.solved_batch_support import SENTINEL, STATE_KEYS, assert_raw_refusals, batch_in, ctls, inputs, params, q, run  # noqa: F401

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 257, 1000)
U = 2.0 ** -53
WANT_ALL = ("primal", "stationarity", "lambda", "grad", "active", "flags")


def _certify(q, ctl, b, grf, want=WANT_ALL, summary=True, **kw):
    res, out = run(q, ctl.certify_batch, b, grf, want=want, summary=summary, **kw)
    res.pop("summary", None)
    if summary:
        from quadruped_control_amd.balance_controller import certify_summary

        res["summary"] = certify_summary(out["summary"])
    return res


def _sweep_bars(P, b, grf):
    """(grad [n,12], lam [n,4,3], primal [n], stationarity [n]) bars of the module docstring"""
    bb = KR.with_feet(b)
    n = grf.shape[0]
    A, bv = wrench_data(P, bb)
    f = np.abs(np.einsum("nij,nkj->nki", bb["Rwb"].reshape(n, 3, 3), grf.reshape(n, 4, 3))).reshape(n, 12)
    S, W = np.abs(np.asarray(P["S"], float).reshape(6, 6)), np.abs(np.asarray(P["W"], float).reshape(12, 12))
    T = 2.0 * (np.einsum("nji,nj->ni", np.abs(A), (np.einsum("nij,nj->ni", np.abs(A), f) + np.abs(bv) + 1e3) @ S.T) + f @ W.T)
    grad = 4 * 64 * U * T
    t = grad.reshape(n, 4, 3)
    lam = np.stack([t[..., 0], t[..., 1], P["mu"] * (t[..., 0] + t[..., 1]) + t[..., 2]], axis=-1)
    primal = 16 * 2 * U * (f.reshape(n, 4, 3).sum(axis=2).max(axis=1) * (1.0 + P["mu"]) + P["fzmax"])
    return grad, lam, primal, lam[..., 2].max(axis=1)


@pytest.fixture(scope="module")
def odd_ctls(q):
    """this module's own handles at ODD_KIN's hip and links"""
    from tests.solved_batch_support import odd_handle

    out = {k: odd_handle(q, k) for k in ("uniform", "dense")}
    yield out
    for c in out.values():
        c.close()


def _check_against_restatement(P, b, grf, got, ref):
    n = grf.shape[0]
    assert np.array_equal(got["active"], ref["active"])
    assert np.array_equal(got["flags"], ref["flags"])
    bg, bl, bp, bs = _sweep_bars(P, b, grf)
    assert np.all(np.abs(got["grad"] - ref["grad"]) <= bg)
    assert np.all(np.abs(got["lambda"].reshape(n, 4, 3) - ref["lam"]) <= bl)
    assert np.all(np.abs(got["primal"] - ref["primal"]) <= bp)
    gn = 1.0 + np.linalg.norm(ref["grad"], axis=1)
    assert np.all(np.abs(got["stationarity"] - ref["stationarity"]) <= bs / gn + 4 * U * ref["stationarity"])
    s, r = got["summary"], ref["summary"]
    for k in ("n_fail", "n_nonfinite", "n_swing_nonzero", "arg_primal", "arg_stationarity"):
        assert s[k] == r[k], (k, s, r)


# ------------------------------------------------------------------ tails and block edges
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("source", ["feet", "joint_q", "duty"])
def test_sizes_contact_patterns_and_inputs(q, ctls, n, source):
    """Every size, every contact pattern, feet + stance bytes and joint_q + gait_phase (with the handle's duty and a given one):
    all outputs against the restatement, nothing written past the end (each array is allocated with a sentinel row behind it)."""
    import torch

    P = params(q, "uniform")
    b, grf = inputs(n, source)
    ref = KR.certificate(P, b, grf, default_duty=KR.DEFAULT_DUTY)
    dev = q.to_device(b)
    shapes = {"primal": ((n + 1,), torch.float64), "stationarity": ((n + 1,), torch.float64), "lambda": ((n + 1, 4, 3), torch.float64),
              "grad": ((n + 1, 12), torch.float64), "active": ((n + 1, 4), torch.uint8), "flags": ((n + 1,), torch.int32)}
    big = {k: torch.full(s, 77 if dt != torch.float64 else SENTINEL, dtype=dt, device="cuda") for k, (s, dt) in shapes.items()}
    out = {k: v[:n] for k, v in big.items()}
    out["summary"] = torch.zeros(56, dtype=torch.uint8, device="cuda")
    res = ctls["uniform"].certify_batch(dev, torch.from_numpy(grf).cuda(), want=WANT_ALL, out=out)
    torch.cuda.synchronize()
    from quadruped_control_amd.balance_controller import certify_summary

    got = {k: v.cpu().numpy() for k, v in res.items() if k != "summary"}
    got["summary"] = certify_summary(res["summary"])
    _check_against_restatement(P, b, grf, got, ref)
    for k, v in big.items():
        tail = v[n].cpu().numpy()
        assert np.all(tail == (SENTINEL if v.dtype == torch.float64 else 77)), k


def test_joint_q_source_at_the_odd_model(q, odd_ctls):
    """The joint_q source on a handle at ODD_KIN (n = 65): every output against the restatement, which gets the feet of ODD_KIN's
    forward kinematics; the same bars.  The default model's feet on the same angles are centimetres away (asserted)."""
    from tests.solved_batch_support import odd_inputs

    P = params(q, "uniform")
    b, b_ref, grf, _ = odd_inputs(65)
    assert np.abs(b_ref["feet"] - KR.with_feet(b)["feet"]).max() > 0.01
    ref = KR.certificate(P, b_ref, grf, default_duty=KR.DEFAULT_DUTY)
    got = _certify(q, odd_ctls["uniform"], b, grf)
    _check_against_restatement(P, b_ref, grf, got, ref)


def test_non_optimal_points_against_50_digits_at_the_odd_model(q, odd_ctls):
    """test_non_optimal_points_against_50_digits' joint_q case on a handle at ODD_KIN, n = 65: the same body, the 50-digit pass
    through ODD_KIN's forward kinematics."""
    from tests.solved_batch_support import odd_inputs

    b, b_ref, grf, kin = odd_inputs(65)
    _non_optimal_points(q, odd_ctls["dense"], b, b_ref, grf, kin, 40)


@pytest.mark.parametrize("form", ["uniform", "per-axis", "dense"])
def test_every_formulation_uses_the_full_weights(q, ctls, form):
    """The certificate reads the handle's full S and W whatever form the solver runs: uniform W, per-axis W, dense S and W."""
    P = params(q, form)
    b, grf = inputs(257, "feet")
    got = _certify(q, ctls[form], b, grf)
    _check_against_restatement(P, b, grf, got, KR.certificate(P, b, grf))


# ------------------------------------------------------------------ non-optimal points against 50 digits
@pytest.mark.parametrize("source", ["feet", "joint_q"])
def test_non_optimal_points_against_50_digits(q, ctls, source):
    """Feasible but wrong forces (module docstring): the integer outputs equal the restatement's exactly on all 257 robots, and on
    the first 32 the device is at most 8 x as far from the 50-digit value as the numpy restatement is (floor 16 * 2^-53 * sum of
    |terms|).  Measured worst ratios device distance / bar: profiles/kkt_certificate.md."""
    b, grf = inputs(257, source)
    _non_optimal_points(q, ctls["dense"], b, b, grf, None if source == "feet" else (DMR.HIP.reshape(-1), DMR.LINKS.reshape(-1)), 200)


def _non_optimal_points(q, ctl, b, b_ref, grf, kin, least_failed):
    """b: what the device reads; b_ref: what the restatements read (b itself, or b with the model's feet)"""
    P = params(q, "dense")
    ref = KR.certificate(P, b_ref, grf)
    got = _certify(q, ctl, b, grf)
    source = "feet" if kin is None else "joint_q"
    b = b_ref
    assert ref["summary"]["n_fail"] >= least_failed and ref["summary"]["n_nonfinite"] == 0  # (the robots without a stance foot carry no force: they pass)
    assert np.array_equal(got["active"], ref["active"]) and np.array_equal(got["flags"], ref["flags"])
    for k in ("n_fail", "n_nonfinite", "n_swing_nonzero", "arg_primal", "arg_stationarity"):
        assert got["summary"][k] == ref["summary"][k], (k, got["summary"], ref["summary"])
    codes = ref["active"]
    assert set(np.unique(codes & 3)) == {0, 1, 2} and set(np.unique((codes >> 4) & 3)) == {0, 1, 2}  # every single-row case occurs
    worst = {}
    for i in range(32):
        mpv = KR.certificate_mp(P, b, grf, i, ref["active"][i], kin=kin)
        for name, dev_v, np_v in (("grad", got["grad"][i], ref["grad"][i]), ("lam", got["lambda"][i], ref["lam"][i]),
                                  ("primal", got["primal"][i], ref["primal"][i]), ("stationarity", got["stationarity"][i], ref["stationarity"][i])):
            vals, scale = mpv[name]
            d_dev, d_np = KR.distance(dev_v, vals), KR.distance(np_v, vals)
            bar = np.maximum(8.0 * d_np, 16 * U * scale)
            ok = d_dev <= bar
            ratio = float(np.max(d_dev / np.where(bar > 0, bar, 1.0)))
            worst[name] = max(worst.get(name, 0.0), ratio)
            assert np.all(ok), (i, name, d_dev, d_np, scale)
    print(f"kkt certificate, {source}: worst device distance / bar over 32 robots: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ------------------------------------------------------------------ solved points, perturbation
@functools.lru_cache(maxsize=None)
def _solved(n):
    import torch

    import quadruped_control_amd as q
    from quadruped_control_amd import workloads

    P = q.cheetah_params(mu=0.6)
    b = {k: np.ascontiguousarray(v) for k, v in workloads.config3(n=n).items()}
    ctl = q.BalanceController.from_params(P, device=0)
    out = ctl.control_batch(q.to_device(b))
    torch.cuda.synchronize()
    res = out["grf_body"].cpu().numpy(), out["status"].cpu().numpy()
    ctl.close()
    return b, res[0], res[1]


def test_solved_points_pass_the_projects_bars(q, ctls):
    """After control_batch every robot with status 0 passes assert_kkt's defaults on the device: primal < 1e-7, stationarity < 1e-8."""
    b, grf, status = _solved(1000)
    got = _certify(q, ctls["uniform"], b, grf)
    ok = status == 0
    assert ok.sum() >= 990
    assert np.all(got["primal"][ok] < 1e-7) and np.all(got["stationarity"][ok] < 1e-8) and np.all(got["flags"][ok] == 0)
    ref = KR.certificate(params(q, "uniform"), b, grf)
    assert got["summary"]["n_fail"] == ref["summary"]["n_fail"] == int((~ok & ((ref["primal"] > 1e-7) | (ref["stationarity"] > 1e-8))).sum())


def test_failed_robots_are_counted_where_zero_forces_violate(q):
    """A handle capped at two recalculations leaves most robots unsolved, with zero forces: n_fail is the number of robots with
    status != 0 whose zero forces really violate the bounds (fzmin = 10 N: every one with a stance foot), as the restatement counts."""
    import torch
    from quadruped_control_amd import workloads

    P = q.cheetah_params(mu=0.6)
    b = {k: np.ascontiguousarray(v) for k, v in workloads.config3(n=257).items()}
    ctl = q.BalanceController.from_params(P, device=0, max_iter=2)
    dev = q.to_device(b)
    out = ctl.control_batch(dev)
    cert = ctl.certify_batch(dev, out["grf_body"])
    torch.cuda.synchronize()
    from quadruped_control_amd.balance_controller import certify_summary

    status, grf = out["status"].cpu().numpy(), out["grf_body"].cpu().numpy()
    s = certify_summary(cert["summary"])
    ctl.close()
    ref = KR.certificate(P, b, grf)
    failed = status != 0
    assert failed.sum() >= 50 and not grf[failed].any()
    bad = ~(ref["primal"] <= 1e-7) | ~(ref["stationarity"] <= 1e-8) | ref["swing_nonzero"]
    assert not bad[~failed].any()
    assert s["n_fail"] == int((failed & bad).sum()) == ref["summary"]["n_fail"]
    assert np.all(cert["primal"].cpu().numpy()[failed & bad] == 10.0)  # fzmin - 0


def test_perturbing_one_force_fails_exactly_that_robot(q, ctls):
    """+1e-3 N on one component of one solved robot: its residual rises above the bars, it becomes the summary's worst robot, n_fail
    grows by exactly one, and every other robot's outputs are bit-identical."""
    b, grf, status = _solved(257)
    assert (status == 0).all()
    base = _certify(q, ctls["uniform"], b, grf)
    assert base["summary"]["n_fail"] == 0
    victim = 133
    foot = int(np.flatnonzero(b["stance"][victim])[0])
    g2 = grf.copy()
    g2[victim, 3 * foot + 2] += 1e-3
    got = _certify(q, ctls["uniform"], b, g2)
    assert got["stationarity"][victim] > 1e-8 or got["primal"][victim] > 1e-7
    assert got["summary"]["n_fail"] == 1
    assert victim in (got["summary"]["arg_stationarity"], got["summary"]["arg_primal"])
    others = np.arange(257) != victim
    for k in WANT_ALL:
        assert np.array_equal(got[k][others], base[k][others]), k


# ------------------------------------------------------------------ the summary
def test_summary_is_the_reduction_of_the_per_robot_arrays(q, ctls):
    """Bit-equal to reducing the device's own per-robot arrays on the host; identical with every per-robot pointer NULL; one NaN
    state sets n_nonfinite = 1 and leaves worst_* finite.  n = 1000: sixteen workgroups, the last one with a tail."""
    b, grf = inputs(1000, "feet")
    got = _certify(q, ctls["uniform"], b, grf)
    host = KR.summarize(got["primal"], got["stationarity"], (got["flags"] & 1) != 0)
    assert got["summary"] == host
    alone = _certify(q, ctls["uniform"], b, grf, want=())
    assert alone == {"summary": got["summary"]}
    bn = dict(b, x=b["x"].copy())
    bn["x"][517, 1] = np.nan
    nan = _certify(q, ctls["uniform"], bn, grf)
    s = nan["summary"]
    assert s["n_nonfinite"] == 1 and nan["flags"][517] & 2 and np.isnan(nan["stationarity"][517])
    assert np.isfinite(s["worst_primal"]) and np.isfinite(s["worst_stationarity"]) and s["arg_stationarity"] != 517
    assert s == KR.summarize(nan["primal"], nan["stationarity"], (nan["flags"] & 1) != 0)
    assert not (nan["stationarity"][517] <= 1e-8) and s["n_fail"] >= got["summary"]["n_fail"]  # a NaN fails


@pytest.mark.parametrize("source", ["feet", "joint_q"])
def test_second_round_of_the_grid_stride(q, ctls, source):
    """n = 4096 x 64 + 65 = 262 209 robots: the grid is capped at 4096 one-wave workgroups, so workgroup 0 walks a full second round,
    carrying its summary accumulator across, and workgroup 1 has one live lane (robot n - 1) and 63 tail lanes in its second.  The
    batch is inputs(130) - placed forces, all 16 contact masks - with robot 15 poisoned by a NaN position (bit 1), robot 21 with a
    force on a swing foot (bit 0) and robot 31 failed (all-zero forces under four stance feet), tiled on the device (index =
    arange(n) % 130).  Robot i of the large launch equals robot i % 130 of the n = 130 launch of the same kernel - the launch
    test_sizes_contact_patterns_and_inputs holds to the restatement - in every per-robot output, bit for bit, NaN positions
    included.  The summary of the large launch equals the host reduction of its own per-robot arrays (KR.summarize), and its counts
    are the tiled counts.  Then two forces are moved: a normal force of robot n - 1 far above fzmax, the unique worst primal
    residual, and robot 262 144 + 5 becomes the period's worst stationarity robot with one more push, the unique worst stationarity
    residual (both settled on the restatement, asserted there first): arg_primal and arg_stationarity name them - indices beyond
    2^18, found in a second round."""
    import torch
    from quadruped_control_amd.balance_controller import certify_summary

    n, p = 4096 * 64 + 65, 130
    a, c = n - 1, 262144 + 5
    ctl, P = ctls["uniform"], params(q, "uniform")
    b, grf = inputs(p, source)
    b, grf = {k: v.copy() for k, v in b.items()}, grf.copy()
    for k in b:  # (robot n - 1 is period robot 128, contact pattern 0: it gets robot 127's four stance feet)
        b[k][a % p] = b[k][127]
    grf[a % p] = grf[127]
    grf[31] = 0.0                  # fails: fzmin - 0 under four stance feet
    grf[21, 3:6] = (1.0, 0.0, 0.0)  # a force on a swing foot (contact pattern 5): flags bit 0
    ref = KR.certificate(P, b, grf, default_duty=KR.DEFAULT_DUTY)  # (before the poison: the restatement's worst robots are finite ones)
    b["x"][15, 1] = np.nan         # poisoned: flags bit 1
    # the two moved forces, settled on the restatement alone: the period's worst stationarity robot w with one more push, as robot c
    w = int(np.argmax(ref["stationarity"]))
    comp, push = {"feet": (1, -5.0), "joint_q": (0, -5.0)}[source]
    foot_w = [l for l in range(4) if (w >> l) & 1][0]
    moved = grf.copy()
    moved[w, 3 * foot_w + comp] += push
    moved[a % p, 2] -= 1.0e3       # grf_body = -Rwb^T f: the world normal force of foot 0 rises by ~1e3 N, far above fzmax
    ref2 = KR.certificate(P, {k: np.where(np.isnan(v), 0.0, v) if k == "x" else v for k, v in b.items()}, moved, default_duty=KR.DEFAULT_DUTY)
    rest = np.delete(ref["stationarity"], 15)
    assert ref2["stationarity"][w] > rest.max() + 1e-3 > ref2["stationarity"][a % p] + 1e-3, (ref2["stationarity"][w], rest.max(), ref2["stationarity"][a % p])
    assert ref2["primal"][a % p] > 100.0 > 2 * max(np.delete(ref["primal"], 15).max(), ref2["primal"][w])
    dev, g = q.to_device(b), torch.from_numpy(grf).cuda()
    small = ctl.certify_batch(dev, g, want=WANT_ALL, summary=True)
    torch.cuda.synchronize()
    host = {k: small[k].cpu().numpy() for k in ("primal", "stationarity", "flags")}
    s_small = certify_summary(small["summary"])
    assert host["flags"][15] & 2 and host["flags"][21] & 1 and not host["primal"][31] <= 1e-7, (host["flags"][15], host["flags"][21], host["primal"][31])
    assert s_small["n_nonfinite"] == 1 and s_small["n_swing_nonzero"] == 1 and s_small["n_fail"] >= 3
    index = torch.arange(n, device="cuda") % p
    tile = lambda v: v.index_select(0, index).contiguous()
    tiled, gt = {k: tile(v) for k, v in dev.items()}, tile(g)
    big = ctl.certify_batch(tiled, gt, want=WANT_ALL, summary=True)
    torch.cuda.synchronize()
    for k in WANT_ALL:
        bits = lambda t: t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t.contiguous()
        want, got = tile(bits(small[k])), bits(big[k])
        assert got.shape == want.shape and torch.equal(got, want), (k, int((got != want).reshape(n, -1).any(dim=1).nonzero()[0]))
    s_big = certify_summary(big["summary"])
    assert s_big == KR.summarize(big["primal"].cpu().numpy(), big["stationarity"].cpu().numpy(), (big["flags"].cpu().numpy() & 1) != 0)
    tiled_sum = lambda per_robot: int(np.asarray(per_robot)[np.arange(n) % p].sum())
    fail = ~(host["primal"] <= 1e-7) | ~(host["stationarity"] <= 1e-8) | ((host["flags"] & 1) != 0)
    assert s_big["n_fail"] == tiled_sum(fail) and s_big["n_nonfinite"] == tiled_sum((host["flags"] & 2) != 0) == 2017
    assert s_big["n_swing_nonzero"] == tiled_sum((host["flags"] & 1) != 0) == 2017
    # robot c becomes the pushed copy of the period's worst robot, robot n - 1 gets its normal force
    for k, v in tiled.items():
        v[c] = dev[k][w]
    gt[c] = torch.from_numpy(moved[w]).cuda()
    gt[a] = torch.from_numpy(moved[a % p]).cuda()
    got = ctl.certify_batch(tiled, gt, want=("primal", "stationarity", "flags"), summary=True)
    torch.cuda.synchronize()
    s = certify_summary(got["summary"])
    pr, stn = got["primal"].cpu().numpy(), got["stationarity"].cpu().numpy()
    assert s == KR.summarize(pr, stn, (got["flags"].cpu().numpy() & 1) != 0)
    fin = lambda v: np.where(np.isfinite(v), v, -np.inf)
    assert (fin(pr)[a] > np.delete(fin(pr), a)).all() and (fin(stn)[c] > np.delete(fin(stn), c)).all()  # unique worsts
    assert s["arg_primal"] == a == n - 1 and s["arg_stationarity"] == c == 262144 + 5, s
    del big, got, tiled, gt, index, small
    torch.cuda.empty_cache()


def test_inputs_are_left_alone_and_the_result_repeats(q, ctls):
    """Every tensor of the batch and grf_body is bit-identical after the call - gait_phase too, although gait_dt is given: the
    certificate advances no clock - and two calls give identical outputs."""
    import torch

    b, grf = inputs(257, "joint_q")
    b = dict(b, gait_dt=np.full(257, 1.0 / 300.0), joint_qdot=np.zeros((257, 12)))
    dev = q.to_device(b)
    g = torch.from_numpy(grf).cuda()
    before = {k: v.clone() for k, v in dev.items()}
    g0 = g.clone()
    one = {k: v.clone() for k, v in ctls["uniform"].certify_batch(dev, g, want=WANT_ALL).items()}
    two = ctls["uniform"].certify_batch(dev, g, want=WANT_ALL)
    torch.cuda.synchronize()
    for k, v in dev.items():
        assert torch.equal(v.view(torch.uint8), before[k].view(torch.uint8)), k
    assert torch.equal(g.view(torch.uint8), g0.view(torch.uint8))
    for k in one:
        assert torch.equal(one[k].view(torch.uint8), two[k].view(torch.uint8)), k
    ref = KR.certificate(params(q, "uniform"), {k: v for k, v in b.items() if k not in ("gait_dt", "joint_qdot")}, grf)
    assert np.array_equal(two["active"].cpu().numpy(), ref["active"])


# ------------------------------------------------------------------ closed loop
def test_rollout_certifies_every_second_step(q):
    """rollout(steps=6, certify_every=2) on an all-solved batch of 64: three summaries with n_fail == 0, and a final state bit-equal
    to the same rollout without certificates."""
    import torch
    from quadruped_control_amd import workloads
    from quadruped_control_amd.balance_controller import certify_summary

    P = q.cheetah_params()
    b = workloads.config2(n=64)
    R = b["Rwb"].reshape(64, 3, 3)
    pw = np.ascontiguousarray((b["x"][:, None, :] + np.einsum("nij,nlj->nli", R, b["feet"].reshape(64, 4, 3))).reshape(64, 12))
    ctl = q.BalanceController.from_params(P, device=0)
    ends = []
    for every in (None, 2):
        dev = q.to_device(b)
        state, out = ctl.rollout(dev, torch.from_numpy(pw).cuda(), steps=6, dt=1.0 / 300.0, certify_every=every)
        torch.cuda.synchronize()
        ends.append(({k: v.clone() for k, v in state.items()}, out))
    ctl.close()
    assert "certificates" not in ends[0][1]
    certs = ends[1][1]["certificates"]
    assert [k for k, _ in certs] == [0, 2, 4]
    assert (ends[1][1]["status"] == 0).all()
    for _, t in certs:
        s = certify_summary(t)
        assert s["n_fail"] == 0 and s["n_nonfinite"] == 0 and s["worst_stationarity"] < 1e-8, s
    for k in ends[0][0]:
        assert torch.equal(ends[0][0][k].view(torch.uint8), ends[1][0][k].view(torch.uint8)), k
    assert torch.equal(ends[0][1]["grf_body"], ends[1][1]["grf_body"])


def test_rollout_tick_certifies_and_refuses_commander_mode(q):
    """rollout_tick(command=None, certify_every=2): the certificate reads joint_q and the contact rule of the tick; in commander
    mode certify_every raises ValueError before anything is launched."""
    import torch
    from quadruped_control_amd import workloads
    from quadruped_control_amd.balance_controller import certify_summary

    P = q.cheetah_params()
    b = workloads.with_joint_angles(workloads.config2(n=64))
    b.pop("feet", None)
    b["joint_qdot"] = np.zeros((64, 12))
    ctl = q.BalanceController.from_params(P, device=0)
    dev = q.to_device({k: np.ascontiguousarray(v) for k, v in b.items()})
    with pytest.raises(ValueError, match="certify_every"):
        ctl.rollout_tick(dev, {"state": None}, steps=2, dt=1.0 / 300.0, leg_inertia=0.02, certify_every=1)
    state, out = ctl.rollout_tick(dev, None, steps=4, dt=1.0 / 300.0, leg_inertia=0.02, certify_every=2)
    torch.cuda.synchronize()
    ctl.close()
    assert [k for k, _ in out["certificates"]] == [0, 2]
    sums = [certify_summary(t) for _, t in out["certificates"]]
    assert sums[0]["n_fail"] == 0, sums[0]  # (the first tick solves config 2's states; later ones are whatever the plant made of them)
    for s in sums:
        assert s["n_nonfinite"] == 0 and s["n_swing_nonzero"] == 0 and s["arg_stationarity"] >= 0, s


# ------------------------------------------------------------------ refusals
def test_refusals_raise_and_launch_nothing(q, ctls):
    """Each refusal of qc_certify_batch raises from Python with the entry point's prefix and launches nothing: the output tensors
    keep their sentinel."""
    import torch
    from quadruped_control_amd import _lib

    ctl = ctls["uniform"]
    n = 65
    b, grf = inputs(n, "feet")
    dev = q.to_device(b)
    g = torch.from_numpy(grf).cuda()
    out = {"primal": torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda"), "summary": torch.full((56,), 77, dtype=torch.uint8, device="cuda")}

    def refused(batch, grf_body, **kw):
        with pytest.raises(RuntimeError, match=r"qc_certify_batch failed \(-1\): qc_certify_batch:"):
            ctl.certify_batch(batch, grf_body, want=kw.pop("want", ("primal",)), out=kw.pop("out", out), **kw)

    refused(dev, None)
    for k in STATE_KEYS:
        refused({a: v for a, v in dev.items() if a != k}, g)
    refused({a: v for a, v in dev.items() if a != "feet"}, g)
    for name in ("act_tol", "primal_tol", "stat_tol"):
        for bad in (-1e-9, float("nan"), float("inf")):
            refused(dev, g, **{name: bad})
    refused(dev, g, want=(), summary=False, out=None)
    # the struct itself, the handle, `in`, `io` and n: straight on the C ABI
    lib = _lib.load()
    io = _lib.QcCertifyIo()
    lib.qc_default_certify(ctypes.byref(io))
    io.grf_body, io.primal, io.summary = g.data_ptr(), out["primal"].data_ptr(), out["summary"].data_ptr()
    bi = batch_in(dev, STATE_KEYS + ("feet", "stance"))
    assert_raw_refusals(lib.qc_certify_batch, lambda: (ctl._h, n, bi, io), "qc_certify_io", 96, 88,
                        [(out["primal"], SENTINEL, True), (out["summary"], 77, False)])
