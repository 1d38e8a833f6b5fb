"""GPU: qc_sensitivity_swing_batch (csrc/qc_sensitivity_swing.hpp) against the 50-digit restatement
(tests/sensitivity_swing_restatement.py), its mask and flags, its in-place forms, central differences of control_batch(want_torques=True)
itself, tick_autograd against the chain of direct calls and against fused_tick_autograd, and rollout_tick_autograd through a trot.

Batch sizes 1, 15, 16, 17, 257 and 4097: a lane is one (robot, leg) row and a workgroup one wave, so 16 robots fill a wave - tail lanes,
one wave +- 1 robot, many workgroups with the last one partly filled.  The inputs are the restatement's in-reach pool (its first N_REF
robots, repeated), the contact patterns its masks(): all-swing, the two trot diagonals, one swing leg, all-stance and a per-robot mix.

The bar against 50 digits, per output entry: K EPS x condition sum, K = 4 x C_SWING - C_SWING the float64 restatement's own worst
distance, measured on the CPU (tests/test_sensitivity_swing_cpu.py) and never on the device; the factor 4 is the siblings' allowance
for operation order and FMA contraction."""
import ctypes

import numpy as np
import pytest

from tests import leg_plant_adjoint_restatement as LA
from tests import sensitivity_swing_restatement as SW
from tests.device_math_reference import KINS, ODD_KIN
from tests.solved_batch_support import EPS, SENTINEL, assert_raw_refusals, batch_in, params, q  # noqa: F401

pytestmark = pytest.mark.gpu
SIZES = (1, 15, 16, 17, 257, 4097)
N_REF = 65
K_BAR = {k: 4.0 * c for k, c in SW.C_SWING.items()}
K_BAR_OF = {"default": K_BAR, "odd": {k: 4.0 * c for k, c in SW.C_SWING_ODD.items()}}  # (C_SWING_ODD: measured on the CPU at ODD_KIN)
SECOND_ROUND_N, PERIOD = 65536 + 17, 130  # one full second round of the 4096-workgroup grid (16 robots a wave) and four live rows
ALL = SW.OUTPUTS + ("flags",)
SWING_KEYS = ("Rwb", "x", "joint_q", "joint_qdot", "swing_pos", "swing_vel")


@pytest.fixture(scope="module")
def ctl(q):
    c = q.BalanceController.from_params(params(q, "uniform"), device=0)
    c.set_tuning(race=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def odd_ctl(q):
    """a handle of this module's own at ODD_KIN (never set_kinematics on a shared one: the model would leak)"""
    c = q.BalanceController.from_params(params(q, "uniform"), device=0)
    c.set_tuning(race=0)
    c.set_kinematics(**ODD_KIN.handle_arguments())
    yield c
    c.close()


@pytest.fixture(scope="module")
def handles(ctl, odd_ctl):
    return {"default": ctl, "odd": odd_ctl}


def _reference(kin):
    b = {k: v[:N_REF] for k, v in SW.model_pool(kin).items()}
    stance = SW.masks(N_REF)
    tb, ins = SW.cotangent(N_REF), {k: v[:N_REF] for k, v in SW.accumulators(N_REF).items()}
    ref, cond, flags, raw = SW.swing_adjoint_mp(b, stance == 0, tb, kin=kin, **ins)
    assert not flags.any()
    return dict(b=b, stance=stance, tb=tb, ins=ins, ref=ref, cond=cond, raw=raw)


@pytest.fixture(scope="module")
def reference():
    """the 50-digit pass on the first N_REF robots of the pool with every accumulator, once"""
    return _reference(KINS["default"])


@pytest.fixture(scope="module")
def references(reference):
    """the default model's reference and ODD_KIN's (its pool clamped on both sides in every joint), once each"""
    class Lazy(dict):  # (ODD_KIN's pass is built when an odd-model test first asks for it)
        def __missing__(self, model):
            self[model] = _reference(KINS[model])
            return self[model]

    return Lazy(default=reference)


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tile(a, n):
    return np.ascontiguousarray(a[np.arange(n) % a.shape[0]])


def _full(b):
    """the swing pool's arrays with the rest of the state a solve reads: at rest, the desired state the robot's own"""
    n = b["x"].shape[0]
    eye = np.tile(np.eye(3).reshape(9), (n, 1))
    return dict(b, Rwb_d=eye, xdot=np.zeros((n, 3)), w=np.zeros((n, 3)), x_d=b["x"].copy(), xdot_d=np.zeros((n, 3)), w_d=np.zeros((n, 3)))


def _run(q, ctl, b, tb, want=ALL, out=None, **ins):
    import torch

    r = ctl.sensitivity_swing_batch(q.to_device(b), _cuda(tb), want=want, out=out, **{k: _cuda(v) for k, v in ins.items()})
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


@pytest.mark.parametrize("n", SIZES)
def test_against_50_digits(q, handles, references, n):
    """_against_50_digits at the default model (this id is the one the test always had)"""
    _against_50_digits(q, handles, references, n, "default")


@pytest.mark.parametrize("n", SIZES)
def test_against_50_digits_at_the_odd_model(q, handles, references, n):
    """_against_50_digits at ODD_KIN: the same body, the same assertions"""
    _against_50_digits(q, handles, references, n, "odd")


def _against_50_digits(q, handles, references, n, model):
    """Every output within K EPS x condition sum of the 50-digit pass; rows without a contribution (stance legs) equal it exactly.  The
    mask comes from stance bytes, for n = 17 from the phases at the handle's duty and for n = 16 from the phases at a per-robot duty.
    At ODD_KIN (a handle of its own, K from C_SWING_ODD) the pool is clamped at tau_min and at tau_max in every joint and holds
    torques within |kff| of a limit: the device's clamp mask is the 50-digit pass's bit for bit (gain_bar's last three entries are s),
    and gain_bar's nine entries per leg are held like every other output."""
    c, ctl, K_BAR = references[model], handles[model], K_BAR_OF[model]
    b = {k: _tile(v, n) for k, v in c["b"].items()}
    st = _tile(c["stance"], n)
    if n == 17:
        b["gait_phase"] = np.where(st != 0, 0.3, 0.9)
    elif n == 16:
        b["gait_phase"], b["gait_duty"] = np.where(st != 0, 0.3, 0.7), np.full(n, 0.5)
    else:
        b["stance"] = st
    got = _run(q, ctl, b, _tile(c["tb"], n), **{k: _tile(v, n) for k, v in c["ins"].items()})
    assert not got["flags"].any()
    for k in SW.OUTPUTS:
        ref, cond, val = _tile(c["ref"][k], n), _tile(c["cond"][k], n), got[k].reshape((n,) + SW.SIZES[k])
        live = cond > 0
        assert np.array_equal(val[~live], ref[~live]), k
        worst = float(np.max(np.abs(val - ref)[live] / (EPS * cond[live]))) if live.any() else 0.0
        print(f"n={n} {model} {k}: worst {worst:.4f} EPS x condition sum (bar {K_BAR[k]})")
        assert worst <= K_BAR[k], (k, worst)
    kin = KINS[model]
    raw, tb = _tile(c["raw"], n), _tile(c["tb"], n).reshape(n, 4, 3)
    passes = ~(raw < kin.tau_min) & ~(raw > kin.tau_max)  # (raw is NaN for a stance leg: left out below)
    swing = np.isfinite(raw)
    s = got["gain_bar"].reshape(n, 4, 3, 3)[:, :, 2]
    assert np.array_equal(s[swing], np.where(passes, tb, 0.0)[swing])  # the clamp mask, bit for bit


def test_mask_and_flags(q, handles):
    """_mask_and_flags at the default model"""
    _mask_and_flags(q, handles, "default")


def test_mask_and_flags_at_the_odd_model(q, handles):
    """_mask_and_flags at ODD_KIN: the same body, the same assertions"""
    _mask_and_flags(q, handles, "odd")


def _mask_and_flags(q, handles, model):
    """Saturated joints give exact zeros in that component; flagged legs NaN with the expected bits; all-stance zeros, or the `_in`
    arrays, bit for bit.  At ODD_KIN the saturated pool is the one clamped in every joint with torques within |kff| of a limit, and
    the device's clamp mask equals the restatement's bit for bit (the float64 and the 50-digit masks agree: the CPU test)."""
    n, kin, ctl = N_REF, KINS[model], handles[model]
    b = SW.pool(n, saturate=True) if model == "default" else SW.model_pool(kin, n)
    b["stance"] = np.zeros((n, 4), np.uint8)
    tb = SW.cotangent(n)
    _, flags, raw = SW.swing_adjoint_np(b, np.ones((n, 4), bool), tb, kin=kin)
    if model == "default":
        sat = (raw < SW.TAU_MIN - 1.0) | (raw > SW.TAU_MAX + 1.0)
        assert not flags.any() and sat.sum() > n and (np.abs(raw)[~sat] < 19.0).all()  # no torque near a limit: the masks agree
    else:
        sat = (raw < kin.tau_min) | (raw > kin.tau_max)
        near = np.minimum(np.abs(raw - kin.tau_min), np.abs(raw - kin.tau_max))
        assert not flags.any() and all((raw[:, :, j] < kin.tau_min).any() and (raw[:, :, j] > kin.tau_max).any() for j in range(3))
        assert near.min() > 0.05 and all((near[:, :, j] < abs(kin.jc_kff[j])).any() for j in range(3))  # near a limit, 1e13 roundings off it
    got = _run(q, ctl, b, tb)
    assert not got["flags"].any()
    g = got["gain_bar"].reshape(n, 4, 3, 3)
    for name, val in (("joint_q_bar", got["joint_q_bar"]), ("joint_qdot_bar", got["joint_qdot_bar"]), ("kp", g[:, :, 0]), ("kd", g[:, :, 1]), ("kff", g[:, :, 2])):
        val = val.reshape(n, 4, 3)
        assert (val[sat] == 0.0).all() and (val[~sat] != 0.0).all(), name
    assert np.array_equal(g[:, :, 2][~sat], tb.reshape(n, 4, 3)[~sat])  # kff's cotangent is s itself
    # flagged legs
    fb, expect = SW.flagged_pool(kin)
    fb["stance"] = np.zeros((4, 4), np.uint8)
    got = _run(q, ctl, fb, SW.cotangent(4), **SW.accumulators(4))
    assert np.array_equal(got["flags"], expect), got["flags"]
    for i in range(4):
        for k in SW.PER_LEG:
            bad = np.isnan(got[k][i].reshape(SW.SIZES[k])).all(axis=1)
            assert bad.tolist() == [leg == i for leg in range(4)] and np.isfinite(got[k][i].reshape(SW.SIZES[k])[~bad]).all(), (i, k)
        for k in SW.PER_ROBOT:
            assert np.isnan(got[k][i]).all(), (i, k)
    # all stance
    b["stance"] = np.ones((n, 4), np.uint8)
    ins = SW.accumulators(n)
    got = _run(q, ctl, b, tb, **ins)
    bits = lambda a: np.ascontiguousarray(a, np.float64).reshape(-1).view(np.int64)
    for k in SW.OUTPUTS:
        want = ins.get(k + "_in", np.zeros((n,) + SW.SIZES[k]))
        assert np.array_equal(bits(got[k]), bits(want)), k
    got = _run(q, ctl, b, tb)
    assert all(np.array_equal(bits(got[k]), bits(np.zeros((n,) + SW.SIZES[k]))) for k in SW.OUTPUTS) and not got["flags"].any()


def test_second_round_of_the_grid_stride(q, ctl):
    """n = 65 536 + 17 robots, 262 212 rows: the grid is capped at 4096 one-wave workgroups of 16 robots, so workgroup 0 walks a full
    second round and workgroup 1 has four live rows in its second.  The batch is a period of PERIOD robots tiled on the device (index
    = arange(n) % PERIOD): the restatement's pool under its mix of contact masks, four robots with a flagged leg each (flagged_pool)
    and one robot with a NaN position.  Robot i of the large launch equals robot i % PERIOD of the n = PERIOD launch of the same
    kernel - the launch the tests above hold to 50 digits - in every output, bit for bit, NaN positions included: a row's arithmetic
    reads no other lane."""
    import torch

    n, p = SECOND_ROUND_N, PERIOD
    b = SW.pool(p)
    b["stance"] = SW.masks(p)
    fb, expect = SW.flagged_pool()
    for k in fb:
        b[k][40:44] = fb[k]
    b["stance"][40:44] = 0
    b["x"][77, 1] = np.nan
    b["stance"][77] = (1, 0, 0, 1)
    tb, ins = SW.cotangent(p), SW.accumulators(p)
    small = ctl.sensitivity_swing_batch(q.to_device(b), _cuda(tb), want=ALL, **{k: _cuda(v) for k, v in ins.items()})
    torch.cuda.synchronize()
    flags = small["flags"].cpu().numpy()
    assert np.array_equal(flags[40:44], expect) and flags[77] == 0b0110 and np.count_nonzero(flags) == 5, flags
    assert len({tuple(r) for r in b["stance"].tolist()}) > len(SW.PATTERNS)
    index = torch.arange(n, device="cuda") % p
    dev = {k: v.index_select(0, index).contiguous() for k, v in q.to_device(b).items()}
    big = ctl.sensitivity_swing_batch(dev, _cuda(tb).index_select(0, index).contiguous(), want=ALL,
                                      **{k: _cuda(v).index_select(0, index).contiguous() for k, v in ins.items()})
    torch.cuda.synchronize()
    for k in ALL:
        bits = lambda t: t if t.dtype == torch.int32 else t.contiguous().view(torch.int64)
        want, got = bits(small[k]).index_select(0, index), bits(big[k])
        assert got.shape == want.shape and torch.equal(got, want), (k, int((got != want).reshape(n, -1).any(dim=1).nonzero()[0]))
    assert bool(torch.isnan(big["x_bar"][n - 1 - (n - 1 - 77) % p]).all())  # (a poisoned robot of the second round)
    del dev, big, small, index
    torch.cuda.empty_cache()


def test_in_place_and_output_groups(q, ctl, reference):
    """Every `_in` aliased to its output gives the out-of-place bits; rows beyond n keep the sentinel; every output asked for alone, and
    each output group alone, gives the bits of the call that asks for everything."""
    import torch

    c, n = reference, 17
    b = {k: _tile(v, n) for k, v in c["b"].items()}
    b["stance"] = _tile(c["stance"], n)
    tb = _tile(c["tb"], n)
    ins = {k: _tile(v, n) for k, v in c["ins"].items()}
    base = _run(q, ctl, b, tb, **ins)
    whole = {k: torch.full((n + 2,) + SW.SIZES[k], SENTINEL, dtype=torch.float64, device="cuda") for k in SW.OUTPUTS}
    whole["flags"] = torch.full((n + 2,), 77, dtype=torch.int32, device="cuda")
    out = {k: t[:n] for k, t in whole.items()}
    for k in ("joint_q_bar", "Rwb_bar", "x_bar"):
        out[k].copy_(_cuda(ins[k + "_in"]).view_as(out[k]))
    r = ctl.sensitivity_swing_batch(q.to_device(b), _cuda(tb), want=ALL, out=out, **{k + "_in": out[k] for k in ("joint_q_bar", "Rwb_bar", "x_bar")})
    torch.cuda.synchronize()
    for k in ALL:
        assert r[k] is out[k] and np.array_equal(out[k].cpu().numpy().reshape(base[k].shape), base[k], equal_nan=True), k
        assert bool((whole[k][n:] == (77 if k == "flags" else SENTINEL)).all()), k
    for want in [(k,) for k in ALL] + [SW.PER_LEG, SW.PER_ROBOT]:
        got = _run(q, ctl, b, tb, want=want, **ins)
        assert set(got) == set(want) and all(np.array_equal(got[k], base[k]) for k in want), want


DIRECTIONS = {"swing_pos": 12, "swing_vel": 12, "x": 3, "Rwb": 9, "joint_q": 12, "joint_qdot": 12}
FD_H = 1e-6


def test_central_differences_of_control_batch(q, ctl, reference):
    """<gradient, v> of L = <joint_tau_bar, joint_tau of the swing legs> against central differences of control_batch(want_torques=True)
    itself on the CPU test's pool, one committed direction per input; its step and its bar (h = 1e-6; 1e-6 of sum |gradient_i v_i| +
    1e-6: tests/test_sensitivity_swing_cpu.py derives them).  No case is excluded: every torque stays strictly inside the limits."""
    import torch

    c, n = reference, N_REF
    b = _full(dict(c["b"], stance=c["stance"]))
    swing = (c["stance"] == 0)[:, :, None]
    tb = c["tb"].reshape(n, 4, 3)
    grad = _run(q, ctl, b, c["tb"], want=SW.OUTPUTS)
    rng = np.random.default_rng(41)

    def loss(bb):
        tau = ctl.control_batch(q.to_device(bb), want_torques=True)["joint_tau"]
        torch.cuda.synchronize()
        tau = tau.cpu().numpy().reshape(n, 4, 3)
        assert (np.abs(tau[np.broadcast_to(swing, tau.shape)]) < 19.5).all()
        return (np.where(swing, tau, 0.0) * tb).sum(axis=(1, 2))

    excluded = 0
    for name, m in DIRECTIONS.items():
        v = rng.uniform(-1.0, 1.0, (n, m))
        fd = (loss(dict(b, **{name: b[name] + FD_H * v})) - loss(dict(b, **{name: b[name] - FD_H * v}))) / (2 * FD_H)
        g = grad[name + "_bar"].reshape(n, -1)
        an, scale = (g * v).sum(axis=1), (np.abs(g) * np.abs(v)).sum(axis=1)
        err = np.abs(fd - an)
        print(f"FD {name}: worst error {err.max():.3e}, worst error / bar {np.max(err / (1e-6 * scale + 1e-6)):.3f}")
        assert (err <= 1e-6 * scale + 1e-6).all(), (name, float(err.max()))
    assert excluded == 0


def _leaves(q, b, names):
    dev = q.to_device(b)
    for k in names:
        dev[k].requires_grad_(True)
    return dev


def test_tick_autograd(q, ctl, reference):
    """tick_autograd equals the chain of direct calls bit for bit; on an all-stance batch it equals fused_tick_autograd; the joint_gains
    gradient is gain_bar summed over robots and legs."""
    import torch
    from quadruped_control_amd.autograd import TICK_DIFFERENTIABLE, TICK_SWING_DIFFERENTIABLE

    c, n = reference, N_REF
    b = _full(dict(c["b"], stance=c["stance"]))
    rng = np.random.default_rng(43)
    ct, cg = _cuda(rng.normal(0.0, 1.0, (n, 12))), _cuda(rng.normal(0.0, 1.0, (n, 12)))
    dev = _leaves(q, b, TICK_SWING_DIFFERENTIABLE)
    gains = torch.zeros(9, dtype=torch.float64, device="cuda", requires_grad=True)
    tau, grf, status = ctl.tick_autograd(dev, joint_gains=gains)
    plain = ctl.control_batch(q.to_device(b), want_torques=True)
    assert torch.equal(tau, plain["joint_tau"]) and torch.equal(grf, plain["grf_body"]) and torch.equal(status, plain["status"])
    ((tau * ct).sum() + (grf * cg).sum()).backward()
    # the chain of direct calls
    raw = q.to_device(b)
    k = ctl.sensitivity_kinematics_batch(raw, plain["grf_body"], plain["status"], joint_tau_bar=ct, grf_bar_in=cg, want=("grf_bar", "joint_q_bar"))
    s = ctl.sensitivity_batch(raw, plain["grf_body"], k["grf_bar"].view(n, 12), want=("x_bar", "xdot_bar", "w_bar", "x_d_bar", "xdot_d_bar", "w_d_bar", "feet_bar", "b_bar"))
    s.update(ctl.sensitivity_rotation_batch(raw, plain["grf_body"], k["grf_bar"].view(n, 12), s["b_bar"], s["feet_bar"], want=("Rwb_bar", "Rwb_d_bar")))
    s["joint_q_bar"] = ctl.sensitivity_kinematics_batch(raw, feet_bar=s["feet_bar"], joint_q_bar_in=k["joint_q_bar"], want=("joint_q_bar",))["joint_q_bar"]
    s.update(ctl.sensitivity_swing_batch(raw, ct, want=SW.OUTPUTS, joint_q_bar_in=s["joint_q_bar"], Rwb_bar_in=s["Rwb_bar"], x_bar_in=s["x_bar"]))
    torch.cuda.synchronize()
    for name in TICK_SWING_DIFFERENTIABLE:
        assert torch.equal(dev[name].grad.reshape(-1), s[name + "_bar"].reshape(-1)), name
    assert torch.equal(gains.grad, s["gain_bar"].sum(dim=(0, 1))) and bool(gains.grad.abs().min() > 0)
    assert bool(dev["swing_pos"].grad.abs().max() > 0) and bool(dev["joint_qdot"].grad.abs().max() > 0)
    # all stance: the fused stance tick's gradients
    allst = dict(b, stance=np.ones((n, 4), np.uint8))
    dev = _leaves(q, allst, TICK_SWING_DIFFERENTIABLE)
    tau, grf, _ = ctl.tick_autograd(dev)
    ((tau * ct).sum() + (grf * cg).sum()).backward()
    fused = _leaves(q, {k: v for k, v in allst.items() if k not in ("joint_qdot", "swing_pos", "swing_vel")}, TICK_DIFFERENTIABLE)
    tau_f, grf_f, _ = ctl.fused_tick_autograd(fused)
    ((tau_f * ct).sum() + (grf_f * cg).sum()).backward()
    assert torch.equal(tau, tau_f) and torch.equal(grf, grf_f)
    for name in TICK_DIFFERENTIABLE:
        assert torch.equal(dev[name].grad, fused[name].grad), name
    assert all(not bool(dev[name].grad.any()) for name in ("joint_qdot", "swing_pos", "swing_vel"))
    with pytest.raises(ValueError, match="tick_autograd: the batch carries gait_dt"):
        ctl.tick_autograd(dict(dev, gait_dt=dev["x"]))
    with pytest.raises(ValueError, match="tick_autograd: the batch lacks"):
        ctl.tick_autograd({k: t for k, t in dev.items() if k != "swing_vel"})


def test_tick_autograd_at_the_odd_model_against_central_differences(q, odd_ctl):
    """The composed check at ODD_KIN: tick_autograd on this module's odd handle, a trot mask (the two diagonals in turn, n = 17, the swing
    references held LIFT above the model's own feet), against central differences of control_batch(want_torques=True) along the
    rollout test's committed kind of directions (joint_q, x, swing_pos), with its step (SW.ROLLOUT_H), its keep rule - solved, no
    sensitivity or swing flag, the working set and the clamp mask of the tick unchanged at -2h, -h, h, 2h - and its bar, |FD(h) -
    FD(2h)| + 1e-5 |gradient| |direction|.  The kept share is at least 0.5."""
    import torch
    from quadruped_control_amd.autograd import TICK_SWING_DIFFERENTIABLE

    n, h = 17, SW.ROLLOUT_H
    b = SW.trot_start(n, ODD_KIN)
    rng = np.random.default_rng(0x0DD)
    ct, cg = rng.normal(0.0, 1.0, (n, 12)), rng.normal(0.0, 1.0, (n, 12))
    v = {k: rng.normal(0.0, 1.0, b[k].shape) for k in SW.ROLLOUT_DIRECTIONS}
    lo, hi = ODD_KIN.tau_min, ODD_KIN.tau_max

    def tick(k):
        bb = dict(b, **{name: np.ascontiguousarray(b[name] + k * h * v[name]) for name in v})
        _, out = odd_ctl.rollout_tick(q.to_device(bb), None, 1, LA.DT, LA.STAND_INERTIA)
        tau, grf = out["joint_tau"].cpu().numpy(), out["grf_body"].cpu().numpy()
        return (tau * ct + grf * cg).sum(axis=1), out["active_set"].cpu().numpy(), out["status"].cpu().numpy(), (tau <= lo) | (tau >= hi)

    L0, w0, st0, cl0 = tick(0)
    dev = _leaves(q, b, TICK_SWING_DIFFERENTIABLE)
    tau, grf, status = odd_ctl.tick_autograd(dev)
    plain = odd_ctl.control_batch(q.to_device(b), want_torques=True)
    assert torch.equal(tau, plain["joint_tau"]) and np.array_equal(((tau.detach().cpu().numpy() * ct) + grf.detach().cpu().numpy() * cg).sum(axis=1), L0)
    keep = st0 == 0
    keep &= odd_ctl.sensitivity_batch(q.to_device(b), plain["grf_body"], torch.ones_like(plain["grf_body"]), want=("flags",))["flags"].cpu().numpy() == 0
    keep &= odd_ctl.sensitivity_swing_batch(q.to_device(b), torch.ones_like(plain["joint_tau"]), want=("flags",))["flags"].cpu().numpy() == 0
    pts = {k: tick(k) for k in (-2, -1, 1, 2)}
    for _, wk, stk, clk in pts.values():
        keep &= (stk == 0) & (wk == w0) & (clk == cl0).all(axis=1)
    print("kept", keep.mean(), "entries at the clamp at the base point:", int(cl0.sum()))
    assert keep.mean() >= 0.5, keep.mean()
    kept = _cuda(keep.astype(np.float64))[:, None]
    ((tau * _cuda(ct) + grf * _cuda(cg)) * kept).sum().backward()
    torch.cuda.synchronize()
    g = {name: dev[name].grad.cpu().numpy() for name in v}
    fd1, fd2 = (pts[1][0] - pts[-1][0]) / (2 * h), (pts[2][0] - pts[-2][0]) / (4 * h)
    an = sum((g[name] * v[name]).sum(axis=1) for name in v)
    scale = np.sqrt(sum((g[name] ** 2).sum(axis=1) for name in v)) * np.sqrt(sum((v[name] ** 2).sum(axis=1) for name in v))
    err, t = np.abs(fd1 - an), np.abs(fd1 - fd2)
    print("worst relative error", float((err[keep] / scale[keep]).max()), "worst t", float((t[keep] / scale[keep]).max()))
    assert (scale[keep] > 0).all() and bool(np.abs(g["swing_pos"][keep]).max() > 0)
    assert np.all(err[keep] <= t[keep] + 1e-5 * scale[keep])


def test_rollout_tick_autograd_through_a_trot(q):
    """rollout_tick_autograd on a trot mask with held references: the forward values are rollout_tick(batch, None, ...)'s bit for bit; the
    gradient in the start state (joint_q, x) and in swing_pos against central differences of rollout_tick under fd_support's keep
    rule - solved, no sensitivity flag, no plant flag, the working set and the clamp mask of every step unchanged at every point -
    with the leg-plant test's bar, |FD(h) - FD(2h)| + 1e-5 |gradient| |direction|.  The kept share is at least 0.5; the start
    (SW.trot_start) was chosen on the CPU, where the CPU loop alone keeps 0.985 (SW.cpu_rollout_kept, printed here)."""
    import torch

    P = params(q, "uniform")
    n, H, h = SW.ROLLOUT_N, SW.ROLLOUT_STEPS, SW.ROLLOUT_H
    b, c, v = SW.rollout_case()
    cpu_kept = SW.cpu_rollout_kept(P)
    print("kept by the CPU loop alone:", cpu_kept.mean())
    assert cpu_kept.mean() > 0.5
    lo, hi = LA.tau_limits()
    ctl = q.BalanceController.from_params(P, device=0)
    ctl.set_tuning(race=0)

    def rollout(k):
        start = dict(b, **{name: np.ascontiguousarray(b[name] + k * h * v[name]) for name in v})
        words, status, clamp, flags = [], [], [], []
        for steps in range(1, H + 1):  # (the last tick of an s-step rollout is step s - 1's)
            state, out = ctl.rollout_tick(q.to_device(start), None, steps, LA.DT, LA.STAND_INERTIA)
            words.append(out["active_set"].cpu().numpy())
            status.append(out["status"].cpu().numpy())
            tau = out["joint_tau"].cpu().numpy()
            clamp.append((tau <= lo) | (tau >= hi))
            flags.append(out["flags"].cpu().numpy())
        final = {name: state[name].cpu().numpy() for name in SW.STATE}
        return sum((final[name] * c[name]).sum(axis=1) for name in SW.STATE), np.array(words), np.array(status), np.array(clamp), np.array(flags), final

    L0, w0, st0, cl0, fl0, final0 = rollout(0)
    keep = (st0 == 0).all(axis=0) & (fl0 == 0).all(axis=0)
    _, rec = ctl.rollout_tick(q.to_device(b), None, H, LA.DT, LA.STAND_INERTIA, record_every=1)
    for _, hist in rec["history"]:
        bk = dict(q.to_device(b), **{name: hist[name] for name in SW.STATE})
        o = ctl.control_batch(bk, want_torques=True)
        keep &= ctl.sensitivity_batch(bk, o["grf_body"], torch.ones_like(o["grf_body"]), want=("flags",))["flags"].cpu().numpy() == 0
        keep &= ctl.sensitivity_swing_batch(bk, torch.ones_like(o["joint_tau"]), want=("flags",))["flags"].cpu().numpy() == 0
    pts = {k: rollout(k) for k in (-2, -1, 1, 2)}
    for Lk, wk, stk, clk, flk, _ in pts.values():
        keep &= (stk == 0).all(axis=0) & (wk == w0).all(axis=0) & (clk == cl0).all(axis=(0, 2)) & (flk == 0).all(axis=0)
    print("kept", keep.mean(), "entries at the clamp at the base point:", int(cl0.sum()))

    dev = q.to_device(b)
    for name in v:
        dev[name].requires_grad_(True)
    before = {name: t.detach().clone() for name, t in dev.items()}
    state, out = ctl.rollout_tick_autograd(dev, H, LA.DT, LA.STAND_INERTIA)
    for name in SW.STATE:
        assert np.array_equal(state[name].detach().cpu().numpy(), final0[name]), name  # forward: ctl.rollout_tick's bits
    assert torch.equal(out["active_set"], torch.from_numpy(w0[-1]).cuda()) and np.array_equal(out["flags"].cpu().numpy(), fl0[-1])
    assert all(torch.equal(dev[name].detach(), before[name]) for name in dev)  # `batch` is not modified
    assert keep.mean() >= 0.5, keep.mean()
    kept = torch.from_numpy(keep.astype(np.float64)).cuda()[:, None]
    sum((state[name] * torch.from_numpy(c[name]).cuda() * kept).sum() for name in SW.STATE).backward()
    torch.cuda.synchronize()
    g = {name: dev[name].grad.cpu().numpy() for name in v}
    fd1, fd2 = (pts[1][0] - pts[-1][0]) / (2 * h), (pts[2][0] - pts[-2][0]) / (4 * h)
    an = sum((g[name] * v[name]).sum(axis=1) for name in v)
    scale = np.sqrt(sum((g[name] ** 2).sum(axis=1) for name in v)) * np.sqrt(sum((v[name] ** 2).sum(axis=1) for name in v))
    err, t = np.abs(fd1 - an), np.abs(fd1 - fd2)
    rel = lambda a: float((a[keep] / scale[keep]).max())
    print("worst relative error", rel(err), "worst t", rel(t), "worst error beyond t", rel(np.maximum(err - t, 0.0)))
    assert (scale[keep] > 0).all() and bool(np.abs(g["swing_pos"][keep]).max() > 0)
    assert np.all(err[keep] <= t[keep] + 1e-5 * scale[keep])
    assert not any(g[name][~keep].any() for name in v)
    for key in ("gait_dt", "swing_state", "feet"):
        with pytest.raises(ValueError, match=f"rollout_tick_autograd: the batch carries {key}"):
            ctl.rollout_tick_autograd(dict(dev, **{key: dev["x"]}), H, LA.DT, LA.STAND_INERTIA)
    with pytest.raises(ValueError, match="swing_pos and swing_vel go together"):
        ctl.rollout_tick_autograd({k: t for k, t in dev.items() if k != "swing_vel"}, H, LA.DT, LA.STAND_INERTIA)
    ctl.close()


def test_refusals_launch_nothing(q, ctl, reference):
    """Every refusal of qc_sensitivity_swing_batch returns -1 with its prefix and leaves the guarded outputs as they were; n == 0 launches
    nothing; the same structs, valid, do launch."""
    import torch
    from quadruped_control_amd import _lib

    c, n = reference, 17
    lib = _lib.load()
    b = {k: _tile(v, n) for k, v in c["b"].items()}
    b["stance"] = np.zeros((n, 4), np.uint8)
    dev = q.to_device(b)
    tb = _cuda(_tile(c["tb"], n))
    outs = {k: torch.full((n,) + SW.SIZES[k], SENTINEL, dtype=torch.float64, device="cuda") for k in SW.OUTPUTS}
    flags = torch.full((n,), 77, dtype=torch.int32, device="cuda")

    def io():
        s = _lib.QcSensitivitySwingIo()
        lib.qc_default_sensitivity_swing(ctypes.byref(s))
        s.joint_tau_bar = tb.data_ptr()
        for k, t in outs.items():
            setattr(s, k, t.data_ptr())
        s.flags = flags.data_ptr()
        return s

    keys = SWING_KEYS + ("stance",)
    guards = [(t, SENTINEL, True) for t in outs.values()] + [(flags, 77, True)]

    def refused(what, bi, s):
        rc = lib.qc_sensitivity_swing_batch(ctl._h, n, ctypes.byref(bi), ctypes.byref(s), None)
        assert rc == -1 and _lib.last_error().startswith("qc_sensitivity_swing_batch:"), (what, rc, _lib.last_error())
        torch.cuda.synchronize()
        assert all(bool((t == sentinel).all()) for t, sentinel, _ in guards), what

    for missing in SWING_KEYS:
        refused("no " + missing, batch_in(dev, [k for k in keys if k != missing]), io())
    extra = batch_in(dev, keys)
    extra.swing_state = dev["x"].data_ptr()
    refused("swing_state", extra, io())
    extra = batch_in(dev, keys)
    extra.gait_dt = dev["x"].data_ptr()
    refused("gait_dt", extra, io())
    s = io()
    s.joint_tau_bar = None
    refused("no joint_tau_bar", batch_in(dev, keys), s)
    s = _lib.QcSensitivitySwingIo()
    lib.qc_default_sensitivity_swing(ctypes.byref(s))
    s.joint_tau_bar = tb.data_ptr()
    refused("no output", batch_in(dev, keys), s)
    with pytest.raises(ValueError, match="^qc_sensitivity_swing_batch: gait_dt"):
        ctl.sensitivity_swing_batch(dict(dev, gait_dt=dev["x"][:, 0].contiguous()), tb)
    with pytest.raises(ValueError, match="unknown output"):
        ctl.sensitivity_swing_batch(dev, tb, want=("grf_bar",))
    assert_raw_refusals(lib.qc_sensitivity_swing_batch, lambda: (ctl._h, n, batch_in(dev, keys), io()), "qc_sensitivity_swing_io",
                        ctypes.sizeof(_lib.QcSensitivitySwingIo), ctypes.sizeof(_lib.QcSensitivityKinIo), guards)
