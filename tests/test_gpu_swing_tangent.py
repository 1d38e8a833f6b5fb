"""GPU: qc_swing_torque_tangent_batch (csrc/qc_swing_tangent.hpp) against the restatement (tests/swing_tangent_restatement.py), its
NULL tangents and in-place forms, the grid cap, the pairing with the device's adjoint, the chain behind torque_tangent() against
central differences of control_batch(want_torques=True), the flagged legs, rollout_swing_tangent() and rollout_swing_transition()
through a trot, and the refusals.

A lane is one (direction, robot, leg) row and a workgroup one wave: 16 robots of one direction fill a wave, so n in {1, 63, 64, 65, 130}
x K in {1, 3} puts tail lanes, whole waves and a direction boundary inside a wave on the grid.  Every array carries sentinel rows
behind its last row.  Two handles: the default kinematics, and ODD_KIN - the swing tests' model, whose pool is clamped on both sides
in every joint.

The bar against the restatement, per entry: 4 x C_ST x EPS x condition sum - C_ST the float64 restatement's own worst distance from
50 digits, measured on the CPU (tests/test_swing_tangent_cpu.py) and never on the device; the factor 4 is the siblings' allowance for
operation order and FMA contraction."""
import ctypes

import numpy as np
import pytest

from tests import leg_plant_adjoint_restatement as LA
from tests import leg_plant_tangent_restatement as LT
from tests import sensitivity_swing_restatement as SW
from tests import swing_tangent_restatement as ST
from tests import tangent_restatement as QR
from tests.device_math_reference import KINS, ODD_KIN
from tests.gpu_arrays import SENTINEL, _device_arrays, _tile, assert_same_bits
from tests.solved_batch_support import EPS, assert_raw_refusals, batch_in, params, q  # noqa: F401

pytestmark = pytest.mark.gpu
N_REF, K_REF = 65, 3
SHAPES = tuple((n, K) for n in (1, 63, 64, 65, 130) for K in (1, 3))
SWING_KEYS = ("Rwb", "x", "joint_q", "joint_qdot", "swing_pos", "swing_vel")
STATE = LA.INPUTS[:-1]
DT = LA.DT


def _header_constant(name):
    """`constexpr int name = value;` of csrc/qc_swing_tangent.hpp"""
    import os
    import re

    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "quadruped_control_amd", "csrc", "qc_swing_tangent.hpp")).read()
    return int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))


CAP_ROWS = _header_constant("SWING_TANGENT_MAX_BLOCKS") * _header_constant("SWING_TANGENT_BLOCK")


@pytest.fixture(scope="module")
def handles(q):
    """the default kinematics, and a handle of this module's own at ODD_KIN (never set_kinematics on a shared one)"""
    out = {}
    for model in ("default", "odd"):
        c = q.BalanceController.from_params(params(q, "uniform"), device=0)
        c.set_tuning(race=0)
        if model == "odd":
            c.set_kinematics(**ODD_KIN.handle_arguments())
        out[model] = c
    yield out
    for c in out.values():
        c.close()


def _reference(kin, n=N_REF, K=K_REF, seed=47):
    b = {k: v[:n] for k, v in SW.model_pool(kin).items()}
    stance = SW.masks(n)
    tans = ST.random_tangents(n, K, seed)
    val, flags, raw = ST.swing_tangent_np(b, stance == 0, tans, kin=kin)
    cond = ST._swing_tangent(ST._Mp, b, stance == 0, tans, "jacobian", kin)[1]
    assert not flags.any()
    return dict(b=b, stance=stance, tans=tans, ref=val, cond=cond, raw=raw)


@pytest.fixture(scope="module")
def references():
    """per model, once: swing_tangent_np on the first N_REF robots of the pool, K_REF seeded directions, and the condition sums"""
    class Lazy(dict):
        def __missing__(self, key):
            import mpmath as mp

            with mp.workdps(ST.DPS):
                self[key] = _reference(KINS[key]) if isinstance(key, str) else _reference(KINS[key[0]], SW.POOL, 1, 67)
            return self[key]

    return Lazy()


def _contact(stance, way):
    """the contact mask given the ways the adjoint's tests give it: stance bytes, phases at the handle's duty, phases at a per-robot duty"""
    if way == "stance":
        return {"stance": stance}
    if way == "gait_phase":
        return {"gait_phase": np.where(stance != 0, 0.3, 0.9)}
    return {"gait_phase": np.where(stance != 0, 0.3, 0.7), "gait_duty": np.full(stance.shape[0], 0.5)}


def _call(ctl, b, tans, n, K, given=None, zeros=False, alias=None, want=("joint_tau_tan", "flags")):
    """One swing-tangent call over n robots and K directions (b: host arrays of n rows, the contact inputs among them; tans: {name:
    [K, n, m]}), every array with sentinel rows behind its last row.  given: the tangents handed over (default all; the others NULL,
    or zeros with zeros=True); alias: the tangent joint_tau_tan is written over.  Returns (joint_tau_tan host [K n + 2, 12] or None,
    flags [n + 2] or None, {array: host after the call}, {array: host before})."""
    import torch

    from quadruped_control_amd import tangent as T

    given = tuple(tans) if given is None else given
    d = _device_arrays(b, n)
    flat = {k: np.ascontiguousarray(np.asarray(v).reshape(K * n, -1)) for k, v in tans.items()}
    host = {k: (v if k in given else np.zeros_like(v)) for k, v in flat.items() if k in given or zeros}
    td = _device_arrays(host, K * n)
    before = {**{k: v[0].cpu().numpy() for k, v in d.items()}, **{k: v[0].cpu().numpy() for k, v in td.items()}}
    out = {}
    target = None
    if "joint_tau_tan" in want:
        target = td[alias] if alias else _device_arrays({"joint_tau_tan": np.full((1, 12), SENTINEL)}, K * n)["joint_tau_tan"]
        out["joint_tau_tan"] = target[1]
    flags = torch.full((n + 2,), -77, dtype=torch.int32, device="cuda")
    if "flags" in want:
        out["flags"] = flags[:n]
    T.swing_torque_tangent(ctl, {k: v[1] for k, v in d.items()}, {k: v[1].reshape((K, n, -1)) for k, v in td.items()}, want=want, out=out)
    torch.cuda.synchronize()
    after = {**{k: v[0].cpu().numpy() for k, v in d.items()}, **{k: v[0].cpu().numpy() for k, v in td.items()}}
    return (None if target is None else target[0].cpu().numpy()), flags.cpu().numpy(), after, before


def _tiled_case(c, n, K):
    b = {k: _tile(v, n) for k, v in c["b"].items()}
    tans = {k: np.ascontiguousarray(np.stack([_tile(v[d], n) for d in range(K)])) for k, v in c["tans"].items()}
    ref = np.stack([_tile(c["ref"][d], n) for d in range(K)]).reshape(K * n, 12)
    cond = np.stack([_tile(c["cond"][d], n) for d in range(K)]).reshape(K * n, 12)
    return b, _tile(c["stance"], n), tans, ref, cond


def _worst(got, ref, cond, rows):
    live = cond > 0
    assert np.array_equal(got[:rows][~live], ref[~live]) and (got[rows:] == SENTINEL).all()
    return float(np.max(np.abs(got[:rows] - ref)[live] / (EPS * cond[live])))


# ------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("model", ("default", "odd"))
def test_against_the_restatement(handles, references, model):
    """Every entry within 4 C_ST EPS x condition sum of swing_tangent_np, zero-condition entries (stance rows, clamped entries) bit-equal:
    n in {1, 63, 64, 65, 130} x K in {1, 3} over the tiled pool.  Worst ratios on the MI355X (profiles/swing_tangent.md): 0.909 at the default model, 0.662 at the odd one."""
    c, bar = references[model], 4.0 * ST.C_ST[model]
    worst = 0.0
    for n, K in SHAPES:
        b, stance, tans, ref, cond = _tiled_case(c, n, K)
        got, flags, after, before = _call(handles[model], dict(b, stance=stance), tans, n, K)
        assert not flags[:n].any() and flags[n:].tolist() == [-77, -77]
        assert all(np.array_equal(after[k], before[k], equal_nan=True) for k in after)  # the inputs and their sentinels stay intact
        w = _worst(got, ref, cond, K * n)
        print(f"{model} n={n} K={K}: worst {w:.4f} EPS x condition sum (bar {bar})")
        assert w <= bar, (n, K, w)
        worst = max(worst, w)
    kin = KINS[model]
    clamped = ((c["raw"] < kin.tau_min) | (c["raw"] > kin.tau_max)).any()
    assert clamped == (model == "odd")
    print(f"{model}: worst over the shapes {worst:.4f}")


@pytest.mark.parametrize("way", ("stance", "gait_phase", "gait_duty"))
def test_the_pool_with_the_contact_mask_given_in_every_way(handles, references, way):
    """The 257-robot pool, one direction, the mask from stance bytes, from the phases at the handle's duty and from the phases at a
    per-robot duty: the same bar."""
    c, n = references[("default", "pool")], SW.POOL
    got, flags, _, _ = _call(handles["default"], dict(c["b"], **_contact(c["stance"], way)), c["tans"], n, 1)
    assert not flags[:n].any()
    w = _worst(got, c["ref"].reshape(n, 12), c["cond"].reshape(n, 12), n)
    print(f"pool, mask by {way}: worst {w:.4f} EPS x condition sum (bar {4.0 * ST.C_ST['default']})")
    assert w <= 4.0 * ST.C_ST["default"], w


# ------------------------------------------------------------------ 2. NULL tangents, in place
@pytest.mark.parametrize("n,K", ((17, 3), (64, 1)))
def test_null_tangents_and_in_place(handles, references, n, K):
    """Each input tangent alone with the others NULL equals the same call with explicit zeros, bit for bit; joint_tau_tan written over
    joint_tau_tan_in, over joint_q_tan and over swing_pos_tan equals the call beside them; sentinels and the inputs of `in` stay."""
    c, ctl = references["odd"], handles["odd"]
    b, stance, tans, _, _ = _tiled_case(c, n, K)
    b = dict(b, stance=stance)
    base, _, _, _ = _call(ctl, b, tans, n, K)
    for name in ST.TANGENTS:
        alone, _, after, before = _call(ctl, b, tans, n, K, given=(name,))
        zeros, _, _, _ = _call(ctl, b, tans, n, K, given=(name,), zeros=True)
        assert np.array_equal(alone.view(np.int64), zeros.view(np.int64)), name
        assert (alone[K * n:] == SENTINEL).all() and all(np.array_equal(after[k], before[k]) for k in after), name
        assert np.isfinite(alone[:K * n]).all() and (name == "joint_tau_tan_in" or not np.array_equal(alone, base))
    for name in ("joint_tau_tan_in", "joint_q_tan", "swing_pos_tan"):
        over, _, after, before = _call(ctl, b, tans, n, K, alias=name)
        assert np.array_equal(over.view(np.int64), base.view(np.int64)), name  # (the sentinel rows behind the last row included)
        assert all(np.array_equal(after[k], before[k]) for k in after if k != name), name


# ------------------------------------------------------------------ 3. past the grid cap
def test_past_the_block_cap(handles):
    """The smallest n at K = 3 whose 4 n K rows exceed SWING_TANGENT_MAX_BLOCKS x SWING_TANGENT_BLOCK - by less than two waves -, so the
    grid strides and the second round's only wave is mostly tail lanes: one launch equals, row for row and bit for bit, the same
    robots run one direction per launch (uncapped pieces)."""
    import torch

    from quadruped_control_amd import tangent as T

    K = 3
    n = CAP_ROWS // (4 * K) + 1
    assert 4 * (n - 1) * K <= CAP_ROWS < 4 * n * K < CAP_ROWS + 128 and 4 * n <= CAP_ROWS
    pool = SW.pool(130, saturate=True)
    dev = {k: torch.from_numpy(_tile(v, n)).cuda() for k, v in dict(pool, stance=SW.masks(130)).items()}
    g = torch.Generator(device="cuda").manual_seed(0x5719)
    tans = {k: torch.randn((K, n, m), generator=g, dtype=torch.float64, device="cuda") for k, m in ST.TANGENTS.items()}
    big = T.swing_torque_tangent(handles["default"], dev, tans, want=("joint_tau_tan", "flags"))
    for d in range(K):
        one = T.swing_torque_tangent(handles["default"], dev, {k: v[d:d + 1].contiguous() for k, v in tans.items()}, want=("joint_tau_tan", "flags"))
        assert_same_bits(big["joint_tau_tan"][d], one["joint_tau_tan"][0], f"joint_tau_tan, direction {d}")
        assert torch.equal(big["flags"], one["flags"])
    assert bool(torch.isfinite(big["joint_tau_tan"]).all()) and bool((big["joint_tau_tan"][:, -1] != 0).any()) and not bool(big["flags"].any())


# ------------------------------------------------------------------ 4. the pairing with the device's adjoint
@pytest.mark.parametrize("model", ("default", "odd"))
def test_pairing_with_the_device_adjoint(q, handles, references, model):
    """<joint_tau_bar, dtau - joint_tau_tan_in> = <swing_pos_bar, dpos> + <swing_vel_bar, dvel> + <joint_q_bar, dq> + <joint_qdot_bar,
    dqdot> + <x_bar, dx> + <Rwb_bar, [delta]x Rwb> with ctl.sensitivity_swing_batch's cotangents, within 4 C_SDOT EPS x the magnitudes
    of all terms on both sides."""
    import torch

    c, ctl, n = references[model], handles[model], N_REF
    b = dict(c["b"], stance=c["stance"])
    tb = SW.cotangent(n)
    got, _, _, _ = _call(ctl, b, c["tans"], n, K_REF)
    bars = ctl.sensitivity_swing_batch(q.to_device(b), torch.from_numpy(tb).cuda(), want=SW.OUTPUTS)
    torch.cuda.synchronize()
    bars = {k: v.cpu().numpy() for k, v in bars.items()}
    lhs, rhs, terms = ST.pairing(tb, got[:K_REF * n].reshape(K_REF, n, 12), c["tans"], bars, b["Rwb"])
    live = (c["stance"] == 0).any(axis=1)
    assert np.array_equal(lhs[:, ~live], rhs[:, ~live]) and (np.abs(lhs[:, live]) > 0).all()
    worst = float(np.max(np.abs(lhs - rhs)[:, live] / (EPS * terms[:, live])))
    print(f"{model}: pairing, worst {worst:.4f} EPS x term magnitudes (bar {4.0 * ST.C_SDOT[model]})")
    assert worst <= 4.0 * ST.C_SDOT[model], worst


# ------------------------------------------------------------------ 5. the chain behind torque_tangent()
def _trot_ctl(q):
    c = q.BalanceController.from_params(params(q, "uniform"), device=0)
    c.set_tuning(race=0)
    return c


def test_chain_identity_against_central_differences_of_control_batch(q):
    """On a trot mask (SW.rollout_case's start), tangent_batch() -> torque_tangent() -> swing_torque_tangent() in place gives the tangent
    of control_batch(want_torques=True)'s complete joint_tau along the committed directions in joint_q, x and swing_pos: <ct, joint_tau_tan>
    against central differences, with the rule, the bar and the kept-share cap of the trot test of tests/test_gpu_sensitivity_swing.py -
    solved, no sensitivity or swing flag, the working set and the clamp mask unchanged at -2h, -h, h, 2h; |FD(h) - FD(2h)| + 1e-5
    |gradient| |direction| (the gradient from tick_autograd, for the scale alone); kept >= 0.5."""
    import torch

    from quadruped_control_amd import tangent as T
    from quadruped_control_amd.autograd import TICK_SWING_DIFFERENTIABLE

    ctl = _trot_ctl(q)
    n, h = SW.ROLLOUT_N, SW.ROLLOUT_H
    b, _, v = SW.rollout_case()
    ct = np.random.default_rng(0x7A41).normal(0.0, 1.0, (n, 12))
    lo, hi = LA.tau_limits()

    def tick(k):
        bb = dict(b, **{name: np.ascontiguousarray(b[name] + k * h * v[name]) for name in v})
        _, out = ctl.rollout_tick(q.to_device(bb), None, 1, DT, LA.STAND_INERTIA)
        tau = out["joint_tau"].cpu().numpy()
        return (tau * ct).sum(axis=1), out["active_set"].cpu().numpy(), out["status"].cpu().numpy(), (tau <= lo) | (tau >= hi)

    L0, w0, st0, cl0 = tick(0)
    dev = q.to_device(b)
    plain = ctl.control_batch(dev, want_torques=True)
    keep = st0 == 0
    keep &= ctl.sensitivity_batch(dev, plain["grf_body"], torch.ones_like(plain["grf_body"]), want=("flags",))["flags"].cpu().numpy() == 0
    seeds = {name + "_tan": torch.from_numpy(np.ascontiguousarray(a)).cuda() for name, a in v.items()}
    solve = T.tangent_batch(ctl, {k: t for k, t in dev.items() if k not in ("joint_qdot", "swing_pos", "swing_vel")}, plain["grf_body"],
                            {k: seeds[k] for k in ("joint_q_tan", "x_tan")}, want=("grf_tan", "flags"))
    tau_tan = T.torque_tangent(ctl, dev, plain["grf_body"], plain["status"], {"grf_tan": solve["grf_tan"], "joint_q_tan": seeds["joint_q_tan"]})["joint_tau_tan"]
    swing_rows = torch.from_numpy(np.repeat(b["stance"] == 0, 3, axis=1)).cuda()
    assert not bool(tau_tan.reshape(n, 12)[swing_rows].any())  # exact zeros in the swing rows
    stance_part = tau_tan.clone()
    res = T.swing_torque_tangent(ctl, dev, dict(seeds, joint_tau_tan_in=tau_tan), want=("joint_tau_tan", "flags"),
                                 out={"joint_tau_tan": tau_tan, "flags": torch.zeros((n,), dtype=torch.int32, device="cuda")})
    torch.cuda.synchronize()
    assert res["joint_tau_tan"].data_ptr() == tau_tan.data_ptr()
    assert torch.equal(tau_tan.reshape(n, 12)[~swing_rows], stance_part.reshape(n, 12)[~swing_rows]) and bool(tau_tan.reshape(n, 12)[swing_rows].any())
    keep &= (solve["flags"].cpu().numpy() == 0) & (res["flags"].cpu().numpy() == 0)
    pts = {k: tick(k) for k in (-2, -1, 1, 2)}
    for _, wk, stk, clk in pts.values():
        keep &= (stk == 0) & (wk == w0) & (clk == cl0).all(axis=1)
    print("kept", keep.mean(), "entries at the clamp at the base point:", int(cl0.sum()))
    assert keep.mean() >= 0.5, keep.mean()
    leaves = q.to_device(b)
    for k in TICK_SWING_DIFFERENTIABLE:
        leaves[k].requires_grad_(True)
    tau, _, _ = ctl.tick_autograd(leaves)
    (tau * torch.from_numpy(ct).cuda()).sum().backward()
    g = {name: leaves[name].grad.cpu().numpy() for name in v}
    an = (tau_tan.cpu().numpy().reshape(n, 12) * ct).sum(axis=1)
    fd1, fd2 = (pts[1][0] - pts[-1][0]) / (2 * h), (pts[2][0] - pts[-2][0]) / (4 * h)
    scale = np.sqrt(sum((g[name] ** 2).sum(axis=1) for name in v)) * np.sqrt(sum((v[name] ** 2).sum(axis=1) for name in v))
    err, t = np.abs(fd1 - an), np.abs(fd1 - fd2)
    print("worst relative error", float((err[keep] / scale[keep]).max()), "worst t", float((t[keep] / scale[keep]).max()))
    assert (scale[keep] > 0).all() and np.all(err[keep] <= t[keep] + 1e-5 * scale[keep])
    ctl.close()


# ------------------------------------------------------------------ 6. flagged legs
@pytest.mark.parametrize("model", ("default", "odd"))
def test_flagged_legs(handles, model):
    """SW.flagged_pool(): the expected bits; NaN in the flagged leg's row in all K directions whatever joint_tau_tan_in holds, the other
    legs finite; a flags-only call gives the same word and writes nothing else."""
    kin, K = KINS[model], 3
    fb, expect = SW.flagged_pool(kin)
    b = dict(fb, stance=np.zeros((4, 4), np.uint8))
    tans = ST.random_tangents(4, K, seed=61)
    got, flags, _, _ = _call(handles[model], b, tans, 4, K)
    assert np.array_equal(flags[:4], expect), flags
    rows = got[:K * 4].reshape(K, 4, 4, 3)
    for i in range(4):
        bad = np.isnan(rows[:, i]).all(axis=(0, 2))
        assert bad.tolist() == [leg == i for leg in range(4)] and np.isfinite(rows[:, i][:, ~bad]).all(), i
    none, only, after, before = _call(handles[model], b, tans, 4, K, want=("flags",))
    assert none is None and np.array_equal(only, flags) and all(np.array_equal(after[k], before[k], equal_nan=True) for k in after)


# ------------------------------------------------------------------ 7. the rollout through a trot
def _pair(bars, R, tan, held=None):
    """(sum, sum of magnitudes) per robot of <bars, tangents> at one interface of the rollout (tests/test_gpu_leg_plant_tangent.py's),
    with the held swing_pos pairing added where `held` = (swing_pos_bar, swing_pos_tan) is given"""
    n = R.shape[0]
    dR = (LT.PT.hat(tan["Rwb_rot_tan"].reshape(n, 3)) @ R.reshape(n, 3, 3)).reshape(n, 9)
    total, mag = np.zeros(n), np.zeros(n)
    for bar, t in ((bars["Rwb"], dR),) + tuple((bars[k], tan[k + "_tan"]) for k in STATE[1:]) + ((held,) if held else ()):
        prod = bar.reshape(n, -1) * t.reshape(n, -1)
        total += prod.sum(axis=1)
        mag += np.abs(prod).sum(axis=1)
    return total, mag


def test_rollout_swing_tangent_through_a_trot(q):
    """rollout_swing_tangent over SW.ROLLOUT_STEPS = 3 steps from SW.trot_start() (SW.rollout_case: the loss <c, final six state arrays>,
    the committed directions in joint_q, x and the held swing_pos), race = 0.
    The state ends bit for bit where ctl.rollout_tick leaves it; the flags are 0.
    Central differences of ctl.rollout_tick with the rule and the cap of item 5 over every step (statuses, plant flags, working-set
    words and clamp masks equal at all five points; kept >= 0.5 - the CPU loop alone keeps 0.985, SW.cpu_rollout_kept) and the bar
    |FD(h) - FD(2h)| + 1e-5 |gradient| |direction|.
    <bar, tangent> against rollout_tick_autograd over the same steps, the bar accumulated interface by interface as
    tests/test_gpu_leg_plant_tangent.py accumulates its own: 4 C_DOT C_LDOT max(C_TDOT, C_SDOT) EPS sum_s cond_s (mag_s + mag_{s+1}),
    the held swing_pos's pairing - its cotangent from the remaining steps - counted at every interface."""
    import torch

    from quadruped_control_amd import tangent as T

    P = params(q, "uniform")
    ctl = _trot_ctl(q)
    n, H, h = SW.ROLLOUT_N, SW.ROLLOUT_STEPS, SW.ROLLOUT_H
    b, c, v = SW.rollout_case()
    lo, hi = LA.tau_limits()
    cd = {k: torch.from_numpy(a).cuda() for k, a in c.items()}
    seeds = {k + "_tan": torch.from_numpy(np.ascontiguousarray(a)).cuda() for k, a in v.items()}

    def rollout(k):
        start = dict(b, **{name: np.ascontiguousarray(b[name] + k * h * v[name]) for name in v})
        words, status, clamp, flags = [], [], [], []
        for steps in range(1, H + 1):
            state, out = ctl.rollout_tick(q.to_device(start), None, steps, DT, LA.STAND_INERTIA)
            words.append(out["active_set"].cpu().numpy())
            status.append(out["status"].cpu().numpy())
            tau = out["joint_tau"].cpu().numpy()
            clamp.append((tau <= lo) | (tau >= hi))
            flags.append(out["flags"].cpu().numpy())
        final = {name: state[name].cpu().numpy() for name in STATE}
        return sum((final[name] * c[name]).sum(axis=1) for name in STATE), np.array(words), np.array(status), np.array(clamp), np.array(flags), final

    L0, w0, st0, cl0, fl0, final0 = rollout(0)
    _, rec = ctl.rollout_tick(q.to_device(b), None, H, DT, LA.STAND_INERTIA, record_every=1)
    states = [{k: hist[k] for k in STATE} for _, hist in rec["history"]]
    tan, flags = [], None
    for s in range(H + 1):
        dev = q.to_device(b)
        state, res = T.rollout_swing_tangent(ctl, dev, s, DT, LA.STAND_INERTIA, seeds)
        tan.append({k: res[k].cpu().numpy() for k in T._TICK_STATE})
        flags = res["flags"].cpu().numpy()
        if s == H:
            states.append({k: dev[k].clone() for k in STATE})
            for name in STATE:
                assert np.array_equal(state[name].cpu().numpy(), final0[name]), name  # ctl.rollout_tick's bits
    assert not flags.any(), flags
    bars, held, cond = [], [], []
    for s in range(H):
        leaf = dict(q.to_device(b), **{k: t.clone().requires_grad_(True) for k, t in states[s].items()})
        leaf["swing_pos"].requires_grad_(True)
        final, _ = ctl.rollout_tick_autograd(leaf, H - s, DT, LA.STAND_INERTIA)
        sum((final[k] * cd[k]).sum() for k in STATE).backward()
        bars.append({k: leaf[k].grad.cpu().numpy() for k in STATE})
        held.append((leaf["swing_pos"].grad.cpu().numpy(), v["swing_pos"]))
        now = dict(q.to_device(b), **states[s])
        grf = ctl.control_batch(now, want_torques=True)["grf_body"].cpu().numpy()
        host = {k: t for k, t in dict(b, **{k: t.cpu().numpy() for k, t in states[s].items()}).items() if k not in ("joint_qdot", "swing_pos", "swing_vel")}
        cond.append(QR.tangent(P, host, grf, {"x_tan": np.zeros((1, n, 3))})["cond"])
    bars.append(c)
    held.append(None)
    torch.cuda.synchronize()
    sides = [_pair(bars[s], states[s]["Rwb"].cpu().numpy(), tan[s], held[s]) for s in range(H + 1)]
    lhs, rhs = sides[H][0], sides[0][0]
    bar = 4 * QR.C_DOT * LT.C_LDOT * max(LT.C_TDOT, ST.C_SDOT["default"]) * EPS * sum(cond[s] * (sides[s][1] + sides[s + 1][1]) for s in range(H))
    assert np.isfinite(lhs).all() and np.isfinite(rhs).all() and (np.abs(lhs) > 0).all()
    ratio = np.abs(lhs - rhs) / bar
    print("dot product against reverse mode: worst gap / bar", float(ratio.max()), "worst gap / (EPS magnitudes)",
          float((np.abs(lhs - rhs) / (EPS * (sides[0][1] + sides[H][1]))).max()))
    assert (ratio <= 1.0).all(), float(ratio.max())
    # central differences of ctl.rollout_tick
    g = {k: (bars[0][k] if k in bars[0] else held[0][0]) for k in v}
    pts = {k: rollout(k) for k in (-2, -1, 1, 2)}
    keep = (st0 == 0).all(axis=0) & (fl0 == 0).all(axis=0)
    for Lk, wk, stk, clk, flk, _ in pts.values():
        keep &= (stk == 0).all(axis=0) & (wk == w0).all(axis=0) & (clk == cl0).all(axis=(0, 2)) & (flk == 0).all(axis=0)
    fd1, fd2 = (pts[1][0] - pts[-1][0]) / (2 * h), (pts[2][0] - pts[-2][0]) / (4 * h)
    scale = np.sqrt(sum((g[k] ** 2).sum(axis=1) for k in v)) * np.sqrt(sum((v[k] ** 2).sum(axis=1) for k in v))
    err, t = np.abs(fd1 - lhs), np.abs(fd1 - fd2)
    print("central differences: kept", keep.mean(), "worst relative error", float((err[keep] / scale[keep]).max()), "worst t", float((t[keep] / scale[keep]).max()))
    assert keep.mean() >= 0.5, keep.mean()
    assert np.all(err[keep] <= t[keep] + 1e-5 * scale[keep])
    ctl.close()


def test_rollout_swing_tangent_memory_does_not_grow_with_steps(q, handles):
    """torch.cuda.max_memory_allocated over rollout_swing_tangent (K = 12 seeded directions) at steps = 1 and 4: the peaks are EQUAL."""
    import torch

    from quadruped_control_amd import tangent as T

    n, K = 256, 12
    b = SW.trot_start(n)
    rng = np.random.default_rng(0x5719A)
    tans = {k: torch.from_numpy(rng.normal(0.0, 0.01, (K, n, m))).cuda() for k, m in T.ROLLOUT_SWING_TANGENTS.items()}

    def peak(H):
        dev = q.to_device(b)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        keep = T.rollout_swing_tangent(handles["default"], dev, H, DT, LA.STAND_INERTIA, tans)
        torch.cuda.synchronize()
        top = torch.cuda.max_memory_allocated() - base
        del keep
        return top

    peak(1)  # (what a first call sets up once is not tangent memory)
    p1, p4 = peak(1), peak(4)
    print(f"peak bytes, n = {n}, K = {K}: steps = 1: {p1}, steps = 4: {p4}")
    assert p1 == p4, (p1, p4)


# ------------------------------------------------------------------ 8. the transition matrix
def test_rollout_swing_transition(q, handles):
    """steps = 0 gives the identity; a column equals the single-seed rollout bit for bit at chunk None and 5; with an all-stance mask and
    zero references given it equals rollout_tick_transition bit for bit."""
    import torch

    from quadruped_control_amd import tangent as T

    ctl, n, H = handles["default"], 17, 2
    b = SW.trot_start(n)
    ident = T.rollout_swing_transition(ctl, q.to_device(b), 0, DT, LA.STAND_INERTIA)
    assert torch.equal(ident["phi"], torch.eye(36, dtype=torch.float64, device="cuda").expand(n, 36, 36)) and not bool(ident["flags"].any())
    full = T.rollout_swing_transition(ctl, q.to_device(b), H, DT, LA.STAND_INERTIA)
    chunked = T.rollout_swing_transition(ctl, q.to_device(b), H, DT, LA.STAND_INERTIA, chunk=5)
    assert full["columns"] == list(T.TICK_TRANSITION_COLUMNS) and torch.equal(full["flags"], chunked["flags"]) and not bool(full["flags"].any())
    assert_same_bits(chunked["phi"], full["phi"], "phi at chunk = 5")
    assert bool(torch.isfinite(full["phi"]).all())
    for col in (1, 4, 13, 30):
        name, comp = T.TICK_TRANSITION_COLUMNS[col]
        seed = torch.zeros((n, T.ROLLOUT_TICK_TANGENTS[name + "_tan"]), dtype=torch.float64, device="cuda")
        seed[:, comp] = 1.0
        _, res = T.rollout_swing_tangent(ctl, q.to_device(b), H, DT, LA.STAND_INERTIA, {name + "_tan": seed})
        rows = torch.cat([res[k].reshape(n, -1) for k in T._TICK_STATE], dim=-1)
        assert_same_bits(full["phi"][:, :, col].contiguous(), rows, f"column {col}")
    swing_legs = torch.from_numpy(np.repeat(b["stance"] == 0, 3, axis=1)).cuda()
    qdot_cols = full["phi"][:, :, 24:]  # a swing leg's joint_qdot is read by the tick's PD law and by the plant: those columns are not 0
    assert bool((qdot_cols.abs().sum(dim=1) > 0)[swing_legs].all())
    stand = dict(b, stance=np.ones((n, 4), np.uint8), swing_pos=np.zeros((n, 12)), swing_vel=np.zeros((n, 12)))
    with_refs = T.rollout_swing_transition(ctl, q.to_device(stand), H, DT, LA.STAND_INERTIA)
    plain = T.rollout_tick_transition(ctl, q.to_device({k: a for k, a in stand.items() if k not in ("swing_pos", "swing_vel")}), H, DT, LA.STAND_INERTIA)
    assert_same_bits(with_refs["phi"], plain["phi"], "phi, all stance")
    assert torch.equal(with_refs["flags"], plain["flags"])


# ------------------------------------------------------------------ 9. refusals
def test_refusals_launch_nothing(q, handles, references):
    """Every refusal of qc_swing_torque_tangent_batch returns -1 with its prefix and leaves the guarded outputs as they were; n == 0
    launches nothing; the same structs, valid, do launch.  The Python entry points raise ValueError with the library's message, and
    the two rollouts refuse what has no forward mode before anything is launched."""
    import torch

    from quadruped_control_amd import _lib
    from quadruped_control_amd import tangent as T

    c, ctl, n, K = references["default"], handles["default"], 17, 2
    lib = T._library()
    b, stance, tans, _, _ = _tiled_case(c, n, K)
    b["stance"] = np.zeros((n, 4), np.uint8)
    dev = q.to_device(b)
    td = {k: torch.from_numpy(a).cuda() for k, a in tans.items()}
    out = torch.full((K, n, 4, 3), SENTINEL, dtype=torch.float64, device="cuda")
    flags = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    guards = [(out, SENTINEL, True), (flags, 77, True)]

    def io():
        s = T.QcSwingTangentIo()
        lib.qc_default_swing_tangent(ctypes.byref(s))
        s.n_dir = K
        for k, t in td.items():
            setattr(s, k, t.data_ptr())
        s.joint_tau_tan, s.flags = out.data_ptr(), flags.data_ptr()
        return s

    keys = SWING_KEYS + ("stance",)

    def refused(what, bi, s, text):
        rc = lib.qc_swing_torque_tangent_batch(ctl._h, n, ctypes.byref(bi), ctypes.byref(s), None)
        assert rc == -1 and _lib.last_error().startswith("qc_swing_torque_tangent_batch:") and text in _lib.last_error(), (what, rc, _lib.last_error())
        torch.cuda.synchronize()
        assert all(bool((t == sentinel).all()) for t, sentinel, _ in guards), what

    for missing in SWING_KEYS:
        refused("no " + missing, batch_in(dev, [k for k in keys if k != missing]), io(), "are required")
    extra = batch_in(dev, keys)
    extra.swing_state = dev["x"].data_ptr()
    refused("swing_state", extra, io(), "swing_state must be NULL")
    extra = batch_in(dev, keys)
    extra.gait_dt = dev["x"].data_ptr()
    refused("gait_dt", extra, io(), "gait_dt must be NULL")
    s = io()
    s.n_dir = 0
    refused("n_dir", batch_in(dev, keys), s, "n_dir must be >= 1")
    s = io()
    s.joint_tau_tan = s.flags = None
    refused("no output", batch_in(dev, keys), s, "no output requested")
    s = io()
    for k in td:
        setattr(s, k, None)
    refused("no tangent", batch_in(dev, keys), s, "no tangent given")
    s = io()
    s.n_dir = 0xFFFFFF * 64 // (4 * n) + 1
    refused("beyond one launch", batch_in(dev, keys), s, "4 * n * n_dir is beyond one launch")
    assert_raw_refusals(lib.qc_swing_torque_tangent_batch, lambda: (ctl._h, n, batch_in(dev, keys), io()), "qc_swing_tangent_io",
                        ctypes.sizeof(T.QcSwingTangentIo), ctypes.sizeof(T.QcTorqueTangentIo), guards, beyond=0xFFFFFF * 64 // 4 + 1)
    # the Python entry points: the library's words, and nothing written
    out.fill_(SENTINEL)
    with pytest.raises(ValueError, match="^qc_swing_torque_tangent_batch: gait_dt must be NULL"):
        T.swing_torque_tangent(ctl, dict(dev, gait_dt=dev["x"][:, 0].contiguous()), td, out={"joint_tau_tan": out})
    with pytest.raises(ValueError, match="^qc_swing_torque_tangent_batch: no tangent given"):
        T.swing_torque_tangent(ctl, dev, {}, out={"joint_tau_tan": out[0]})  # (no tangent: one direction)
    with pytest.raises(ValueError, match="^qc_swing_torque_tangent_batch: Rwb, x, joint_q, joint_qdot, swing_pos and swing_vel are required"):
        T.swing_torque_tangent(ctl, {k: t for k, t in dev.items() if k != "swing_vel"}, td, out={"joint_tau_tan": out})
    with pytest.raises(ValueError, match="swing_torque_tangent: unknown tangent"):
        T.swing_torque_tangent(ctl, dev, {"grf_tan": td["joint_q_tan"]})
    with pytest.raises(ValueError, match="unknown output"):
        T.swing_torque_tangent(ctl, dev, td, want=("grf_tan",))
    full = _full(b)
    before = {k: t.clone() for k, t in q.to_device(full).items()}
    seeds = {"x_tan": td["x_tan"]}
    for fn, extra_args in ((T.rollout_swing_tangent, (seeds,)), (T.rollout_swing_transition, ())):
        who = fn.__name__
        for bad, text in ((dict(before, swing_state=before["x"]), "swing_state"), (dict(before, gait_dt=before["x"]), "gait_dt"),
                          ({k: t for k, t in before.items() if k != "swing_pos"}, "swing_pos and swing_vel, both"),
                          ({k: t for k, t in before.items() if k != "swing_vel"}, "swing_pos and swing_vel, both")):
            with pytest.raises(ValueError, match=f"^{who}: .*{text}"):
                fn(ctl, bad, 2, DT, LA.STAND_INERTIA, *extra_args)
    for kw, text in ((dict(command={}), "commander mode has no forward mode"), (dict(lean={}), "lean has no forward mode")):
        with pytest.raises(ValueError, match=f"^rollout_swing_tangent: {text}"):
            T.rollout_swing_tangent(ctl, before, 2, DT, LA.STAND_INERTIA, seeds, **kw)
    with pytest.raises(ValueError, match="^rollout_swing_tangent: unknown tangent"):
        T.rollout_swing_tangent(ctl, before, 2, DT, LA.STAND_INERTIA, {"feet_tan": td["joint_q_tan"]})
    with pytest.raises(ValueError, match="^rollout_swing_tangent: no tangent given"):
        T.rollout_swing_tangent(ctl, before, 2, DT, LA.STAND_INERTIA, {})
    with pytest.raises(ValueError, match="^rollout_swing_transition: chunk must be >= 1"):
        T.rollout_swing_transition(ctl, before, 2, DT, LA.STAND_INERTIA, chunk=0)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    fresh = q.to_device(full)
    assert all(torch.equal(before[k], fresh[k]) for k in fresh)  # nothing was stepped


def _full(b):
    """the swing pool's arrays with the rest of the state a solve reads: at rest, the desired state the robot's own"""
    n = b["x"].shape[0]
    eye = np.tile(np.eye(3).reshape(9), (n, 1))
    return dict(b, Rwb_d=eye, xdot=np.zeros((n, 3)), w=np.zeros((n, 3)), x_d=b["x"].copy(), xdot_d=np.zeros((n, 3)), w_d=np.zeros((n, 3)))
