"""GPU: rollout_commander_tangent() and rollout_lean_tangent() (quadruped_control_amd/tangent.py) at n = 65, K = 3, 3 steps of a trot
whose diagonal is replanned at the second tick for the even robots (tests/test_gpu_swing_reference_tangent.py's start), race = 0:
the state, the phases and the records against ctl.rollout_tick() bit for bit; <loss gradient, final tangents> against the reverse mode
of rollout_commander_autograd() / rollout_gait_autograd(lean=...) with seeds on twist_tan / schedule_tan; a command sequence; tangent
memory at 2 and 6 steps; six unit twist seeds against central differences of rollout_tick().

The bar of the dot products is the accumulated one of the sibling rollout tests: the identity holds step by step between the
interfaces s and s + 1,  bar = 4 C_DOT C_LDOT max(C_TDOT, C_SDOT, C_RDOT, C_CDOT | C_MDOT) EPS sum_s cond_s (mag_s + mag_{s+1}),  mag_s the
magnitudes of <bar_s, tan_s> at interface s - bar_s from the reverse mode of the remaining H - s steps run from the recorded state s with
everything carried as a leaf, tan_s from the forward-mode rollout over s steps -, cond_s the reduced condition number of solve s."""
import numpy as np
import pytest

from tests import com_reference_tangent_restatement as MT
from tests import commander_tangent_restatement as CT
from tests import leg_plant_adjoint_restatement as LA
from tests import leg_plant_tangent_restatement as LT
from tests import swing_reference_restatement as RR
from tests import swing_reference_tangent_restatement as RT
from tests import swing_tangent_restatement as ST
from tests import tangent_restatement as QR
from tests.gpu_arrays import assert_same_bits, q  # noqa: F401
from tests.solved_batch_support import EPS, params
from tests.test_gpu_swing_reference_tangent import _bytes, _cuda, _fresh, _handle, _rollout_start

pytestmark = pytest.mark.gpu
N, K, H, DT = 65, 3, 3, LA.DT
STATE = LA.INPUTS[:-1]
MOVED = STATE + ("gait_phase", "swing_state")
DESIRED = ("Rwb_d", "x_d", "xdot_d", "w_d")
TWIST = np.array([0.3, -0.1, 0.0, 0.0, 0.0, 0.2])


@pytest.fixture(scope="module")
def ctl(q):
    c = _handle(q, RR.DEFAULT_MODEL)
    yield c
    c.close()


def _records(q, n):
    """commander records of robots that stand and run, a command pending: (device uint8 tensor)"""
    from quadruped_control_amd.balance_controller import new_commander_states

    rec = new_commander_states(n)
    rec["standing"], rec["gait_running"] = 1, 1
    return _cuda(_bytes(rec))


def _start(q, n):
    """the trot's start without a desired state of its own: commander mode keeps it in the records"""
    return {k: v for k, v in _rollout_start(RR.DEFAULT_MODEL, n).items() if k not in DESIRED}


def _command(q, n, twist=None, seed=3):
    rng = np.random.default_rng(seed)
    tw = TWIST[None] + 0.05 * rng.normal(size=(n, 6)) if twist is None else twist
    return dict(state=_records(q, n), twist=_cuda(tw), fresh=_cuda(np.ones(n, np.uint8)))


def _pair(bars, tan, rotations):
    """(sum, magnitudes) per robot of <bars, tangents>: `rotations` name -> the [n,9] matrix whose entrywise bar pairs with [tan]x R"""
    n = next(iter(rotations.values())).shape[0]
    total, mag = np.zeros(n), np.zeros(n)
    for name, bar in bars.items():
        t = tan[name]
        if name in rotations:
            t = ST.skew_times(np.asarray(t).reshape(n, 3), rotations[name].reshape(n, 9))
        if np.asarray(bar).size == np.asarray(t).size and np.asarray(bar).shape[0] == n:
            prod = np.asarray(bar).reshape(n, -1) * np.asarray(t).reshape(n, -1)
            total += prod.sum(axis=1)
            mag += np.abs(prod).sum(axis=1)
        else:  # a parameter shared by the batch: one number, spread over the robots so that the per-robot sums still add up
            prod = np.asarray(bar).reshape(-1) * np.asarray(t).reshape(-1)
            total += prod.sum() / n
            mag += np.abs(prod).sum() / n
    return total, mag


def _cond(ctl, q, state, desired, n):
    """the reduced condition number of the solve of a step: on its state, its desired state and the mask its tick used"""
    P = params(q, "uniform")
    mask = (state["swing_state_after"].cpu().numpy().reshape(-1).view(RR.STATE_DTYPE)["leg_state"] == 1).astype(np.uint8)
    dev = dict({k: state[k] for k in ("Rwb", "x", "xdot", "w", "joint_q")}, **desired, stance=_cuda(mask))
    grf = ctl.control_batch(dev)["grf_body"].cpu().numpy()
    host = {k: t.cpu().numpy() for k, t in dev.items()}
    return QR.tangent(P, host, grf, {"x_tan": np.zeros((1, n, 3))})["cond"]


def _grad(t):
    import torch

    return (torch.zeros_like(t) if t.grad is None else t.grad).cpu().numpy()


def _commander_pairing(q, ctl, lean, rng):
    """K = 3 directions of rollout_commander_tangent() (seeds on twist_tan and, with `lean` = (schedule, mode, gain), on a shared
    schedule_tan) over 0 ... H steps, and the reverse mode of the remaining steps from every interface with everything carried as a leaf
    (the commander step, the lean and the gait step as rollout_commander_autograd() chains them).  Returns (states, plain-rollout
    inputs, per direction: (lhs, rhs, bar, magnitudes at both ends) per robot, the bars of interface 0)."""
    import torch

    from quadruped_control_amd import autograd as AG
    from quadruped_control_amd import tangent as T

    n = N
    b = _start(q, n)
    c = {k: _cuda(rng.normal(0.0, 1.0, b[k].shape)) for k in STATE}
    seed = rng.normal(0.0, 1.0, (K, n, 6))
    sched_seed = rng.normal(0.0, 0.05, (K, 4, 4))
    cmd0 = _command(q, n)
    seeds = {"twist_tan": _cuda(seed)}
    kw = {}
    if lean is not None:
        seeds["schedule_tan"] = _cuda(sched_seed)
        kw["lean"] = dict(schedule=lean[0], mode=lean[1], gain=lean[2])
    tan, states = [], []
    for s in range(H + 1):
        dev, cmd = _fresh(q, b, n), dict(cmd0, state=cmd0["state"].clone())
        _, res = T.rollout_commander_tangent(ctl, dev, cmd, s, DT, LA.STAND_INERTIA, DT, seeds, **kw)
        torch.cuda.synchronize()
        assert not res["flags"].cpu().numpy().any(), (s, res["flags"])
        assert tuple(res["x_tan"].shape) == (K, n, 3)
        t = {k[:-4]: res[k].cpu().numpy() for k in T._TICK_STATE + T._GAIT_RECORD + ("x_d_tan", "xdot_d_tan", "w_d_tan")}
        t.update(Rwb=res["Rwb_rot_tan"].cpu().numpy(), Rwb_d=res["Rwb_d_rot_tan"].cpu().numpy(), Vb=res["Vb_tan"].cpu().numpy(), twist=seed, schedule=sched_seed)
        tan.append(t)
        states.append(dict({k: v.clone() for k, v in dev.items()}, cmd_state=cmd["state"].clone()))
    # reverse mode from every interface: the remaining steps with everything carried as a leaf
    scalars, clock = {}, torch.full((n,), DT, dtype=torch.float64, device="cuda")
    bars, cond = [], []
    for s in range(H):
        st = states[s]
        leaf = {k: st[k].clone().requires_grad_(True) for k in STATE}
        col = {k: t.clone().requires_grad_(True) for k, t in AG._commander_columns(st["cmd_state"]).items()}
        ps, pf = (t.clone().requires_grad_(True) for t in AG._record_points(st["swing_state"]))
        twist = cmd0["twist"].clone().requires_grad_(True)
        sch = None if lean is None else lean[0].clone().requires_grad_(True)
        run = dict({k: t for k, t in st.items() if k not in ("swing_state", "gait_phase", "cmd_state")}, **leaf)
        record, phase, cstate, Vb, desired = st["swing_state"], st["gait_phase"], st["cmd_state"], col["Vb"], tuple(col[k] for k in DESIRED)
        p0, p1, active, flags = ps, pf, None, torch.zeros((n,), dtype=torch.int32, device="cuda")
        tracked_first = None
        for j in range(s, H):
            cmd = dict(scalars, state=cstate, twist=twist, fresh=cmd0["fresh"]) if j == 0 else dict(scalars, state=cstate)
            *desired, Vb, cstate, _run, _applied = AG.commander_step_autograd(ctl, run, cmd, tuple(desired), Vb)
            tracked = dict(zip(DESIRED, desired))
            if lean is not None:  # the tick alone tracks the leaned value
                tracked["x_d"] = AG._lean_x_d(ctl, (sch, lean[1], lean[2]), run, phase, None, desired[1])
            if tracked_first is None:
                tracked_first = {k: t.detach().contiguous() for k, t in tracked.items()}
            run, out, (phase, record, p0, p1, _, active) = AG._gait_step(ctl, run, tracked, phase, None, clock, record, p0, p1, True, active, flags, DT,
                                                                         LA.STAND_INERTIA, 1e-7, None, None)
        sum((run[k] * c[k]).sum() for k in STATE).backward()
        bars.append(dict({k: _grad(leaf[k]) for k in STATE}, **{k: _grad(col[k]) for k in col}, p_start=_grad(ps), p_final=_grad(pf),
                         **({"twist": _grad(twist)} if s == 0 else {}), **({} if lean is None else {"schedule": _grad(sch)})))
        cond.append(_cond(ctl, q, dict(st, swing_state_after=states[s + 1]["swing_state"]), tracked_first, n))
    bars.append({k: c[k].cpu().numpy() for k in STATE})
    rot = lambda s: {"Rwb": states[s]["Rwb"].cpu().numpy(), "Rwb_d": AG._commander_columns(states[s]["cmd_state"])["Rwb_d"].cpu().numpy()}
    unit = 4 * QR.C_DOT * LT.C_LDOT * max(LT.C_TDOT, ST.C_SDOT["default"], RT.C_RDOT, CT.C_CDOT, MT.C_MDOT if lean is not None else 0.0) * EPS
    per_direction = []
    for k in range(K):
        sides = [_pair(bars[s], {name: t[k] for name, t in tan[s].items()}, rot(s)) for s in range(H + 1)]
        bar = unit * sum(cond[s] * (sides[s][1] + sides[s + 1][1]) for s in range(H))
        per_direction.append((sides[H][0], sides[0][0], bar, sides[0][1] + sides[H][1]))
    return states, (b, cmd0), per_direction, bars[0], tan


def test_rollout_commander_tangent_against_rollout_tick_and_reverse_mode(q, ctl):
    """K = 3 seeds on twist_tan: the final state against ctl.rollout_tick(batch, command, ...) bit for bit, and per direction and robot
    <c, final tangents> against <the reverse mode's twist gradient, the seed> within the accumulated bar."""
    states, (b, cmd0), per_direction, bars0, tan = _commander_pairing(q, ctl, None, np.random.default_rng(0xC0DE))
    plain, pc = _fresh(q, b, N), dict(cmd0, state=cmd0["state"].clone())
    ctl.rollout_tick(plain, pc, H, DT, LA.STAND_INERTIA)
    for k in MOVED:
        assert_same_bits(states[H][k], plain[k], k)  # ctl.rollout_tick(batch, command, ...)'s bits
    assert_same_bits(states[H]["cmd_state"], pc["state"], "the commander records")
    assert np.abs(tan[H]["p_final"][:, 0::2]).sum() > 0 and np.abs(tan[H]["x_d"]).sum() > 0 and not np.abs(tan[H]["x_d"][..., 2]).any()
    assert np.abs(bars0["twist"]).sum() > 0
    for k, (lhs, rhs, bar, mags) in enumerate(per_direction):
        assert np.isfinite(lhs).all() and np.isfinite(rhs).all() and (np.abs(lhs) > 0).all()
        ratio = np.abs(lhs - rhs) / bar
        print(f"commander rollout against reverse mode, direction {k}: worst gap / bar", float(ratio.max()), "worst gap / (EPS magnitudes)",
              float((np.abs(lhs - rhs) / (EPS * mags)).max()))
        assert (ratio <= 1.0).all(), (k, float(ratio.max()))


def test_a_leaned_commander_rollout_against_reverse_mode(q, ctl):
    """The leaned commander path - offset mode at gain 0.7, x_d_in_tan the commander's x_d_tan, K = 3 seeds on twist_tan AND on a
    shared schedule_tan - against the reverse mode of the same chain (commander_step_autograd, com_reference_autograd for the tick
    alone, the gait step): the schedule is shared, so the identity is one number per direction over the batch; the bar is the
    accumulated one, with C_MDOT among the stage constants."""
    sched = _cuda(np.full((4, 4), 0.2) + 0.02 * np.random.default_rng(7).normal(size=(4, 4)))
    _, _, per_direction, bars0, _ = _commander_pairing(q, ctl, (sched, "offset", 0.7), np.random.default_rng(0x1EA7))
    assert np.abs(bars0["twist"]).sum() > 0 and np.abs(bars0["schedule"]).sum() > 0
    for k, (lhs, rhs, bar, mags) in enumerate(per_direction):
        gap = abs(lhs.sum() - rhs.sum())
        assert np.isfinite(gap) and abs(lhs.sum()) > 0
        print(f"leaned commander rollout against reverse mode, direction {k}: gap / bar", float(gap / bar.sum()), "gap / (EPS magnitudes)", float(gap / (EPS * mags.sum())))
        assert gap <= bar.sum(), (k, gap, bar.sum())


def test_a_command_sequence(q, ctl):
    """twist [steps,n,6] (cold solves throughout: the one-step calls it is compared with have no previous working set): the state and the records equal H one-step rollout_tick() calls, each with its own fresh command, bit for bit;
    a twist_tan on step 1 alone leaves step 0's tangents zero and equals the single-command rollout started from the state after step 0"""
    import torch

    from quadruped_control_amd import tangent as T

    n = N
    b = _start(q, n)
    rng = np.random.default_rng(0x5E9)
    seq = TWIST[None, None] + 0.05 * rng.normal(size=(H, n, 6))
    seed = np.zeros((K, H, n, 6))
    seed[:, 1] = rng.normal(0.0, 1.0, (K, n, 6))
    records = _records(q, n)
    plain, rec = _fresh(q, b, n), records.clone()
    for k in range(H):
        ctl.rollout_tick(plain, dict(state=rec, twist=_cuda(seq[k]), fresh=_cuda(np.ones(n, np.uint8))), 1, DT, LA.STAND_INERTIA, warm=False)
    dev, cmd = _fresh(q, b, n), dict(state=records.clone(), twist=_cuda(seq))
    _, res = T.rollout_commander_tangent(ctl, dev, cmd, H, DT, LA.STAND_INERTIA, DT, {"twist_tan": _cuda(seed)}, warm=False)
    torch.cuda.synchronize()
    for k in MOVED:
        assert_same_bits(dev[k], plain[k], k)
    assert_same_bits(cmd["state"], rec, "the commander records")
    assert tuple(res["x_tan"].shape) == (K, n, 3) and not bool(res["flags"].any()) and bool(res["x_tan"].abs().sum() > 0)
    # the same from the state after step 0, as a single fresh command with that seed
    dev1, cmd1 = _fresh(q, b, n), dict(state=records.clone(), twist=_cuda(seq[0]), fresh=_cuda(np.ones(n, np.uint8)))
    ctl.rollout_tick(dev1, cmd1, 1, DT, LA.STAND_INERTIA, warm=False)
    dev1 = {k: v for k, v in dev1.items() if k != "gait_dt"}
    _, res1 = T.rollout_commander_tangent(ctl, dev1, dict(state=cmd1["state"], twist=_cuda(seq[1]), fresh=_cuda(np.ones(n, np.uint8))), 1, DT,
                                          LA.STAND_INERTIA, DT, {"twist_tan": _cuda(seed[:, 1])}, warm=False)
    dev2, cmd2 = _fresh(q, b, n), dict(state=records.clone(), twist=_cuda(seq[:2]))
    _, res2 = T.rollout_commander_tangent(ctl, dev2, cmd2, 2, DT, LA.STAND_INERTIA, DT, {"twist_tan": _cuda(seed[:, :2])}, warm=False)
    for k in T._TICK_STATE + ("x_d_tan", "Vb_tan"):
        assert_same_bits(res2[k], res1[k], k)


def test_tangent_memory_does_not_grow_with_the_horizon(q, ctl):
    import torch

    from quadruped_control_amd import tangent as T

    n = 64
    b = _start(q, n)
    cmd0 = _command(q, n)
    tans = {"twist_tan": _cuda(np.eye(6)[:, None, :].repeat(n, axis=1))}

    def peak(steps):
        dev, cmd = _fresh(q, b, n), dict(cmd0, state=cmd0["state"].clone())
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        keep = T.rollout_commander_tangent(ctl, dev, cmd, steps, DT, LA.STAND_INERTIA, DT, tans)
        torch.cuda.synchronize()
        top = torch.cuda.max_memory_allocated() - base
        del keep
        return top

    peak(2)  # (what a first call sets up once is not tangent memory)
    p2, p6 = peak(2), peak(6)
    print(f"peak bytes, n = {n}, K = 6: steps = 2: {p2}, steps = 6: {p6}")
    assert p2 == p6, (p2, p6)


def test_six_unit_twist_seeds_against_central_differences(q, ctl):
    """The Jacobian of the loss <c, final state> in the command from six unit seeds against central differences of
    ctl.rollout_tick(batch, command, ...) along each twist component, under the sibling rollout tests' rule: kept where the statuses and
    the plant's flags are 0 and the records' integer words agree at all five points, kept >= 0.5, |FD(h) - analytic| <= |FD(h) - FD(2h)| +
    1e-5 |gradient| |v| (here |v| = 1)."""
    import torch

    from quadruped_control_amd import tangent as T

    n, h = N, 1e-4
    b = _start(q, n)
    rng = np.random.default_rng(0xFD)
    c = {k: rng.normal(0.0, 1.0, b[k].shape) for k in STATE}
    cmd0 = _command(q, n)
    tw0 = cmd0["twist"].cpu().numpy()
    dev, cmd = _fresh(q, b, n), dict(cmd0, state=cmd0["state"].clone())
    _, res = T.rollout_commander_tangent(ctl, dev, cmd, H, DT, LA.STAND_INERTIA, DT, {"twist_tan": _cuda(np.eye(6)[:, None, :].repeat(n, axis=1))})
    torch.cuda.synchronize()
    R = dev["Rwb"].cpu().numpy()
    jac = sum((c[k].reshape(1, n, -1) * res[k + "_tan"].cpu().numpy().reshape(6, n, -1)).sum(axis=2) for k in STATE[1:])
    jac += (c["Rwb"].reshape(1, n, 9) * ST.skew_times(res["Rwb_rot_tan"].cpu().numpy(), np.broadcast_to(R.reshape(1, n, 9), (6, n, 9)))).sum(axis=2)
    assert not res["flags"].cpu().numpy().any()

    def rollout(tw):
        d, cm = _fresh(q, b, n), dict(cmd0, state=cmd0["state"].clone(), twist=_cuda(tw))
        state, out = ctl.rollout_tick(d, cm, H, DT, LA.STAND_INERTIA)
        torch.cuda.synchronize()
        L = sum((c[k].reshape(n, -1) * state[k].cpu().numpy().reshape(n, -1)).sum(axis=1) for k in STATE)
        words = d["swing_state"].cpu().numpy().reshape(-1).view(RR.STATE_DTYPE)
        return L, out["status"].cpu().numpy(), out["flags"].cpu().numpy(), np.c_[words["leg_state"], words["has_traj"]]

    _, st0, fl0, w0 = rollout(tw0)
    kept = []
    for j in range(6):
        e = np.zeros(6)
        e[j] = 1.0
        pts = {m: rollout(tw0 + m * h * e) for m in (-2, -1, 1, 2)}
        keep = (st0 == 0) & (fl0 == 0)
        for _, stk, flk, wk in pts.values():
            keep &= (stk == 0) & (flk == 0) & (wk == w0).all(axis=1)
        fd1, fd2 = (pts[1][0] - pts[-1][0]) / (2 * h), (pts[2][0] - pts[-2][0]) / (4 * h)
        scale = np.sqrt((jac ** 2).sum(axis=0))
        err, t = np.abs(fd1 - jac[j]), np.abs(fd1 - fd2)
        kept.append(keep.mean())
        print(f"twist component {j}: kept {keep.mean():.2f}, worst relative error {float((err[keep] / scale[keep]).max()):.2e}")
        assert keep.mean() >= 0.5 and np.all(err[keep] <= t[keep] + 1e-5 * scale[keep]), j


def test_rollout_lean_tangent_against_rollout_tick_and_reverse_mode(q, ctl):
    import torch

    from quadruped_control_amd import autograd as AG
    from quadruped_control_amd import tangent as T

    n = N
    b = _rollout_start(RR.DEFAULT_MODEL, n)
    rng = np.random.default_rng(0x1EA2)
    c = {k: _cuda(rng.normal(0.0, 1.0, b[k].shape)) for k in STATE}
    sched = _cuda(np.full((4, 4), 0.2) + 0.02 * rng.normal(size=(4, 4)))
    seed = rng.normal(0.0, 0.05, (K, 4, 4))
    lean = dict(schedule=sched, mode="replace")
    plain = dict(_fresh(q, b, n), gait_dt=torch.zeros(n, dtype=torch.float64, device="cuda"))
    ctl.rollout_tick(plain, None, H, DT, LA.STAND_INERTIA, lean=lean)
    tan, states = [], []
    for s in range(H + 1):
        dev = _fresh(q, b, n)
        _, res = T.rollout_lean_tangent(ctl, dev, s, DT, LA.STAND_INERTIA, DT, lean, {"schedule_tan": _cuda(seed)})
        torch.cuda.synchronize()
        assert not res["flags"].cpu().numpy().any(), (s, res["flags"])
        t = {k[:-4]: res[k].cpu().numpy() for k in T._TICK_STATE + T._GAIT_RECORD}
        t.update(Rwb=res["Rwb_rot_tan"].cpu().numpy(), schedule=seed)
        tan.append(t)
        states.append({k: v.clone() for k, v in dev.items()})
    for k in MOVED + ("x_d",):
        assert_same_bits(states[H][k], plain[k], k)  # ctl.rollout_tick(batch, None, ..., lean=lean)'s bits
    base = _cuda(b["x_d"])
    bars, cond = [], []
    clock = torch.full((n,), DT, dtype=torch.float64, device="cuda")
    for s in range(H):
        st = states[s]
        leaf = {k: st[k].clone().requires_grad_(True) for k in STATE}
        sch = sched.clone().requires_grad_(True)
        ps, pf = (t.clone().requires_grad_(True) for t in AG._record_points(st["swing_state"]))
        run = dict({k: t for k, t in st.items() if k not in ("swing_state", "gait_phase")}, **leaf)
        record, phase, p0, p1, active, flags = st["swing_state"], st["gait_phase"], ps, pf, None, torch.zeros((n,), dtype=torch.int32, device="cuda")
        for _ in range(s, H):
            x_d = AG._lean_x_d(ctl, (sch, "replace", 1.0), run, phase, None, base)
            run, out, (phase, record, p0, p1, _, active) = AG._gait_step(ctl, run, {"x_d": x_d}, phase, None, clock, record, p0, p1, True, active, flags, DT,
                                                                         LA.STAND_INERTIA, 1e-7, None, None)
        sum((run[k] * c[k]).sum() for k in STATE).backward()
        bars.append(dict({k: _grad(leaf[k]) for k in STATE}, p_start=_grad(ps), p_final=_grad(pf), schedule=_grad(sch)))
        after = states[s + 1]
        want = dict({k: st[k] for k in ("Rwb_d", "xdot_d", "w_d")}, x_d=after["x_d"])
        cond.append(_cond(ctl, q, dict(st, swing_state_after=after["swing_state"]), want, n))
    bars.append({k: c[k].cpu().numpy() for k in STATE})
    assert tuple(res["x_tan"].shape) == (K, n, 3) and np.abs(bars[0]["schedule"]).sum() > 0
    for k in range(K):
        sides = [_pair(bars[s], {name: t[k] for name, t in tan[s].items()}, {"Rwb": states[s]["Rwb"].cpu().numpy()}) for s in range(H + 1)]
        lhs, rhs = sides[H][0].sum(), sides[0][0].sum()  # (the schedule is shared: one identity over the batch)
        bar = 4 * QR.C_DOT * LT.C_LDOT * max(LT.C_TDOT, ST.C_SDOT["default"], RT.C_RDOT, MT.C_MDOT) * EPS * \
            sum((cond[s] * (sides[s][1] + sides[s + 1][1])).sum() for s in range(H))
        assert np.isfinite(lhs) and np.isfinite(rhs) and abs(lhs) > 0
        print(f"lean rollout against reverse mode, direction {k}: gap / bar", float(abs(lhs - rhs) / bar), "gap / (EPS magnitudes)",
              float(abs(lhs - rhs) / (EPS * (sides[0][1] + sides[H][1]).sum())))
        assert abs(lhs - rhs) <= bar, k


def test_a_leaned_commander_rollout_has_the_autograd_twin_forward_values(q, ctl):
    import torch

    from quadruped_control_amd import tangent as T

    n = N
    b = _start(q, n)
    cmd0 = _command(q, n)
    lean = dict(schedule=_cuda(np.full((4, 4), 0.2)), gain=0.7)
    dev, cmd = _fresh(q, b, n), dict(cmd0, state=cmd0["state"].clone())
    seeds = {"twist_tan": _cuda(np.ones((n, 6))), "schedule_tan": _cuda(np.ones((4, 4)))}
    _, res = T.rollout_commander_tangent(ctl, dev, cmd, H, DT, LA.STAND_INERTIA, DT, seeds, lean=lean)
    ref, out = ctl.rollout_commander_autograd(_fresh(q, b, n), dict(cmd0, state=cmd0["state"].clone()), H, DT, LA.STAND_INERTIA, DT, lean=lean)
    torch.cuda.synchronize()
    for k in STATE:
        assert_same_bits(dev[k], ref[k].detach(), k)
    assert_same_bits(dev["gait_phase"], out["gait_phase"], "gait_phase")
    assert_same_bits(cmd["state"], out["cmd_state"], "the commander records")
    assert tuple(res["x_tan"].shape) == (n, 3) and not bool(res["flags"].any()) and bool(torch.isfinite(res["x_tan"]).all())
    assert bool((res["x_d_lean_tan"] != res["x_d_tan"]).any()) and T.COMMANDER_FLAGS_SHIFT == 24 and T.LEAN_FLAGS_SHIFT == 25
