"""-m gpu: commander mode (qc_tick_batch) - the stand-up latch, the gait start and the body-twist integration of the
reference's commander loop (commander_node.cpp:372-531) run inside the complete tick, checked tick by tick against
tests/commander_restatement.py for the commander and oracle.c_oracle for the rest of the tick."""
import ctypes as C

import numpy as np
import pytest

from tests.commander_support import (CASES, DESIRED, MEAS, _base, _check_instantiation, _compare_tick, _controller, _reference_tick,
                                     _state_host, _to_dev)
from tests.gpu_arrays import q  # noqa: F401

pytestmark = pytest.mark.gpu

# Batch sizes that do NOT fill their waves: a lone robot, a partial lane-group set, one robot beyond a whole number of waves
# (4 096 = 256 racing waves of 16, 16 384 = 512 two-lane waves, 32 768 = 512 one-lane waves) and one just above a multiple
# of 64 on the one-lane one-fill kernel.  Idle lane groups shadow the last robot there; the step must still run once per robot.
RAGGED = {
    "ragged-1": (1, {}, 4, None, 0),
    "ragged-3": (3, {}, 4, None, 0),
    "ragged-4097": (4097, {}, 4, None, 0),
    "ragged-16385": (16385, {}, 2, None, 0),
    "ragged-32769": (32769, {}, 1, 1, 0),
    "ragged-1-lane": (140033, {}, 1, 1, 0),
}
ALL_CASES = dict(CASES, **RAGGED)


def _heights(base_x2, tick, rng_params):
    """COM heights rising from the workload's value toward 0.26 + e (e within the band for most robots, 0.02 above it for
    some: those never stand), reaching it at robot-dependent ticks T (0 = from the start)."""
    T, e = rng_params
    goal = 0.26 + e
    frac = np.where(T == 0, 1.0, np.minimum(1.0, tick / np.maximum(T, 1)))
    return goal + (base_x2 - goal) * (1.0 - frac)


@pytest.mark.parametrize("case", list(CASES))
def test_closed_loop_commander_parity(q, case):
    import torch

    from oracle import c_oracle as O
    from tests import commander_restatement as CR

    n, tune, lanes, mode, ticks = CASES[case]
    P, ctl = _controller(q, tune)
    _check_instantiation(ctl, n, lanes, mode, case)
    rng = np.random.default_rng(0xC0DE + n)
    base = _base(n)
    meas = {k: base[k] for k in MEAS}
    T = rng.integers(0, max(2, ticks // 2), n)
    e = np.where(rng.uniform(size=n) < 0.15, 0.02, rng.uniform(-0.003, 0.003, n))
    dt = rng.uniform(0.002, 0.005, n)
    cmd = CR.Commander(n)
    ref_phase = base["gait_phase"].copy()
    ref_swing = O.new_swing_states(n)
    d_state = _to_dev(q.new_commander_states(n).view(np.uint8))
    d_phase = _to_dev(base["gait_phase"])
    d_swing = _to_dev(q.new_swing_states(n).view(np.uint8))
    d_dt = _to_dev(dt)
    d_meas = {k: _to_dev(v) for k, v in meas.items() if k != "x"}
    ran = applied_any = 0
    for tick in range(ticks):
        x = meas["x"].copy()
        x[:, 2] = _heights(base["x"][:, 2], tick, (T, e))
        twist = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.1, 0.1, n), np.zeros(n),
                          rng.uniform(-0.02, 0.02, n), rng.uniform(-0.02, 0.02, n), rng.uniform(-0.05, 0.05, n)], axis=1)
        fresh = (rng.uniform(size=n) < 0.3).astype(np.uint8)
        batch = dict(d_meas, x=_to_dev(x), gait_phase=d_phase, gait_dt=d_dt, swing_state=d_swing)
        out = ctl.tick_batch(batch, dict(state=d_state, twist=_to_dev(twist), fresh=_to_dev(fresh)))
        torch.cuda.synchronize()
        m = dict(meas, x=x)
        run, applied, r = _reference_tick(O, P, m, cmd, ref_phase, ref_swing, dt, twist, fresh)
        dev = dict(out={k: v.cpu().numpy() for k, v in out.items()}, state=_state_host(q, d_state), phase=d_phase.cpu().numpy(),
                   swing=d_swing.cpu().numpy().view(q.SWING_STATE_DTYPE))
        _compare_tick(q, O, P, ctl, tick, n, dev, dict(cmd=cmd, out=r, phase=ref_phase, swing=ref_swing), case)
        ran += int(run.sum())
        applied_any += int(applied.sum())
    # the run covered every branch: robots that never stood, robots that started the gait, and commands applied
    assert ran > 0 and applied_any > 0
    assert (cmd.standing == 0).any() and (cmd.gait_running == 1).any()
    if ticks >= 16:
        assert (ref_swing["has_traj"] == 1).any()


def _standing_states(q, base, n):
    s = q.new_commander_states(n)
    s["standing"] = 1
    s["gait_running"] = 1
    for k in DESIRED:
        s[k] = base[k]
    return s


@pytest.mark.parametrize("case", list(ALL_CASES))
def test_commander_step_changes_nothing_else(q, case):
    """A running robot with no pending command: qc_tick_batch must give what qc_control_batch gives when fed the state's desired
    values - bit for bit, over two ticks (the planner state carried) - and leave the commander state untouched."""
    import torch

    n, tune, lanes, mode, _ = ALL_CASES[case]
    _, ctl = _controller(q, tune)
    _check_instantiation(ctl, n, lanes, mode, case)
    base = _base(n)
    dt = _to_dev(np.full(n, 1.0 / 300.0))
    st0 = _standing_states(q, base, n)
    d_state = _to_dev(st0.view(np.uint8))
    d_meas = {k: _to_dev(base[k]) for k in MEAS}
    d_des = {k: _to_dev(base[k]) for k in DESIRED}
    ph_a, ph_b = _to_dev(base["gait_phase"]), _to_dev(base["gait_phase"])
    sw_a, sw_b = _to_dev(q.new_swing_states(n).view(np.uint8)), _to_dev(q.new_swing_states(n).view(np.uint8))
    zeros = _to_dev(np.zeros(n, np.uint8))
    junk = _to_dev(np.full((n, 6), 7.0))
    for tick in range(2):
        # (tick 1: a `fresh` array of zeros with a twist behind it changes nothing either)
        command = dict(state=d_state) if tick == 0 else dict(state=d_state, fresh=zeros, twist=junk)
        oa = ctl.tick_batch(dict(d_meas, gait_phase=ph_a, gait_dt=dt, swing_state=sw_a), command)
        ob = ctl.control_batch(dict(d_meas, **d_des, gait_phase=ph_b, gait_dt=dt, swing_state=sw_b), want_torques=True)
        torch.cuda.synchronize()
        for k in ("grf_body", "status", "joint_tau"):
            assert torch.equal(oa[k], ob[k]), (case, tick, k)
        assert torch.equal(ph_a, ph_b) and torch.equal(sw_a, sw_b), (case, tick)
        assert _state_host(q, d_state).tobytes() == st0.tobytes(), (case, tick)


@pytest.mark.parametrize("n,lanes,mode", [(600, 4, None), (20000, 2, None), (140000, 1, 1)] + [(c[0], c[2], c[3]) for c in RAGGED.values()])
def test_commander_step_runs_exactly_once(q, n, lanes, mode):
    """Cold-started config-3 robots leave stragglers that the lane-group tails (re-packed records) finish: after
    ONE launch every robot's commander, clock and planner have advanced exactly one step.  (The RAGGED sizes leave partial waves and
    idle lane groups; below 600 robots there are too few for a straggler statistic.)"""
    import torch

    from oracle import c_oracle as O
    from tests import commander_restatement as CR

    P, ctl = _controller(q, {})
    _check_instantiation(ctl, n, lanes, mode, "exactly-once")
    base = _base(n)
    rng = np.random.default_rng(5)
    x = base["x"].copy()
    x[:, 2] = 0.26 + rng.uniform(-0.004, 0.004, n)  # every robot inside the band
    kind = np.arange(n) % 4
    s = q.new_commander_states(n)
    s["standing"] = (kind >= 1).astype(np.int32)          # 0: stands up this tick
    s["gait_running"] = (kind >= 2).astype(np.int32)      # 1: starts the gait this tick
    s["cmd_pending"] = (kind == 3).astype(np.int32)       # 2: runs; 3: runs and applies its held command
    s["Vb"] = rng.uniform(-0.1, 0.1, (n, 6))
    cmd = CR.Commander(n)
    cmd.standing[:], cmd.gait_running[:], cmd.cmd_pending[:] = s["standing"], s["gait_running"], s["cmd_pending"]
    cmd.Vb[:] = s["Vb"]
    dt = np.full(n, 1.0 / 300.0)
    d_state = _to_dev(s.view(np.uint8))
    d_phase = _to_dev(base["gait_phase"])
    d_swing = _to_dev(q.new_swing_states(n).view(np.uint8))
    meas = dict({k: base[k] for k in MEAS}, x=x)
    out = ctl.tick_batch(dict({k: _to_dev(v) for k, v in meas.items()}, gait_phase=d_phase, gait_dt=_to_dev(dt), swing_state=d_swing),
                         dict(state=d_state), want_iterations=True)
    torch.cuda.synchronize()
    it = out["iterations"].cpu().numpy()
    if n >= 600:
        assert it.max() > np.median(it) + 3  # stragglers: the hand-over paths ran
    ref_phase, ref_swing = base["gait_phase"].copy(), O.new_swing_states(n)
    run, applied, r = _reference_tick(O, P, meas, cmd, ref_phase, ref_swing, dt, None, None)
    assert (run == (kind >= 2)).all() and (applied == (kind == 3)).all()
    if n % 4 == 0:
        assert run.sum() == applied.sum() * 2
    dev = dict(out={k: v.cpu().numpy() for k, v in out.items()}, state=_state_host(q, d_state), phase=d_phase.cpu().numpy(),
               swing=d_swing.cpu().numpy().view(q.SWING_STATE_DTYPE))
    _compare_tick(q, O, P, ctl, 0, n, dev, dict(cmd=cmd, out=r, phase=ref_phase, swing=ref_swing), f"once-{n}")


def test_tick_batch_argument_validation(q):
    """Every missing, extra or inconsistent pointer, a wrong struct_size and bad scalars: QC_ERR_INVALID with a message, nothing
    launched (the outputs keep their fill, the state and the clock do not move)."""
    import torch

    from quadruped_control_amd import _lib

    n = 8
    _, ctl = _controller(q, {})
    lib = _lib.load()
    base = _base(n)
    keep = {k: _to_dev(base[k]) for k in MEAS + DESIRED}
    st0 = q.new_commander_states(n)
    st0["standing"] = st0["gait_running"] = 1
    d_state = _to_dev(st0.view(np.uint8))
    d_phase = _to_dev(base["gait_phase"])
    d_swing = _to_dev(q.new_swing_states(n).view(np.uint8))
    d_dt = _to_dev(np.full(n, 0.01))
    d_tw = _to_dev(np.zeros((n, 6)))
    d_fr = _to_dev(np.ones(n, np.uint8))
    d_st = _to_dev(np.ones((n, 4), np.uint8))
    out = {"grf_body": _to_dev(np.full((n, 12), 5.0)), "status": _to_dev(np.full(n, -1, np.int32)), "joint_tau": _to_dev(np.full((n, 12), 5.0))}

    def valid():
        bi = _lib.QcBatchIn()
        for k in MEAS:
            setattr(bi, k, keep[k].data_ptr())
        bi.gait_phase, bi.gait_dt, bi.swing_state = d_phase.data_ptr(), d_dt.data_ptr(), d_swing.data_ptr()
        c = _lib.QcCommandIn()
        lib.qc_default_command(C.byref(c))
        c.state, c.twist, c.fresh = d_state.data_ptr(), d_tw.data_ptr(), d_fr.data_ptr()
        bo = _lib.QcBatchOut()
        for k, v in out.items():
            setattr(bo, k, v.data_ptr())
        return bi, c, bo

    cases = []
    for k in ("Rwb", "x", "xdot", "w", "joint_q", "joint_qdot", "gait_phase", "gait_dt", "swing_state"):
        cases.append((f"missing {k}", lambda bi, c, bo, k=k: setattr(bi, k, None)))
    for k in DESIRED:
        cases.append((f"extra {k}", lambda bi, c, bo, k=k: setattr(bi, k, keep[k].data_ptr())))
    for k in ("stance", "swing_pos", "swing_vel"):
        cases.append((f"extra {k}", lambda bi, c, bo, k=k: setattr(bi, k, (d_st if k == "stance" else keep["joint_q"]).data_ptr())))
    for k in ("grf_body", "status", "joint_tau"):
        cases.append((f"missing out {k}", lambda bi, c, bo, k=k: setattr(bo, k, None)))
    cases += [("missing state", lambda bi, c, bo: setattr(c, "state", None)),
              ("fresh without twist", lambda bi, c, bo: setattr(c, "twist", None)),
              ("struct_size small", lambda bi, c, bo: setattr(c, "struct_size", C.sizeof(c) - 8)),
              ("struct_size zero", lambda bi, c, bo: setattr(c, "struct_size", 0)),
              ("nan stand_height", lambda bi, c, bo: setattr(c, "stand_height", float("nan"))),
              ("negative stand_tol", lambda bi, c, bo: setattr(c, "stand_tol", -1.0)),
              ("inf cmd_dt", lambda bi, c, bo: setattr(c, "cmd_dt", float("inf")))]
    torch.cuda.synchronize()
    for name, spoil in cases:
        bi, c, bo = valid()
        spoil(bi, c, bo)
        rc = lib.qc_tick_batch(ctl._h, n, C.byref(bi), C.byref(c), None, C.byref(bo), None)
        assert rc == -1, name
        msg = _lib.last_error()
        assert msg.startswith("qc_tick_batch:") and len(msg) > 20, (name, msg)
    for k, v in (("null in", (None, "c")), ("null cmd", ("bi", None)), ("null out", ("bi", "c"))):
        bi, c, bo = valid()
        args = [C.byref(bi) if v[0] else None, C.byref(c) if v[1] else None, C.byref(bo) if k != "null out" else None]
        assert lib.qc_tick_batch(ctl._h, n, args[0], args[1], None, args[2], None) == -1, k
    torch.cuda.synchronize()
    assert (out["status"] == -1).all() and (out["grf_body"] == 5.0).all() and (out["joint_tau"] == 5.0).all()
    assert _state_host(q, d_state).tobytes() == st0.tobytes()
    assert np.array_equal(d_phase.cpu().numpy(), base["gait_phase"])
    # and the valid call runs: the gait was running, so the command is applied in this very tick
    bi, c, bo = valid()
    assert lib.qc_tick_batch(ctl._h, n, C.byref(bi), C.byref(c), None, C.byref(bo), None) == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert (out["status"] != -1).all() and not np.array_equal(d_phase.cpu().numpy(), base["gait_phase"])
    s = _state_host(q, d_state)
    assert (s["cmd_pending"] == 0).all() and (s["x_d"][:, 2] == 0.26).all()
    # the Python layer refuses a desired state in the batch
    with pytest.raises(ValueError, match="desired state"):
        ctl.tick_batch(dict(keep, gait_phase=d_phase, gait_dt=d_dt, swing_state=d_swing), dict(state=d_state))
