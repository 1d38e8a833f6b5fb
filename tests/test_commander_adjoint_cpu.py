"""CPU tests of the commander step and its reverse pass (qc_commander_step_batch, qc_commander_step_adjoint_batch): the restated forward
against commander_restatement.Commander, the float64 reverse pass against 50 digits and against central differences, the pass-through,
zeroing and flag rules, the host logic of the two entry points, the exported symbols.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np

from tests import commander_adjoint_restatement as CA
from tests import commander_restatement as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 257


def _pool():
    st, Rwb, x, twist, fresh, kinds = CA.pool(N)
    return st, Rwb, x, twist, fresh, np.array(kinds)


def test_pool_covers_every_branch():
    st, Rwb, x, twist, fresh, kinds = _pool()
    _, out = CA.step_np(st, Rwb, x, twist, fresh)
    applied, run = out["applied"].astype(bool), out["run"].astype(bool)
    f = fresh.astype(bool)
    assert (applied & f).any() and (applied & ~f).any() and (run & ~applied).any() and (~run & f).any() and (~run & ~f).any()
    d = np.linalg.norm(twist[:, 3:6], axis=1) * CA.SCALARS["cmd_dt"]
    assert (d[kinds == "om0"] == 0.0).all() and applied[kinds == "om0"].all()
    assert ((d[kinds == "below"] < 1e-12) & (d[kinds == "below"] > 0)).all() and ((d[kinds == "above"] > 1e-12) & (d[kinds == "above"] < 1e-11)).all()
    yaw = np.arctan2(Rwb[kinds == "yaw_pi", 3], Rwb[kinds == "yaw_pi", 0])
    assert (np.pi - np.abs(yaw) < 2e-3).all() and (yaw > 0).any() and (yaw < 0).any()
    assert applied[kinds == "latch_applied"].all() and not run[kinds == "latching"].any()


def test_forward_equals_the_commander_restatement_bit_for_bit():
    """three ticks on the pool: fresh on the first, nothing on the second, a second command for every third robot on the last"""
    st, Rwb, x, twist, fresh, _ = _pool()
    C = CR.Commander(N)
    C.standing[:], C.gait_running[:], C.cmd_pending[:] = st["standing"], st["gait_running"], st["cmd_pending"]
    C.Vb[:], C.Rwb_d[:], C.x_d[:], C.xdot_d[:], C.w_d[:] = st["Vb"], st["Rwb_d"], st["x_d"], st["xdot_d"], st["w_d"]
    again = (np.arange(N) % 3 == 0).astype(np.uint8)
    for tw, fr in ((twist, fresh), (None, None), (-twist, again)):
        st, out = CA.step_np(st, Rwb, x, tw, fr)
        run, applied = C.step(Rwb, x, tw, fr)
        assert np.array_equal(run, out["run"].astype(bool)) and np.array_equal(applied, out["applied"].astype(bool))
        assert np.array_equal(C.flags(), np.stack([st["standing"], st["gait_running"], st["cmd_pending"]], axis=1))
        for k, v in C.desired().items():
            assert np.array_equal(v, st[k]) and np.array_equal(v, out[k]), k
        assert np.array_equal(C.Vb, st["Vb"])


def test_reverse_pass_against_50_digits():
    """Every output of the float64 reverse pass within C_REF x EPS x condition sum of the 50-digit one, on the whole pool - om = 0, |d|
    either side of 1e-12, yaw near +-pi included.  The measured ratios are printed; C_REF holds them rounded up."""
    st, Rwb, x, twist, fresh, kinds = _pool()
    bars, ins = CA.cotangents(N), CA.accumulators(N)
    val, flags = CA.adjoint_np(st, Rwb, x, twist, fresh, bars, **ins)
    ref, cond, flags_mp = CA.adjoint_mp(st, Rwb, x, twist, fresh, bars, **ins)
    assert not flags.any() and not flags_mp.any()
    ratios = {k: CA.worst_ratio(val[k], ref[k], cond[k]) for k in CA.OUTPUTS}
    print("float64 reverse pass / 50 digits, worst |difference| / (EPS x condition sum):", {k: round(v, 3) for k, v in ratios.items()})
    for k in CA.OUTPUTS:
        assert ratios[k] <= CA.C_REF[k], (k, ratios[k])
        assert ratios[k] >= 0.25 * CA.C_REF[k] or ratios[k] == 0.0, f"C_REF['{k}'] = {CA.C_REF[k]} is far above the measurement {ratios[k]}"
    # a yaw-rate command must get a gradient at om = 0 and below the forward pass's branch
    for kind in ("om0", "below"):
        rows = kinds == kind
        assert (np.abs(val["twist_bar"][rows, 3:6]).max(axis=1) > 1e-6).all()
        assert (np.abs(ref["twist_bar"][rows, 3:6]).max(axis=1) > 1e-6).all()


def test_reverse_pass_against_central_differences():
    """<bars, d out> by central differences of the restated forward in Rwb, x, twist / Vb against <gradient, direction>: the applied
    robots off the |d| < 1e-12 branch, where the forward pass is the analytic function (h = 1e-6: truncation 1e-12, rounding 1e-10)."""
    st, Rwb, x, twist, fresh, kinds = _pool()
    bars = CA.cotangents(N)
    val, _ = CA.adjoint_np(st, Rwb, x, twist, fresh, bars)
    _, out0 = CA.step_np(st, Rwb, x, twist, fresh)
    rows = out0["applied"].astype(bool) & ~np.isin(kinds, ("om0", "below", "above"))
    rng = np.random.default_rng(5)
    dR, dx, dv = rng.uniform(-1, 1, (N, 9)), rng.uniform(-1, 1, (N, 3)), rng.uniform(-1, 1, (N, 6))
    dx[:, 2] = 0.0  # (the latch reads x_z: held)
    h = 1e-6

    def loss(s):
        st2 = st.copy()
        st2["Vb"] = st["Vb"] + s * h * dv
        new, out = CA.step_np(st2, Rwb + s * h * dR, x + s * h * dx, twist + s * h * dv, fresh)
        return sum((bars[k] * out[k]).sum(axis=1) for k in ("Rwb_d", "x_d", "xdot_d", "w_d")) + (bars["Vb"] * new["Vb"]).sum(axis=1)

    fd = (loss(1.0) - loss(-1.0)) / (2 * h)
    an = (val["Rwb_bar"] * dR).sum(axis=1) + (val["x_bar"] * dx).sum(axis=1) + ((val["twist_bar"] + val["Vb_bar"]) * dv).sum(axis=1)
    err = np.abs(fd - an)[rows].max()
    print(f"{rows.sum()} applied robots: worst |central difference - analytic| {err:.2e}")
    assert rows.sum() > 50 and err < 1e-7


def test_pass_through_and_zeroing_rules():
    st, Rwb, x, twist, fresh, _ = _pool()
    bars, ins = CA.cotangents(N), CA.accumulators(N)
    val, _ = CA.adjoint_np(st, Rwb, x, twist, fresh, bars, **ins)
    _, out = CA.step_np(st, Rwb, x, twist, fresh)
    a, f = out["applied"].astype(bool), fresh.astype(bool)
    for k in ("Rwb_d", "x_d", "xdot_d", "w_d"):
        assert np.array_equal(val[k + "_prev_bar"][~a], bars[k][~a]) and not val[k + "_prev_bar"][a].any()
    assert np.array_equal(val["Rwb_bar"][~a], ins["Rwb_bar_in"][~a]) and np.array_equal(val["x_bar"][~a], ins["x_bar_in"][~a])
    assert not val["Vb_bar"][f].any() and not val["twist_bar"][~f].any()
    assert np.array_equal(val["twist_bar"][f & ~a], bars["Vb"][f & ~a]) and np.array_equal(val["Vb_bar"][~f & ~a], bars["Vb"][~f & ~a])
    # x_d_bar[2] is dropped: the height is a constant
    b2 = dict(bars, x_d=bars["x_d"] * np.array([1.0, 1.0, -3.0]))
    val2, _ = CA.adjoint_np(st, Rwb, x, twist, fresh, b2, **ins)
    for k in ("twist_bar", "Vb_bar", "Rwb_bar", "x_bar"):
        assert np.array_equal(val[k][a], val2[k][a])
    # a missing cotangent is a zero one
    only = {"xdot_d": bars["xdot_d"]}
    zeros = {k: (bars[k] if k == "xdot_d" else np.zeros_like(bars[k])) for k in bars}
    v1, _ = CA.adjoint_np(st, Rwb, x, twist, fresh, only)
    v2, _ = CA.adjoint_np(st, Rwb, x, twist, fresh, zeros)
    for k in CA.OUTPUTS:
        assert np.array_equal(v1[k], v2[k])


def test_flag_rule():
    st, Rwb, x, twist, fresh, _ = _pool()
    _, out = CA.step_np(st, Rwb, x, twist, fresh)
    a = np.nonzero(out["applied"])[0]
    idle = np.nonzero(out["applied"] == 0)[0]
    lock = np.array([a[0], a[5], idle[0]])
    Rwb = Rwb.copy()
    Rwb[lock] = np.array([0.0, 0.0, 1.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.0])  # pitch = pi / 2: R00 = R10 = 0
    bars = CA.cotangents(N)
    val, flags = CA.adjoint_np(st, Rwb, x, twist, fresh, bars)
    _, _, flags_mp = CA.adjoint_mp(st[:12], Rwb[:12], x[:12], twist[:12], fresh[:12], {k: v[:12] for k, v in bars.items()})
    assert flags[lock[:2]].tolist() == [1, 1] and flags.sum() == 2 and np.array_equal(flags[:12], flags_mp)
    for k in CA.OUTPUTS:
        assert np.isnan(val[k][lock[:2]]).all() and np.isfinite(np.delete(val[k], lock[:2], axis=0)).all()


def test_host_logic_runs_clean():
    """tests/cpp/commander_step_host_test.cpp: every refusal of check_commander_step_args and check_commander_step_adjoint_args,
    sanitized, stand-alone."""
    import __graft_entry__ as g

    exe = g.build_host_test("commander_step_host_test")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "commander step host logic ok" in r.stdout


def test_exported_symbols():
    from quadruped_control_amd import _lib
    from quadruped_control_amd.balance_controller import COMMANDER_STATE_DTYPE

    names = ("qc_default_commander_step", "qc_commander_step_batch", "qc_default_commander_step_adjoint", "qc_commander_step_adjoint_batch")
    for name in names:
        assert name in _lib.EXPORTS
    if os.path.exists(_lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
        for name in names:
            assert f" T {name}\n" in out
        assert _lib.load().qc_abi_version() == 6 and _lib.ABI_VERSION == 6  # new entry points, no change to what existed
    assert ctypes.sizeof(_lib.QcCommanderStepIo) == 7 * 8 and ctypes.sizeof(_lib.QcCommanderStepAdjointIo) == 18 * 8
    assert CA.STATE_DTYPE == COMMANDER_STATE_DTYPE
