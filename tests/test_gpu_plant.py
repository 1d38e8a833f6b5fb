"""GPU: qc_plant_step_batch and BalanceController.rollout against the CPU restatements (tests/plant_restatement.py).

Batch sizes 1, 63, 64, 65, 257 and 4097: below, at and above a wave (64 lanes), above a block (256) and a tail behind 16 full
blocks.  Every reference is computed once per module on a pool of robots that the batches tile.

The one-step bars (test_one_step_against_50_digits) are the ones plant_restatement.Er derives along the chain of operations of
the model: every operation passes its operands' bounds on through its derivatives and adds one rounding of a result no larger
than the condition sum of its terms; sin h / h and cos h carry sincos_joint's pinned bars (2 EPS relative, 1 EPS).  On an
ordinary robot they come to 1 - 4 EPS for an entry of Rwb and of feet, one ulp of x and xdot, and ~100 - 200 EPS for w, whose
largest term dt Ib^-1 (r x f) is ~2 rad/s behind sums of ~20 terms (tests/test_plant_cpu.py shows both, and that a plain double
evaluation stays inside them)."""
import ctypes
import functools

import numpy as np
import pytest

from tests import plant_restatement as PR
from tests.gpu_arrays import SENTINEL, P, _device_arrays, _tile, _worst_over_bar, ctl, q  # noqa: F401
from tests.solved_batch_support import assert_raw_refusals

pytestmark = pytest.mark.gpu
EPS = PR.EPS
SIZES = (1, 63, 64, 65, 257, 4097)
STATE = ("Rwb", "x", "xdot", "w")
POOL = 257
FEET_XY = np.array([[-0.196, 0.127], [0.196, 0.127], [-0.196, -0.127], [0.196, -0.127]])


@functools.lru_cache(maxsize=None)
def _pool():
    """POOL robots: row 0 the identity, row 1 a rotation by nearly pi, the others random orthonormal; forces of the size config 3
    produces (normal up to 80 N, lateral up to 20 N) with 30 % of the legs at zero; w = 0 exactly (rows 0, 4, ...), +-1e-12
    (rows 1, 5, ...) and a few rad/s; every second row of the first two kinds carries no force at all, so that the step angle is
    0 exactly, tiny, and ordinary."""
    from scipy.spatial.transform import Rotation

    rng = np.random.default_rng(0x91A27)
    n = POOL
    rv = rng.normal(size=(n, 3))
    rv *= (rng.uniform(0, np.pi, n) / np.linalg.norm(rv, axis=1))[:, None]
    rv[0] = 0.0
    rv[1] = np.array([1.0, 2.0, -2.0]) / 3.0 * (np.pi - 1e-9)
    R = Rotation.from_rotvec(rv).as_matrix()
    assert np.array_equal(R[0], np.eye(3))
    pw = np.zeros((n, 4, 3))
    pw[:, :, :2] = FEET_XY + rng.uniform(-0.03, 0.03, (n, 4, 2))
    grf = rng.uniform(-1, 1, (n, 4, 3)) * np.array([20.0, 20.0, 40.0]) - np.array([0.0, 0.0, 40.0])
    grf[rng.random((n, 4)) < 0.3] = 0.0
    w = rng.uniform(-3, 3, (n, 3))
    w[0::4] = 0.0
    w[1::4] = 1e-12 * rng.choice([-1.0, 1.0], w[1::4].shape)
    grf[0::8] = 0.0
    grf[1::8] = 0.0
    c = np.ascontiguousarray
    return dict(Rwb=c(R.reshape(n, 9)), x=c(np.array([0.0, 0.0, 0.26]) + rng.uniform(-0.05, 0.05, (n, 3))), xdot=c(rng.uniform(-0.5, 0.5, (n, 3))),
                w=c(w), grf_body=c(grf.reshape(n, 12)), foot_world=c(pw.reshape(n, 12)))


@functools.lru_cache(maxsize=None)
def _pool_reference(dt):
    import quadruped_control_amd as q

    P, s = q.cheetah_params(), _pool()
    refs = [PR.plant_step_mp(P["mass"], P["Ib"], *(s[k][i] for k in STATE + ("grf_body", "foot_world")), dt) for i in range(POOL)]
    return {k: (np.stack([r[k][0] for r in refs]), np.stack([r[k][1] for r in refs])) for k in STATE + ("feet",)}


def _step(ctl, host, n, dt, feet="own"):
    """One plant step over n robots (the pool tiled).  feet: "own" (an array of its own), "alias" (written over foot_world) or
    None.  Returns {name: host array [n + 2, k]} of every array after the step, the sentinel rows included."""
    import torch

    d = _device_arrays(host, n)
    if feet == "own":
        d["feet"] = _device_arrays(dict(feet=np.full((1, 12), SENTINEL)), n)["feet"]
    state = {k: d[k][1] for k in STATE}
    ft = d["feet"][1] if feet == "own" else (d["foot_world"][1] if feet == "alias" else None)
    ctl.plant_step(state, d["grf_body"][1], d["foot_world"][1], dt, feet=ft)
    torch.cuda.synchronize()
    return {k: v[0].cpu().numpy() for k, v in d.items()}


# ------------------------------------------------------------------ 1. one step against the 50-digit reference
@pytest.mark.parametrize("dt", [1e-4, 1.0 / 300.0, 1e-2])
def test_one_step_against_50_digits(ctl, dt):
    """Every output entry within its derived bar (module docstring) of the 50-digit evaluation of the model on the same doubles,
    at every batch size; where the step angle is 0 exactly, Exp = I exactly and Rwb comes back bit for bit."""
    s, ref = _pool(), _pool_reference(dt)
    w1 = ref["w"][0]
    still = np.all(w1 == 0.0, axis=1)
    tiny = ~still & (np.linalg.norm(w1, axis=1) * dt < 1e-13)
    assert still.sum() >= 8 and tiny.sum() >= 8 and (~still & ~tiny).sum() >= 100, (still.sum(), tiny.sum())
    for n in SIZES:
        got = _step(ctl, s, n, dt)
        worst = _worst_over_bar(got, ref, STATE + ("feet",), n, n)
        print(f"dt {dt} n {n}: worst error / bar {worst}")
        assert max(worst.values()) <= 1.0, (n, worst)
        assert np.array_equal(got["Rwb"][:n][_tile(still, n)], _tile(s["Rwb"], n)[_tile(still, n)])


# ------------------------------------------------------------------ 2. in place, and only its own rows
@pytest.mark.parametrize("n", SIZES)
def test_in_place_and_only_its_own_rows(ctl, n):
    """The state arrays are inputs and outputs at once, and `feet` may be any array of its layout: written over foot_world - an
    input of the same robot - it gives bit for bit what a separate array gets, and the state comes out the same either way and
    with feet = NULL.  (A lane that wrote before it had read everything would differ here, and from the reference in test 1.)
    Rows behind row n - 1 keep their sentinels in every array; grf_body and, unless aliased, foot_world are not written."""
    s, dt = _pool(), 1.0 / 300.0
    own, alias, none = _step(ctl, s, n, dt, "own"), _step(ctl, s, n, dt, "alias"), _step(ctl, s, n, dt, None)
    for k in STATE:
        assert np.array_equal(own[k], alias[k]) and np.array_equal(own[k], none[k]), k
    assert np.array_equal(own["feet"], alias["foot_world"])
    assert (own["xdot"][:n, 2] != _tile(s["xdot"], n)[:, 2]).all() and (own["feet"][:n] != SENTINEL).all()  # (every robot did step)
    for run in (own, alias, none):
        for k, a in run.items():
            assert (a[n:] == SENTINEL).all(), k
        assert np.array_equal(run["grf_body"][:n], _tile(s["grf_body"], n))
    assert np.array_equal(own["foot_world"][:n], _tile(s["foot_world"], n)) and np.array_equal(none["foot_world"][:n], _tile(s["foot_world"], n))


# ------------------------------------------------------------------ 3. orthonormality under iteration
def test_orthonormality_after_1000_steps(ctl):
    """1 000 torque-free steps (no forces: free fall, tumbling at a few rad/s).  The defect D = Rwb Rwb^T - I obeys
    D' = E D E^T + (E E^T - I) + rounding, E = Exp(dt w'); in the Frobenius norm the first term does not grow, so per step
      * the 3x3 product Rwb' = E Rwb: every entry is three products and two sums of terms with sum |E_rk| |R_kc| <= 1, 3 EPS, so
        |delta|_F <= 9 EPS and the defect gains 2 |Rwb'|_2 |delta|_F <= 18 EPS;
      * E itself: its entries are within 5 EPS of a rotation's (the one-step bars of an Rwb' from the identity), |dE|_F <= 15
        EPS, so |E E^T - I|_F <= 30 EPS.
    max |D| <= |D|_F <= 48 EPS per step: 48 * 1000 * EPS = 1.07e-11 after 1 000 steps."""
    import torch

    steps, n, dt = 1000, 65, 1.0 / 300.0
    s = {k: v.copy() for k, v in _pool().items()}
    rng = np.random.default_rng(5)
    s["w"] = rng.uniform(1.0, 4.0, (POOL, 3)) * rng.choice([-1.0, 1.0], (POOL, 3))
    s["grf_body"][:] = 0.0
    d = _device_arrays(s, n)
    state = {k: d[k][1] for k in STATE}
    launch = ctl.plan_plant(state, d["grf_body"][1], d["foot_world"][1], dt)
    for _ in range(steps):
        launch()
    torch.cuda.synchronize()
    R = state["Rwb"].cpu().numpy().reshape(n, 3, 3)
    defect = float(np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max())
    print(f"max |Rwb Rwb^T - I| after {steps} steps: {defect:.3e} (bound {48 * steps * EPS:.3e})")
    assert defect <= 48 * steps * EPS
    turned = np.abs(R - _tile(s["Rwb"], n).reshape(n, 3, 3)).max(axis=(1, 2))
    assert (turned > 0.1).all()  # (they did tumble)
    v = state["xdot"].cpu().numpy()
    assert np.allclose(v[:, 2], _tile(s["xdot"], n)[:, 2] - steps * dt * PR.G, rtol=0, atol=4 * steps * EPS * 40)


# ------------------------------------------------------------------ 4. one closed-loop step against the checker
@functools.lru_cache(maxsize=None)
def _recorded_rollout(n, steps):
    import torch

    import quadruped_control_amd as q

    P = q.cheetah_params()
    c = q.BalanceController.from_params(P, device=0)
    b, pw = PR.rollout_start(n)
    dev = q.to_device(b)
    state, out = c.rollout(dev, torch.from_numpy(pw).cuda(), steps=steps, dt=1.0 / 300.0, record_every=1)
    torch.cuda.synchronize()
    hist = [{k: t.cpu().numpy() for k, t in rec.items()} for _, rec in out["history"]]
    hist.append({k: dev[k].cpu().numpy() for k in STATE + ("feet",)})
    res = dict(history=hist, status=out["status"].cpu().numpy(), grf=out["grf_body"].cpu().numpy(), start=b, foot_world=pw)
    c.close()
    return res


@pytest.mark.parametrize("k", [0, 10, 50])
def test_closed_loop_step_against_the_checker(P, k):
    """From the DEVICE's state before step k of a rollout (config-2 states): the C oracle's forces, one step of the model on them
    (50 digits), against the device's state after step k.  The plant is linear in the forces, so the project's force bar -
    1e-6 max(1, max |GRF|) per component, df - propagates as
      xdot: dt 4 df / m,   x: dt times that,   w: dt |Iw^-1|_2 sum |r_i| |df_i| <= dt / min(Ib) * 4 r_max sqrt(3) df,
      Rwb:  |dRwb|_2 <= dt |dw|_2 (the rotation by dt w' moves by at most the angle's change),
      feet: |dRwb|_2 r_max + |dx|_2,
    each added to the one-step bar of test 1.  Step by step, so that the closed loop's own dynamics do not amplify a legitimate
    force difference."""
    from oracle import c_oracle

    n, dt = 65, 1.0 / 300.0
    rec = _recorded_rollout(n, 52)
    before, after = rec["history"][k], rec["history"][k + 1]
    batch = dict(rec["start"], **before)
    grf, status, _ = c_oracle.control_batch(P, batch)
    assert (status == 0).all() and (rec["status"] == 0).all()
    pw = rec["foot_world"]
    df = 1e-6 * np.maximum(1.0, np.abs(grf).max(axis=1))
    r_max = np.linalg.norm(pw.reshape(n, 4, 3) - before["x"][:, None, :], axis=2).max(axis=1)
    d_v = dt * 4 * df / P["mass"]
    d_w = dt / np.min(np.diagonal(np.asarray(P["Ib"]).reshape(3, 3))) * 4 * r_max * np.sqrt(3.0) * df
    d_R = dt * np.sqrt(3.0) * d_w
    extra = dict(xdot=d_v, x=dt * d_v, w=d_w, Rwb=d_R, feet=d_R * r_max + np.sqrt(3.0) * dt * d_v)
    worst = {}
    for i in range(n):
        ref = PR.plant_step_mp(P["mass"], P["Ib"], *(before[name][i] for name in STATE), grf[i], pw[i], dt)
        for name, (val, bar) in ref.items():
            ratio = np.abs(after[name][i] - val) / (bar + extra[name][i])
            worst[name] = max(worst.get(name, 0.0), float(ratio.max()))
    print(f"step {k}: worst error / bar {worst}")
    assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------ 5. the whole rollout against the CPU loop
def test_rollout_against_the_cpu_loop(q, P):
    """200 steps at dt = 1/300 on the device against the oracle-in-the-loop CPU restatement from the same start (config-2 states,
    65 robots; the oracle solves every robot at every step of it - asserted here and in tests/test_plant_cpu.py).  The tolerance
    is 10 x the spread of the CPU loop's own final state under a 1e-6 relative perturbation of every force (the project's
    parity bar) - the factor is for another perturbation direction, not another size.  Measured spread (max over robots and
    entries): Rwb 5.0e-8, x 8.1e-9, xdot 9.0e-8, w 1.0e-5, feet 1.3e-8; it is measured again here, and the test uses what it
    measures."""
    import torch

    n, steps, dt = 65, 200, 1.0 / 300.0
    b, pw = PR.rollout_start(n)
    cpu, status = PR.cpu_rollout(P, b, pw, steps, dt)
    assert (status == 0).all()
    cpu_p, status_p = PR.cpu_rollout(P, b, pw, steps, dt, perturb=1e-6)
    assert (status_p == 0).all()
    spread = {k: float(np.abs(cpu_p[k] - cpu[k]).max()) for k in STATE + ("feet",)}
    c = q.BalanceController.from_params(P, device=0)
    dev = q.to_device(b)
    state, out = c.rollout(dev, torch.from_numpy(pw).cuda(), steps=steps, dt=dt)
    torch.cuda.synchronize()
    assert (out["status"].cpu().numpy() == 0).all() and "history" not in out and state["x"] is dev["x"]
    diff = {k: float(np.abs(dev[k].cpu().numpy() - cpu[k]).max()) for k in STATE + ("feet",)}
    print(f"spread under 1e-6 force perturbation {spread}\ndevice - CPU loop {diff}")
    for k in diff:
        assert diff[k] <= 10 * spread[k], (k, diff[k], spread[k])
    # warm-started and cold solves walk to the same minimisers: the rollout without the fed-back working sets agrees as well
    dev2 = q.to_device(b)
    c.rollout(dev2, torch.from_numpy(pw).cuda(), steps=steps, dt=dt, warm=False)
    torch.cuda.synchronize()
    for k in diff:
        assert float(np.abs(dev2[k].cpu().numpy() - cpu[k]).max()) <= 10 * spread[k], k
    c.close()


# ------------------------------------------------------------------ 6. argument errors
def test_argument_errors_launch_nothing(q, ctl):
    """Each rejected call returns QC_ERR_INVALID with a message of qc_plant_step_batch's own and leaves the state as it was.
    Every pointer that is handed over is a valid device array of the right size."""
    import torch

    from quadruped_control_amd import _lib

    lib, n = _lib.load(), 65
    d = _device_arrays(_pool(), n)
    feet = torch.full((n, 12), SENTINEL, dtype=torch.float64, device="cuda")
    before = {k: v[0].clone() for k, v in d.items()}
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def io(**kw):
        s = _lib.QcPlantIo()
        lib.qc_default_plant(ctypes.byref(s))
        for k in STATE + ("grf_body", "foot_world"):
            setattr(s, k, d[k][1].data_ptr())
        s.feet = feet.data_ptr()
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def untouched(what):
        for k, v in d.items():
            assert torch.equal(v[0], before[k]), (what, k)

    def refused(handle, s, what):
        rc = lib.qc_plant_step_batch(handle, n, ctypes.byref(s), stream)
        assert rc == -1 and _lib.last_error().startswith("qc_plant_step_batch:"), (what, rc, _lib.last_error())
        torch.cuda.synchronize()
        untouched(what)
        assert (feet == SENTINEL).all(), what

    for k in STATE + ("grf_body", "foot_world"):
        refused(ctl._h, io(**{k: None}), f"{k} = NULL")
    refused(ctl._h, io(struct_size=0), "struct_size not set")
    for dt in (0.0, -1.0 / 300.0, float("nan"), float("inf")):
        refused(ctl._h, io(dt=dt), f"dt = {dt}")
    # a handle whose inertia no rigid body has: qc_create takes it (the wrench law reads nothing of it), the plant does not
    P = dict(q.cheetah_params())
    P["Ib"] = np.diag([0.011253, -0.036203, 0.042673])
    odd = q.BalanceController.from_params(P, device=0)
    refused(odd._h, io(), "Ib not positive definite")
    assert "positive definite" in _lib.last_error()
    with pytest.raises(RuntimeError, match="qc_plant_step_batch:"):
        odd.plant_step({k: d[k][1] for k in STATE}, d["grf_body"][1], d["foot_world"][1], 1.0 / 300.0)
    odd.close()
    # the Python wrapper checks shapes before it calls
    with pytest.raises(ValueError, match="grf_body"):
        ctl.plant_step({k: d[k][1] for k in STATE}, d["grf_body"][1][:, :6].contiguous(), d["foot_world"][1], 1.0 / 300.0)

    def stepped():
        assert not torch.equal(d["x"][0][:n], before["x"][:n]) and (d["x"][0][n:] == SENTINEL).all(), "x after the valid call"

    # no handle, no io, n beyond one launch, a struct_size of another revision; n = 0 is no error and launches nothing; the same
    # call with everything in order does step
    assert_raw_refusals(lib.qc_plant_step_batch, lambda: (ctl._h, n, None, io()), "qc_plant_io", ctypes.sizeof(_lib.QcPlantIo), 64,
                        [(feet, SENTINEL, True)], beyond=0xFFFFFF * 256 + 1, stream=stream, untouched=untouched, launched=stepped)
