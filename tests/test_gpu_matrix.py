"""-m gpu: oracle parity over EVERY kernel instantiation the launch planner can pick.

The planner (plan_launch, qc_host.hpp) chooses by formulation (uniform 6x6 / general 6x6 / dense 12x12),
lanes per robot (1 / 2 / 4) and kernel mode (1 one fill per wave, 2 one fill
with register-resident constants, 3 paired waves: two one-lane waves per workgroup, the last to arrive finishes both
waves' stragglers from a list in LDS).  Each test forces one branch with qc_set_tuning, checks through qc_query_launch
that this branch is the one that runs, and compares with the C oracle on config-3 inputs (mixed 2/3/4-foot contact
states), cold and warm-started; the joint_q / joint_tau (KIN) instantiations run the fused tick against the oracle's
composition.  Cold runs of all forms must also take the same working-set path (identical iteration counts).
Reference semantics held: balance_controller.cpp:152-153 (QP data), 274-330 (constraint rows).
"""
import numpy as np
import pytest

from tests.gpu_arrays import q  # noqa: F401

pytestmark = pytest.mark.gpu

RTOL = 1e-6  # of max|GRF| per robot; north_star's bar is 1e-4
FORMS = {"uniform": {}, "general": {"force_general": 1}, "dense": {"force_dense": 1}}
FORM_ID = {"uniform": 0, "general": 1, "dense": 2}
# (form, lanes per robot, mode) -> (tuning, robots): every row of kernel_row_for()
CASES = []
for form in ("uniform", "general"):
    CASES += [(form, 1, 1, dict(group=1, one_fill=1), 8200),  # ragged: the last wave holds 8 robots
              (form, 2, 1, dict(group=2, one_fill=1), 8200),  # ragged: the last wave holds 8 robots
              (form, 4, 1, dict(group=4, one_fill=1, race=0), 20480 if form == "uniform" else 8192)]
    CASES += [(form, 1, 3, dict(group=1, pair=1), 8200 + 64 + 13)]  # paired waves: 65 workgroups, the last one with a ragged second wave
CASES += [("uniform", 4, 2, dict(group=4, one_fill=1, race=0), 8192),
          ("dense", 1, 1, dict(group=1, one_fill=1), 8200),  # ragged; the Hessian planes are the workgroup's only LDS (output stock aliased)
          ("dense", 4, 1, dict(group=4, race=0), 8192)]
IDS = [f"{f}-G{g}-mode{m}" for f, g, m, _, _ in CASES]


_cache = {}


def _inputs(q, n):
    """config-3 robots, their oracle solution, and a 'previous tick' (slightly different commands) for warm starts"""
    if n not in _cache:
        from oracle import c_oracle as O
        from quadruped_control_amd import workloads as W

        P = q.cheetah_params(0.6)
        b = W.config3(n, seed=0x5EED00A3)
        ref, st, it = O.control_batch(P, b, threads=8)
        assert (st == 0).all()
        prev = dict(b)
        prev["xdot_d"] = b["xdot_d"] * 0.9
        prev["x"] = b["x"] + 1e-3
        _cache[n] = (P, b, ref, prev)
    return _cache[n]


def _controller(q, P, form, tune):
    ctl = q.BalanceController.from_params(P)
    ctl.set_tuning(**FORMS[form])
    ctl.set_tuning(clamp_steps=1, race=0)  # the classic start and drop rule in every kernel: all instantiations walk the same working-set path
    ctl.set_tuning(**tune)
    return ctl


def _relerr(a, ref):
    scale = np.maximum(1.0, np.abs(ref).max(axis=1, keepdims=True))
    return float(np.max(np.abs(a - ref) / scale))


_iters = {}


@pytest.mark.parametrize("form,G,mode,tune,n", CASES, ids=IDS)
@pytest.mark.parametrize("start", ["cold", "warm"])
def test_kernel_instantiation_vs_oracle(q, form, G, mode, tune, n, start):
    import torch

    from tests.kkt_batch import assert_kkt

    P, b, ref, prev = _inputs(q, n)
    ctl = _controller(q, P, form, tune)
    info = ctl.query_launch(n, warm=(start == "warm"))
    assert (info["form"], info["lanes_per_robot"], info["mode"]) == (FORM_ID[form], G, mode), info
    d = q.to_device(b)
    warm = None
    if start == "warm":
        o0 = q.BalanceController.from_params(P).control_batch(q.to_device(prev), want_active_set=True)
        warm = o0["active_set"]
    o = ctl.control_batch(d, warm=warm, want_iterations=True, want_active_set=True)
    torch.cuda.synchronize()
    assert int((o["status"] != 0).sum()) == 0
    grf = o["grf_body"].cpu().numpy()
    assert _relerr(grf, ref) < RTOL
    assert np.all(grf[np.repeat(b["stance"] == 0, 3, axis=1)] == 0.0)
    assert_kkt(P, b, grf)
    it = o["iterations"].cpu().numpy()
    assert it.min() >= 1 and it.max() <= 200
    if start == "cold":
        _iters[(form, G, mode)] = it
        first = next(iter(_iters.values()))
        if first.shape == it.shape:  # same batch: every form walks the same working-set path
            assert np.array_equal(first, it), (np.flatnonzero(first != it)[:10], IDS)
    else:
        cold = _iters.get((form, G, mode))
        if cold is not None:
            assert it.mean() < 0.8 * cold.mean(), (it.mean(), cold.mean())
        # restarting from the optimal working set takes exactly one recalculation
        again = ctl.control_batch(d, warm=o["active_set"], want_iterations=True)
        torch.cuda.synchronize()
        assert int(again["iterations"].max()) == 1
        assert _relerr(again["grf_body"].cpu().numpy(), ref) < RTOL


# every one-fill branch, both dense widths
KIN_CASES = [c for c in CASES if c[2] != 3]  # (mode 3 has no joint_q variant)


@pytest.mark.parametrize("form,G,mode,tune,n", KIN_CASES, ids=[f"kin-{f}-G{g}-mode{m}" for f, g, m, _, _ in KIN_CASES])
def test_kin_instantiation_vs_oracle(q, form, G, mode, tune, n):
    """joint_q in / joint_tau out variants (KIN = true template instantiations) of the same branches."""
    from oracle import c_oracle as O
    from quadruped_control_amd import workloads as W

    n = min(n, 8192) if not (form == "uniform" and G == 4 and mode == 1) else n
    P = q.cheetah_params(0.6)
    b = W.with_joint_angles(W.config3(n, seed=0x5EED00A4))
    ctl = _controller(q, P, form, tune)
    info = ctl.query_launch(n, kin=True)
    assert (info["form"], info["lanes_per_robot"], info["mode"]) == (FORM_ID[form], G, mode), info
    o = ctl.control_batch_host(b, want_torques=True)
    ref = O.tick_batch(P, b, threads=8)
    assert (o["status"] == 0).all() and (ref["status"] == 0).all()
    assert _relerr(o["grf_body"], ref["grf_body"]) < RTOL
    assert np.max(np.abs(o["joint_tau"] - ref["joint_tau"])) < 1e-6 * 20.0


def test_config5_shard_full_size(q):
    """BASELINE.json configs[4]: one rank's shard of the 2,097,152-robot batch (rank 3 of 8: robots
    [786432, 1048576), seed 0x5EED0005) at full size - every robot solved, feasible and KKT-certified, a
    16,384-robot sample against the oracle, and shards generated independently tile the batch exactly."""
    import torch

    from tests.kkt_batch import assert_kkt
    from oracle import c_oracle as O
    from quadruped_control_amd import workloads as W
    from quadruped_control_amd.sharding import shard_bounds

    total, world, rank = 2097152, 8, 3
    lo, hi = shard_bounds(total, rank, world)
    assert (lo, hi) == (786432, 1048576)
    P = q.cheetah_params(0.6)
    b = W.config5(hi - lo, start=lo)
    ctl = q.BalanceController.from_params(P)
    o = ctl.control_batch(q.to_device(b), want_iterations=True)
    torch.cuda.synchronize()
    assert int((o["status"] != 0).sum()) == 0
    grf = o["grf_body"].cpu().numpy()
    assert_kkt(P, b, grf)
    idx = np.random.default_rng(5).choice(hi - lo, 16384, replace=False)
    sub = {k: np.ascontiguousarray(v[idx]) for k, v in b.items()}
    ref, st, _ = O.control_batch(P, sub, threads=8)
    assert (st == 0).all() and _relerr(grf[idx], ref) < RTOL
    # the same robots as part of a differently cut batch (rank 1 of 4 owns [524288, 1048576)) give the same forces
    lo4, hi4 = shard_bounds(total, 1, 4)
    b4 = W.config5(hi4 - lo4, start=lo4)
    o4 = ctl.control_batch(q.to_device(b4))
    torch.cuda.synchronize()
    g4 = o4["grf_body"].cpu().numpy()[lo - lo4:hi - lo4]
    scale = np.maximum(1.0, np.abs(grf).max(axis=1, keepdims=True))
    assert np.max(np.abs(g4 - grf) / scale) < 1e-8
    hist = np.bincount(b["stance"].sum(axis=1), minlength=5)
    assert hist[2] > 0 and hist[3] > 0 and hist[4] > 0  # mixed 2/3/4-foot contact states


@pytest.mark.parametrize("cap", [1, 2, 3, 6, 9])
def test_iteration_cap_and_bad_inputs_agree_across_widths(q, cap):
    """The recalculation cap (nWSR_ analogue) and non-finite inputs across the re-pack: a robot that runs out of
    recalculations - in the one- or two-lane stage or later in the four-lane tail - and a robot with NaN inputs must
    end with the same status, iteration count and (zero) forces whichever lane-group width solved it."""
    from quadruped_control_amd import workloads as W

    n = 5000
    P = q.cheetah_params(0.6)
    b = W.config3(n, seed=0x5EED00A5)
    bad = np.arange(7, n, 611)
    b["x"][bad[::2], 1] = np.nan
    b["Rwb"][bad[1::2], 4] = np.inf
    outs = {}
    for g in (4, 2, 1, "pair"):
        ctl = q.BalanceController.from_params(P, max_iter=cap).set_tuning(group=1 if g == "pair" else g, one_fill=1, race=0, clamp_steps=1)  # one strategy, one start: the widths must agree exactly
        if g == "pair":  # the paired-waves kernel (mode 3): the cap may strike in the producer or in the list's consumer
            ctl.set_tuning(pair=1)
            assert ctl.query_launch(n)["mode"] == 3
        else:
            assert ctl.query_launch(n)["lanes_per_robot"] == g
        outs[g] = ctl.control_batch_host(b, want_iterations=True, want_active_set=True)
    ref = outs[4]
    assert (ref["status"][bad] == 3).all() and np.all(ref["grf_body"][bad] == 0.0)
    capped = ref["status"] == 1
    assert capped.any() if cap < 9 else True
    assert np.all(ref["grf_body"][capped] == 0.0) and (ref["iterations"][capped] == cap).all()
    for g in (2, 1, "pair"):
        o = outs[g]
        assert np.array_equal(o["status"], ref["status"]), g
        assert np.array_equal(o["iterations"], ref["iterations"]), g
        ok = ref["status"] == 0
        scale = np.maximum(1.0, np.abs(ref["grf_body"][ok]).max(axis=1, keepdims=True))
        assert np.max(np.abs(o["grf_body"][ok] - ref["grf_body"][ok]) / scale) < 1e-8
        assert np.all(o["grf_body"][~ok] == 0.0)
    # racing strategies under the same cap: every robot the classic strategy solves is solved (by whichever strategy
    # gets there first, in at most as many recalculations), bad inputs are still reported, and nothing else changes
    r = q.BalanceController.from_params(P, max_iter=cap).set_tuning(group=4, one_fill=1).control_batch_host(b, want_iterations=True)
    assert (r["status"][bad] == 3).all() and np.all(r["grf_body"][bad] == 0.0)
    ok = ref["status"] == 0
    assert (r["status"][ok] == 0).all() and (r["iterations"][ok] <= ref["iterations"][ok]).all()
    assert np.all(r["grf_body"][r["status"] != 0] == 0.0) and (r["iterations"] <= cap).all()
    scale = np.maximum(1.0, np.abs(ref["grf_body"][ok]).max(axis=1, keepdims=True))
    assert np.max(np.abs(r["grf_body"][ok] - ref["grf_body"][ok]) / scale) < 1e-8


@pytest.mark.parametrize("cap", [2, 6, 7, 9, 200])
def test_dense_twin_race_under_caps_bad_inputs_and_ragged_sizes(q, cap):
    """Round 5: the one-lane dense kernel copies its stragglers into the wave's idle lanes (the twin continues with the other drop
    rule; results are stored straight from registers, the lanes that finished before the fork included).  Against the same kernel
    with the race off (race = 0): identical statuses, forces to 1e-8, never more recalculations; a recalculation cap that strikes
    before the fork, at it or in the race, NaN / inf inputs (status 3 on either side of the fork) and batch sizes that leave a
    ragged or a nearly empty last wave.  (A property test of the race itself - the kernel against the same kernel with race = 0;
    the dense one-lane kernel's comparison with the ORACLE is test_kernel_instantiation_vs_oracle above, race on.)"""
    from quadruped_control_amd import workloads as W

    P = q.cheetah_params(0.6)
    for n in (1, 31, 64, 65, 130, 5000):
        b = W.config3(n, seed=0x5EED00A6 + n)
        bad = np.arange(3, n, 97)
        b["x"][bad[::2], 1] = np.nan
        b["Rwb"][bad[1::2], 4] = np.inf
        twin = q.BalanceController.from_params(P, max_iter=cap).set_tuning(force_dense=1, group=1, one_fill=1)
        solo = q.BalanceController.from_params(P, max_iter=cap).set_tuning(force_dense=1, group=1, one_fill=1, race=0)
        info = twin.query_launch(n)
        assert (info["form"], info["lanes_per_robot"], info["mode"]) == (2, 1, 1)
        o = twin.control_batch_host(b, want_iterations=True, want_active_set=True)
        s_ = solo.control_batch_host(b, want_iterations=True)
        assert (o["status"][bad] == 3).all() and np.all(o["grf_body"][bad] == 0.0)
        good = np.setdiff1d(np.arange(n), bad)
        # a robot the classic rule solves within the cap is solved (owner or twin, whoever is first); a capped one reports the cap
        solved_solo = s_["status"] == 0
        assert (o["status"][solved_solo] == 0).all()
        assert (o["iterations"][good] <= s_["iterations"][good]).all() and (o["iterations"] <= cap).all()
        both = (o["status"] == 0) & solved_solo
        if both.any():
            scale = np.maximum(1.0, np.abs(s_["grf_body"][both]).max(axis=1, keepdims=True))
            assert np.max(np.abs(o["grf_body"][both] - s_["grf_body"][both]) / scale) < 1e-8
        assert np.all(o["grf_body"][o["status"] != 0] == 0.0)
        assert set(np.unique(o["status"])) <= {0, 1, 3}
        if cap == 200:
            assert (o["status"][good] == 0).all()
            if n == 5000:
                assert (o["iterations"] < s_["iterations"]).any()  # the race is in force


@pytest.mark.parametrize("form", ["uniform", "general", "dense"])
def test_planner_boundaries_vs_oracle(q, form):
    """Default settings at every batch size where the planner changes the kernel (racing strategies <= 4 096, four lanes
    <= 16 384, two <= 32 768, one above; single robots; ragged last waves), cold and warm-started: oracle parity and the
    launch the planner reports."""
    import torch

    from oracle import c_oracle as O
    from quadruped_control_amd import workloads as W

    P = q.cheetah_params(0.6)
    sizes = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 16383, 16384, 16385, 32767, 32768, 32769, 65535, 65537]
    if form == "dense":
        sizes = [1, 5, 17, 64, 65, 4096, 4097, 16384, 16385, 20001]
    nmax = max(sizes)
    prev, cur = W.config4(nmax, seed=0x5EED00E1)
    mix = W.config3(nmax, seed=0x5EED00E2)
    # mixed contact states for the cold batch, config 4's two ticks (all feet in stance) for the warm one
    ref_cold, st, _ = O.control_batch(P, mix, threads=8)
    ref_warm, st2, _ = O.control_batch(P, cur, threads=8)
    assert (st == 0).all() and (st2 == 0).all()
    ctl = q.BalanceController.from_params(P).set_tuning(**FORMS[form])
    word = ctl.control_batch(q.to_device(prev), want_active_set=True)["active_set"]
    seen = set()
    for n in sizes:
        info = ctl.query_launch(n)
        seen.add((info["lanes_per_robot"], info["mode"], info["strategies"]))
        if form != "dense":
            assert info["lanes_per_robot"] == (4 if n <= 16384 else (2 if n <= 32768 else 1)), (n, info)
            assert info["strategies"] == (4 if n <= 4096 else 1), (n, info)
        cold = ctl.control_batch(q.to_device({k: v[:n] for k, v in mix.items()}), want_iterations=True)
        warm = ctl.control_batch(q.to_device({k: v[:n] for k, v in cur.items()}), warm=word[:n].contiguous(), want_iterations=True)
        torch.cuda.synchronize()
        assert int((cold["status"] != 0).sum()) == 0 and int((warm["status"] != 0).sum()) == 0, n
        assert _relerr(cold["grf_body"].cpu().numpy(), ref_cold[:n]) < RTOL, n
        assert _relerr(warm["grf_body"].cpu().numpy(), ref_warm[:n]) < RTOL, n
        assert float(warm["iterations"].float().mean()) <= float(cold["iterations"].float().mean()) or n < 64, n
    assert len(seen) >= (4 if form != "dense" else 2), seen


@pytest.mark.parametrize("steps", [0, 2, 3, 6])
@pytest.mark.parametrize("form,G", [("uniform", 1), ("uniform", 2), ("uniform", 4), ("general", 1), ("general", 2), ("dense", 1)])
def test_clamp_steps_vs_oracle(q, form, G, steps):
    """One-fill kernels with several clamp steps before the first ratio test (0 = the kernel's own rule: five on one / two
    lanes per robot, cold start): a different walk to the same minimiser - oracle parity, KKT certificate, restart from the
    reported working set in one recalculation, and a warm-started batch is unaffected by the rule."""
    import torch

    from oracle import c_oracle as O
    from tests.kkt_batch import assert_kkt
    from quadruped_control_amd import workloads as W

    P = q.cheetah_params(0.6)
    n = 8200
    b = W.config3(n, seed=0x5EED00C1) if steps in (0, 3) else W.config2(n, seed=0x5EED00C2)
    ref, st, _ = O.control_batch(P, b, threads=8)
    assert (st == 0).all()
    ctl = q.BalanceController.from_params(P).set_tuning(group=G, one_fill=1, race=0, clamp_steps=steps, **FORMS[form])
    info = ctl.query_launch(n)
    assert (info["form"], info["lanes_per_robot"]) == (FORM_ID[form], G) and info["mode"] >= 1, info
    d = q.to_device(b)
    o = ctl.control_batch(d, want_iterations=True, want_active_set=True)
    torch.cuda.synchronize()
    assert int((o["status"] != 0).sum()) == 0
    grf = o["grf_body"].cpu().numpy()
    assert _relerr(grf, ref) < RTOL
    assert_kkt(P, b, grf)
    classic = q.BalanceController.from_params(P).set_tuning(group=G, one_fill=1, race=0, clamp_steps=1, **FORMS[form])
    c = classic.control_batch(d, want_iterations=True, want_active_set=True)
    assert _relerr(c["grf_body"].cpu().numpy(), ref) < RTOL
    it, it_c = o["iterations"].cpu().numpy(), c["iterations"].cpu().numpy()
    if steps == 0 and G < 4:
        assert not np.array_equal(it, it_c)  # the rule really is in force ...
        assert it.mean() < it_c.mean()  # ... and shortens the average walk
    if steps == 0 and G == 4:
        assert np.array_equal(it, it_c)  # four lanes per robot keep the classic start
    again = ctl.control_batch(d, warm=o["active_set"], want_iterations=True)
    torch.cuda.synchronize()
    assert int(again["iterations"].max()) == 1 and _relerr(again["grf_body"].cpu().numpy(), ref) < RTOL
    again_c = classic.control_batch(d, warm=o["active_set"], want_iterations=True)
    assert torch.equal(again["grf_body"], again_c["grf_body"])


@pytest.mark.parametrize("start", ["cold", "warm"])
@pytest.mark.parametrize("form,G,n", [("uniform", 1, 65536), ("uniform", 2, 20000), ("general", 1, 30011), ("general", 2, 8200),
                                      ("dense", 1, 30011), ("dense", 1, 65536)])
def test_tail_race_vs_oracle(q, form, G, n, start):
    """One / two lanes per robot with the product's defaults: the last <= 8 running robots of a wave race two drop
    rules on the 4-lane body - and, in the one-lane dense form (round 5), every robot still running once at most 32 of a wave
    do is copied into an idle lane that continues with the other drop rule (the twin race; 30 011 robots: a ragged last wave).
    Same minimiser as the oracle, KKT-certified, never more recalculations than with the race switched off, fewer for the
    slowest robot of a cold batch, restart from the reported working set in one."""
    import torch

    from oracle import c_oracle as O
    from tests.kkt_batch import assert_kkt
    from quadruped_control_amd import workloads as W

    P = q.cheetah_params(0.6)
    if start == "warm":
        prev, b = W.config4(n, seed=0x5EED00D1)
    else:
        b = W.config3(n, seed=0x5EED00D2)
    ref, st, _ = O.control_batch(P, b, threads=8)
    assert (st == 0).all()
    d = q.to_device(b)
    warm = None
    if start == "warm":
        warm = q.BalanceController.from_params(P).control_batch(q.to_device(prev), want_active_set=True)["active_set"]
    race = q.BalanceController.from_params(P).set_tuning(group=G, one_fill=1, **FORMS[form])
    solo = q.BalanceController.from_params(P).set_tuning(group=G, one_fill=1, race=0, **FORMS[form])
    assert race.query_launch(n)["lanes_per_robot"] == G
    o = race.control_batch(d, warm=warm, want_iterations=True, want_active_set=True)
    s_ = solo.control_batch(d, warm=warm, want_iterations=True)
    torch.cuda.synchronize()
    assert int((o["status"] != 0).sum()) == 0 and int((s_["status"] != 0).sum()) == 0
    grf = o["grf_body"].cpu().numpy()
    assert _relerr(grf, ref) < RTOL and _relerr(s_["grf_body"].cpu().numpy(), ref) < RTOL
    assert np.all(grf[np.repeat(b["stance"] == 0, 3, axis=1)] == 0.0)
    assert_kkt(P, b, grf)
    it_r, it_s = o["iterations"].cpu().numpy(), s_["iterations"].cpu().numpy()
    assert (it_r <= it_s).all() and it_r.min() >= 1
    if start == "warm":
        assert np.array_equal(it_r, it_s)  # warm-started batches keep the classic tail
    if start == "cold":
        assert (it_r < it_s).any() and it_r.max() <= it_s.max()  # the race is really in force
    again = solo.control_batch(d, warm=o["active_set"], want_iterations=True)
    torch.cuda.synchronize()
    assert int(again["iterations"].max()) == 1 and _relerr(again["grf_body"].cpu().numpy(), ref) < RTOL


@pytest.mark.parametrize("n,strategies", [(4096, 4), (2500, 4), (8192, 2), (6000, 2)])
@pytest.mark.parametrize("start", ["cold", "warm"])
@pytest.mark.parametrize("form", ["uniform", "general", "dense"])
def test_racing_strategies_vs_oracle(q, form, n, strategies, start):
    """4-lane kernels with 2 / 4 pivoting strategies racing per robot (batches that leave SIMDs idle), all three
    formulations: same minimiser as the oracle, KKT-certified, and never more recalculations than the classic
    strategy alone needs."""
    import torch

    from oracle import c_oracle as O
    from tests.kkt_batch import assert_kkt
    from quadruped_control_amd import workloads as W

    P = q.cheetah_params(0.6)
    b = W.config2(n, seed=0x5EED00B2) if n in (4096, 8192) else W.config3(n, seed=0x5EED00B3)
    ref, st, _ = O.control_batch(P, b, threads=8)
    assert (st == 0).all()
    race = q.BalanceController.from_params(P).set_tuning(**FORMS[form])
    if strategies == 2:
        assert race.query_launch(n)["strategies"] == 1  # the 2-way race is built but not the default (measured neutral)
        race.set_tuning(race=2)
    elif start == "warm":
        assert race.query_launch(n, warm=True)["strategies"] == 1  # warm-started batches do not race by default (measured neutral)
        race.set_tuning(race=4)
    info = race.query_launch(n, warm=(start == "warm"))
    assert (info["form"], info["lanes_per_robot"], info["mode"], info["strategies"], info["chunk"]) == \
        (FORM_ID[form], 4, 2 if form == "uniform" else 1, strategies, 16 // strategies), info
    solo = q.BalanceController.from_params(P).set_tuning(race=0, **FORMS[form])
    assert solo.query_launch(n)["strategies"] == 1
    d = q.to_device(b)
    warm = None
    if start == "warm":
        prev = dict(b); prev["x"] = b["x"] + 1e-3
        warm = solo.control_batch(q.to_device(prev), want_active_set=True)["active_set"]
    o = race.control_batch(d, warm=warm, want_iterations=True, want_active_set=True)
    s = solo.control_batch(d, warm=warm, want_iterations=True)
    torch.cuda.synchronize()
    assert int((o["status"] != 0).sum()) == 0
    grf = o["grf_body"].cpu().numpy()
    assert _relerr(grf, ref) < RTOL
    assert_kkt(P, b, grf)
    it_r, it_s = o["iterations"].cpu().numpy(), s["iterations"].cpu().numpy()
    assert (it_r <= it_s).all() and it_r.min() >= 1
    if start == "cold" and strategies == 4:
        assert it_r.max() < it_s.max()  # the point of it: the slowest robot's chain is shorter
    # the winner's working set restarts in one recalculation, whichever strategy found it
    again = solo.control_batch(d, warm=o["active_set"], want_iterations=True)
    torch.cuda.synchronize()
    assert int(again["iterations"].max()) == 1 and _relerr(again["grf_body"].cpu().numpy(), ref) < RTOL
