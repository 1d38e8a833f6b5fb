"""GPU: qc_tangent_batch (csrc/qc_tangent.hpp) against the numpy restatement (tests/tangent_restatement.py), against the shipped
adjoints through the dot-product identity, and its layout, Jacobian, poisoning and refusals.

Batch sizes 1, 63, 64, 65 and 130: tail lanes, one wave +- 1 (a workgroup is one wave), more than one workgroup.  Robot i of every
batch has contact pattern i % 16; the placed forces and the handles are solved_batch_support's.

Bars.  `flags` is compared exactly.  Every entry of grf_tan and b_tan is within 4 x C_TAN x EPS x its condition sum of the float64
restatement - C_TAN the restatement's own measured distance from its 50-digit variant in that unit (tests/tangent_restatement.py,
tests/test_tangent_cpu.py::test_restatement_against_50_digits), the condition sum the one tangent() returns with the value; an entry
whose condition sum is 0 is exact.  The dot product against the device's own adjoints is held to 4 x C_DOT of the CPU test's measure."""
import ctypes

import numpy as np
import pytest

from tests import solved_batch_support as SB
from tests import tangent_restatement as TR
from tests.gpu_arrays import assert_same_bits
from tests.solved_batch_support import EPS, FORMS, SENTINEL, STATE_KEYS, assert_raw_refusals, batch_in, ctls, inputs, params, q  # noqa: F401
from tests.tangent_restatement import C_DOT, C_TAN, dot_gap

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 130)
WANT_ALL = ("grf_tan", "b_tan", "flags")


def _dev(tans):
    import torch

    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in tans.items()}


def _run(q, ctl, b, grf, tans, want=WANT_ALL, **kw):
    import torch

    out = q.tangent.tangent_batch(ctl, q.to_device(b), torch.from_numpy(grf).cuda(), _dev(tans), want=want, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


_assert_close = SB.assert_tangent_close  # (the comparator lives with the shared helpers: tests/test_gpu_odd_law.py uses it too)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("source", ["feet", "joint_q", "duty"])
def test_against_the_restatement(q, ctls, n, source):
    """Placed forces; K = 1 and K = 3 with every tangent array given; all 16 contact masks once n >= 16; the all-swing mask gives
    exact zeros in grf_tan."""
    P = params(q, "uniform")
    b, grf = inputs(n, source)
    for K in (1, 3):
        tans = TR.random_tangents(n, K, 100 + n + K, joint_q=source != "feet")
        got = _run(q, ctls["uniform"], b, grf, tans)
        ref = TR.tangent(P, b, grf, tans)
        _assert_close(got, ref, (n, source, K))
        for i in range(0, n, 16):  # contact pattern 0: every foot swings
            assert got["flags"][i] == 0 and not got["grf_tan"][:, i].any()
        if n >= 16:
            assert np.abs(got["grf_tan"]).max() > 0 and (ref["flags"] == 0).all()


@pytest.fixture(scope="module")
def odd_ctl(q):
    c = SB.odd_handle(q)
    yield c
    c.close()


def test_joint_q_source_at_the_odd_model(q, odd_ctl):
    """joint_q with joint_q_tan on a handle at ODD_KIN, n = 65: the restatement takes ODD_KIN's kinematics and Jacobian; the default
    model on the same angles is far outside the bar."""
    from tests.device_math_reference import ODD_KIN

    P = params(q, "uniform")
    n = 65
    b, _, grf, _ = SB.odd_inputs(n)
    tans = TR.random_tangents(n, 1, 7, joint_q=True, names=("joint_q_tan",))
    got = _run(q, odd_ctl, b, grf, tans)
    ref = TR.tangent(P, b, grf, tans, kin=ODD_KIN)
    _assert_close(got, ref, (n, "joint_q at the odd model"))
    wrong = TR.tangent(P, b, grf, tans)
    assert np.abs(wrong["grf_tan"] - ref["grf_tan"]).max() > 1e-6 * np.abs(ref["grf_tan"]).max()


@pytest.mark.parametrize("kind", list(FORMS))
def test_dot_product_against_the_shipped_adjoints(q, ctls, kind):
    """130 robots solved by control_batch on each formulation: <grf_bar, grf_tan> against the pairing of the tangents with the outputs
    of sensitivity_batch and sensitivity_rotation_batch, per robot with flags == 0, within 4 x C_DOT of the CPU test's measure."""
    import torch
    from quadruped_control_amd import workloads
    from tests import sensitivity_restatement as SR

    ctl = q.BalanceController.from_params(params(q, kind), device=0)  # a handle of the test's own: race = 0 stays with it
    try:
        ctl.set_tuning(race=0)
        n, K = 130, 2
        b = dict(workloads.config3(n=n))
        b["stance"] = ((np.arange(n)[:, None] % 15 + 1 >> np.arange(4)[None, :]) & 1).astype(np.uint8)
        b = {k: np.ascontiguousarray(v) for k, v in b.items()}
        dev = q.to_device(b)
        o = ctl.control_batch(dev)
        torch.cuda.synchronize()
        assert int((o["status"] != 0).sum()) == 0
        gbar = SB.gbar(9000, n)
        gb = torch.from_numpy(gbar).cuda()
        s = ctl.sensitivity_batch(dev, o["grf_body"], gb, want=SR.OUTPUTS + ("flags",))
        r = ctl.sensitivity_rotation_batch(dev, o["grf_body"], gb, s["b_bar"], s["feet_bar"], want=("Rwb_rot_bar", "Rwb_d_rot_bar"))
        tans = TR.random_tangents(n, K, 11)
        t = q.tangent.tangent_batch(ctl, dev, o["grf_body"], _dev(tans), want=WANT_ALL)
        torch.cuda.synchronize()
        s, r, t = ({k: v.cpu().numpy() for k, v in d.items()} for d in (s, r, t))
        assert np.array_equal(t["flags"], s["flags"])
        ok = t["flags"] == 0
        assert ok.mean() > 0.9
        P = params(q, kind)
        grf = o["grf_body"].cpu().numpy()
        active = SR.sensitivity(P, b, grf, gbar)["active"]
        cond = np.array([SR.reduced_condition(P, b, active, i) for i in range(n)])
        for k in range(K):
            gap, lhs = dot_gap(gbar, t["grf_tan"], s, r, tans, k, cond)
            print(kind, k, "worst gap", float(gap[ok].max()), "of", 4 * C_DOT)
            assert (np.abs(lhs[ok]) > 0).mean() > 0.9 and gap[ok].max() <= 4 * C_DOT, (kind, k, float(gap[ok].max()))
    finally:
        ctl.close()


def test_layout_and_determinism(q, ctls):
    """Direction k of a K = 5 launch is bit-equal to a K = 1 launch with that direction; a NULL tangent array equals an array of
    zeros bit for bit; outputs beyond [K][n] keep the sentinel."""
    import torch

    ctl, n, K = ctls["dense"], 65, 5
    b, grf = inputs(n, "joint_q")
    dev, g = q.to_device(b), torch.from_numpy(grf).cuda()
    tans = _dev(TR.random_tangents(n, K, 21, joint_q=True))
    out = {"grf_tan": torch.full((K * n + 2, 4, 3), SENTINEL, dtype=torch.float64, device="cuda"),
           "b_tan": torch.full((K * n + 2, 6), SENTINEL, dtype=torch.float64, device="cuda")}
    views = {k: v[:K * n] for k, v in out.items()}
    big = q.tangent.tangent_batch(ctl, dev, g, tans, want=("grf_tan", "b_tan"), out=views)
    torch.cuda.synchronize()
    for v in out.values():
        assert bool((v[K * n:] == SENTINEL).all()) and not bool((v[:K * n] == SENTINEL).any())
    for k in range(K):
        one = q.tangent.tangent_batch(ctl, dev, g, {name: t[k].contiguous() for name, t in tans.items()}, want=("grf_tan", "b_tan"))
        for name in one:
            assert one[name].shape[0] == n  # the [n, ...] form comes back squeezed
            assert_same_bits(big[name][k], one[name], f"{name}, direction {k}")
    some = {k: v for k, v in tans.items() if k in ("x_tan", "Rwb_rot_tan", "joint_q_tan")}
    zeros = {k: (v if k in some else torch.zeros_like(v)) for k, v in tans.items()}
    a = q.tangent.tangent_batch(ctl, dev, g, some, want=("grf_tan", "b_tan"))
    z = q.tangent.tangent_batch(ctl, dev, g, zeros, want=("grf_tan", "b_tan"))
    for name in a:
        assert_same_bits(a[name].reshape(K * n, -1), z[name].reshape(K * n, -1), f"{name}: NULL against zeros")


def test_jacobian_columns_are_unit_seed_tangents(q, ctls):
    import torch

    ctl, n = ctls["uniform"], 65
    b, grf = inputs(n, "joint_q")
    dev, g = q.to_device(b), torch.from_numpy(grf).cuda()
    wrt = q.tangent.JACOBIAN_WRT + ("feet", "joint_q")
    full = q.tangent.jacobian_batch(ctl, dev, g, wrt=wrt)
    assert full["jac"].shape == (n, 12, 48) and len(full["columns"]) == 48 and full["columns"][0] == ("x", 0) and full["columns"][-1] == ("joint_q", 11)
    chunked = q.tangent.jacobian_batch(ctl, dev, g, wrt=wrt, chunk=7)
    assert_same_bits(chunked["jac"], full["jac"], "chunk = 7 against unchunked")
    assert torch.equal(chunked["flags"], full["flags"])
    for c in (0, 5, 20, 23, 30, 47):
        name, comp = full["columns"][c]
        seed = torch.zeros((n, q.tangent.TANGENTS[name + "_tan"]), dtype=torch.float64, device="cuda")
        seed[:, comp] = 1.0
        one = q.tangent.tangent_batch(ctl, dev, g, {name + "_tan": seed})["grf_tan"]
        assert_same_bits(full["jac"][:, :, c].contiguous(), one.reshape(n, 12), f"column {c} = {name}[{comp}]")
    assert float(full["jac"].abs().max()) > 0


@pytest.mark.parametrize("source", ["feet", "joint_q"])
def test_second_round_of_the_grid_stride(q, ctls, source):
    """gpu_arrays.second_round at n = 4096 x 64 + 65 = 262 209 robots, K = 2, period 130: the grid is capped, workgroup 0 walks a full
    second round and workgroup 1 has one live lane in its second.  The period holds a poisoned robot (a NaN foot: bit 1, NaN in both
    directions) and a failed one (all-zero forces: bit 0).  The large launch equals the n = 130 launch tiled, bit for bit in both
    directions, and its two out-of-period robots equal an n = 2 launch of them."""
    import torch
    from tests.gpu_arrays import SECOND_ROUND_N, sentinel_tensor, second_round

    p, K, ctl = 130, 2, ctls["uniform"]
    b, grf = inputs(p, source)
    b, grf = {k: v.copy() for k, v in b.items()}, grf.copy()
    b["feet" if source == "feet" else "joint_q"][15, 4] = np.nan
    grf[31] = 0.0
    tans = TR.random_tangents(p, K, 31, joint_q=source != "feet")
    b2, grf2 = inputs(140, source)
    tans2 = TR.random_tangents(140, K, 32, joint_q=source != "feet")
    pick = [135, 136]  # contact patterns 7 and 8, robots of another draw

    def rows_of(bb, gg, tt, sel):
        rows = {k: torch.from_numpy(np.ascontiguousarray(v[sel])).cuda() for k, v in bb.items()}
        rows["grf_body"] = torch.from_numpy(np.ascontiguousarray(gg[sel])).cuda()
        for name, t in tt.items():
            for k in range(K):
                rows[f"{name}#{k}"] = torch.from_numpy(np.ascontiguousarray(t[k][sel])).cuda()
        return rows

    def launch(rows, m, over=False):
        batch = {k: v for k, v in rows.items() if k != "grf_body" and "#" not in k}
        tt = {name: torch.stack([rows[f"{name}#{k}"] for k in range(K)]).contiguous() for name in tans}
        out = {"grf_tan": sentinel_tensor((K * m, 4, 3), torch.float64), "b_tan": sentinel_tensor((K * m, 6), torch.float64),
               "flags": sentinel_tensor((m,), torch.int32)}
        res = q.tangent.tangent_batch(ctl, batch, rows["grf_body"], tt, want=WANT_ALL, out=out)
        torch.cuda.synchronize()
        got = {"flags": res["flags"]}
        for k in range(K):
            got[f"grf_tan{k}"], got[f"b_tan{k}"] = res["grf_tan"][k], res["b_tan"][k]
        return got

    small = second_round(launch, rows_of(b, grf, tans, slice(None)), rows_of(b2, grf2, tans2, pick), n=SECOND_ROUND_N)
    flags = small["flags"].cpu().numpy()
    assert flags[15] == 2 and all(bool(torch.isnan(small[f"{name}{k}"][15]).all()) for name in ("grf_tan", "b_tan") for k in range(K))
    assert flags[31] & 1 and np.flatnonzero(flags).tolist() == [15, 31] and not any(bool(small[f"grf_tan{k}"][31].any()) for k in range(K))
    assert not bool(torch.isnan(small["grf_tan0"][14]).any()) and not bool(torch.isnan(small["grf_tan0"][16]).any())
    torch.cuda.empty_cache()


@pytest.mark.parametrize("law", ["cheetah", "odd"])
def test_finite_differences_of_control_batch(q, ctls, law):
    """<grf_bar, grf_tan> against control_batch itself at theta +- h d, for three random directions in the b-type inputs (exactly
    linear on a fixed face): the batch (128 robots of config 3, the 15 contact patterns in turn, race = 0), the keep rule (solved and
    the same want_active_set word at -h, 0, +h, flags 0), the step h = 1e-3 and the bar 1e-6 |theta_bar| |d| of
    tests/test_gpu_sensitivity.py's finite-difference test - with |theta_bar| the norm of sensitivity_batch's cotangents for the same
    grf_bar, the scale that bar is stated in.  Kept share >= 0.75.  law = "odd": the same h, bar and keep rule on a handle at
    solved_batch_support.odd_law with odd_states of the batch; there the kept share must be at least one half, and is printed."""
    import torch
    from quadruped_control_amd import workloads

    ctl = q.BalanceController.from_params(params(q, "uniform") if law == "cheetah" else SB.odd_law(), device=0)  # a handle of the test's own: race = 0 stays with it
    try:
        ctl.set_tuning(race=0)
        n, h = 128, 1e-3
        b = dict(workloads.config3(n=n))
        b["stance"] = ((np.arange(n)[:, None] % 15 + 1 >> np.arange(4)[None, :]) & 1).astype(np.uint8)
        if law == "odd":
            b = SB.odd_states({k: np.ascontiguousarray(v) for k, v in b.items()}, 5)
        keys = ("x", "xdot", "w", "x_d", "xdot_d", "w_d")
        gbar = SB.gbar(9100, n)
        for trial in range(3):
            rng = np.random.default_rng(90 + trial)
            d = {k: rng.normal(0.0, 1.0, (n, 3)) for k in keys}

            def solve(step):
                bb = {k: np.ascontiguousarray(v + step * d[k] if k in d else v) for k, v in b.items()}
                dev = q.to_device(bb)
                o = ctl.control_batch(dev, want_active_set=True)
                torch.cuda.synchronize()
                return dev, o

            dev0, o0 = solve(0.0)
            (_, op), (_, om) = solve(h), solve(-h)
            t = q.tangent.tangent_batch(ctl, dev0, o0["grf_body"], {k + "_tan": torch.from_numpy(v).cuda() for k, v in d.items()}, want=("grf_tan", "flags"))
            s = ctl.sensitivity_batch(dev0, o0["grf_body"], torch.from_numpy(gbar).cuda(), want=tuple(k + "_bar" for k in keys))
            torch.cuda.synchronize()
            flags = t["flags"].cpu().numpy()
            s = {k: v.cpu().numpy() for k, v in s.items()}
            st = [o["status"].cpu().numpy() for o in (o0, op, om)]
            ws = [o["active_set"].cpu().numpy() for o in (o0, op, om)]
            keep = (st[0] == 0) & (st[1] == 0) & (st[2] == 0) & (ws[0] == ws[1]) & (ws[0] == ws[2]) & (flags == 0)
            assert keep.mean() >= (0.75 if law == "cheetah" else 0.5), keep.mean()
            fd = (gbar * (op["grf_body"].cpu().numpy() - om["grf_body"].cpu().numpy())).sum(axis=1) / (2 * h)
            an = (gbar * t["grf_tan"].cpu().numpy().reshape(n, 12)).sum(axis=1)
            scale = np.sqrt(sum((s[k + "_bar"] ** 2).sum(axis=1) for k in keys)) * np.sqrt(sum((d[k] ** 2).sum(axis=1) for k in keys))
            err = np.abs(fd - an)
            print(law, "direction", trial, "kept", keep.mean(), "worst relative error", float((err[keep] / np.maximum(scale[keep], 1e-300)).max()))
            assert (scale[keep] > 0).mean() > (0.9 if law == "cheetah" else 0.75)  # (odd states keep more robots whose face is pinned throughout: 0.84 ... 0.85 measured)
            assert np.all(err[keep] <= 1e-6 * scale[keep])
    finally:
        ctl.close()


def test_indefinite_reduced_system_sets_bit_1(q):
    """A handle whose W (symmetric, positive diagonal, as qc_create asks) is indefinite between the x coordinates of feet 0 and 1:
    on a face where both are free the reduced system has a negative pivot - bit 1, NaN in all K directions; a robot whose face
    pins one of the two is untouched and matches the restatement."""
    P = dict(params(q, "uniform"))
    W = np.asarray(P["W"], float).copy()
    W[0, 3] = W[3, 0] = -50.0  # far beyond what 2 A^T S A adds between two fx
    P["W"] = W
    ctl = q.BalanceController.from_params(P, device=0)
    try:
        n, K = 65, 3
        b, grf = inputs(n, "feet")
        tans = TR.random_tangents(n, K, 41)
        got = _run(q, ctl, b, grf, tans)
        ref = TR.tangent(P, b, grf, tans)
        assert np.array_equal(got["flags"], ref["flags"])
        bad = np.flatnonzero(got["flags"] & 2)
        good = np.setdiff1d(np.arange(n), bad)
        assert 0 < len(bad) < n and len(good) > 16
        assert np.isnan(got["grf_tan"][:, bad]).all() and np.isnan(got["b_tan"][:, bad]).all()
        assert not np.isnan(got["grf_tan"][:, good]).any()
        _assert_close(got, ref, "indefinite W", rows=good)
    finally:
        ctl.close()


def test_refusals_raise_and_launch_nothing(q, ctls):
    """Each refusal of qc_tangent_batch raises ValueError with the library's message and launches nothing: the output keeps its
    sentinel."""
    import torch
    from quadruped_control_amd import _lib

    ctl, n = ctls["uniform"], 65
    b, grf = inputs(n, "feet")
    dev, g = q.to_device(b), torch.from_numpy(grf).cuda()
    x_tan = torch.ones((n, 3), dtype=torch.float64, device="cuda")
    out = {"grf_tan": torch.full((n, 4, 3), SENTINEL, dtype=torch.float64, device="cuda")}

    def refused(words, batch=dev, grf_body=g, tangents=None, **kw):
        with pytest.raises(ValueError, match=r"^qc_tangent_batch: " + words):
            q.tangent.tangent_batch(ctl, batch, grf_body, {"x_tan": x_tan} if tangents is None else tangents, want=kw.pop("want", ("grf_tan",)),
                                    out=kw.pop("out", out), **kw)
        torch.cuda.synchronize()
        assert bool((out["grf_tan"] == SENTINEL).all()), words

    refused("grf_body is required", grf_body=None)
    for k in STATE_KEYS:
        refused("the state arrays", batch={a: v for a, v in dev.items() if a != k})
    refused("feet or joint_q is required", batch={a: v for a, v in dev.items() if a != "feet"})
    for bad in (-1e-9, float("nan"), float("inf")):
        refused("act_tol must be finite", act_tol=bad)
    refused("no output requested", want=("flags",), out=None)
    refused("no tangent given", tangents={})
    refused("joint_q_tan needs joint_q", tangents={"joint_q_tan": torch.ones((n, 12), dtype=torch.float64, device="cuda")})
    lib = q.tangent._library()
    io = q.tangent.QcTangentIo()
    lib.qc_default_tangent(ctypes.byref(io))
    io.grf_body, io.x_tan, io.grf_tan = g.data_ptr(), x_tan.data_ptr(), out["grf_tan"].data_ptr()
    bi = batch_in(dev, STATE_KEYS + ("feet", "stance"))
    io.n_dir = 0
    assert lib.qc_tangent_batch(ctl._h, n, ctypes.byref(bi), ctypes.byref(io), None) == -1 and _lib.last_error() == "qc_tangent_batch: n_dir must be >= 1"
    io.n_dir = 1
    assert_raw_refusals(lib.qc_tangent_batch, lambda: (ctl._h, n, bi, io), "qc_tangent_io", 136, 128, [(out["grf_tan"], SENTINEL, True)])
