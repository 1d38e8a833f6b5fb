"""CPU: the numpy restatement of the forward mode in the handle's parameters (tests/param_tangent_restatement.py) against its own
50-digit variant, against the adjoint's restatement through the pairing identity and against central differences of the C oracle
between two parameter sets, and the C ABI of qc_param_tangent_batch as far as it goes without a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import quadruped_control_amd as q
from tests import device_math_reference as DMR
from tests import kkt_certificate_restatement as KR
from tests import param_tangent_restatement as PT
from tests import sensitivity_params_restatement as PR
from tests import sensitivity_restatement as SR
from tests.fd_support import N_FD, _kept, fd_batch
from tests.param_tangent_restatement import C_PAIR, C_PT, EPS, GROUPS
from tests.solved_batch_support import inputs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
N = 130
CODE3 = (15, 31, 47)  # robots of `placed` that get a code 3 foot: all four feet in stance, foot 0's force taken away

# Central differences of the oracle, per group: (the parameter set's changes - fd_support.GROUPS', so that feet sit on the limits -,
# the relative step h).  h is fd_support.GROUPS' - settled by the sweep on the oracle alone that tests/test_sensitivity_params_cpu.py
# records - lowered by a decade where fewer than 0.9 of fd_batch()'s 480 robots keep their working set at 0, +-h and +-2h: mass, 0.848
# at 1e-2.  The oracle's kept shares at the committed steps (profiles/param_tangent.md): gains 0.969, mass 0.985, Ib 0.973, S 0.985,
# W 1.000, mu 0.998, fzmin 0.990, fzmax 0.985.
FD_GROUPS = {"gains": ({}, 1e-3), "mass": ({}, 1e-3), "Ib": ({}, 1e-2), "S": ({}, 1e-3), "W": ({}, 1e-3), "mu": ({}, 1e-4),
             "fzmin": ({"fzmin": 25.0}, 1e-3), "fzmax": ({"fzmax": 60.0}, 1e-3)}


def directions(P, seed=70):
    """one direction per group of GROUPS, [8, 211] (sensitivity_params_restatement.direction: symmetric in Ib, S and W, relative)"""
    rng = np.random.default_rng(seed)
    return np.stack([PR.direction(rng, g, P) for g in GROUPS])


@pytest.fixture(scope="module")
def placed():
    """inputs(130, "feet") with a code 3 foot on CODE3's robots, the eight directions, the restatement's tangents, the adjoint's
    rows for one cotangent: computed once, never written"""
    P = q.cheetah_params(mu=0.6)
    b, grf = inputs(N, "feet")
    grf = grf.copy()
    for i in CODE3:
        grf[i, 0:3] = 0.0
    D = directions(P)
    gbar = np.random.default_rng(2).normal(0.0, 1.0, (N, 12))
    t = PT.param_tangent(P, b, grf, D)
    s = SR.sensitivity(P, b, grf, gbar)
    pc = PR.param_cotangents(P, b, grf, gbar, s["adjoint"], active=s["active"])
    return dict(P=P, b=b, grf=grf, D=D, gbar=gbar, t=t, s=s, pc=pc)


def test_restatement_against_50_digits():
    """The float64 restatement against param_tangent_mp on every eighth robot of the 130-robot placed-force batch, from `feet` and
    from joint_q, one direction per parameter group.  The distance of every entry of grf_tan and b_tan is measured in EPS x its
    condition sum; an entry whose condition sum is 0 is exact.  The worst per group is printed; the worst of all is the module's
    C_PT (rounded up), and the device's bar is 4 x it."""
    from tests.kkt_certificate_restatement import distance

    P = q.cheetah_params(mu=0.6)
    D = directions(P)
    worst = {}
    for source in ("feet", "joint_q"):
        b, grf = inputs(N, source)
        t = PT.param_tangent(P, b, grf, D)
        assert (t["flags"] == 0).all()
        kin = (DMR.HIP.reshape(-1), DMR.LINKS.reshape(-1)) if source == "joint_q" else None
        for i in range(0, N, 8):
            for k, group in enumerate(GROUPS):
                ref = PT.param_tangent_mp(P, b, grf, D, i, k, t["active"][i], kin=kin)
                for name, sums in (("grf_tan", "grf_sum"), ("b_tan", "b_sum")):
                    d, c = distance(t[name][k, i].reshape(-1), ref[name]), t[sums][k, i].reshape(-1)
                    assert np.all(d[c == 0] == 0), (source, i, group, name)
                    if (c > 0).any():
                        worst[source, group, name] = max(worst.get((source, group, name), 0.0), float((d[c > 0] / (EPS * c[c > 0])).max()))
    print("C_PT measured", worst)
    assert np.abs(t["grf_tan"]).max() > 0 and max(worst.values()) <= C_PT, worst


def _kinds(active, flags):
    """the four kinds of robot the pairing is taken on, as boolean masks [n]: a tied x or y with fz free, a z code 1, a z code 2 (each
    on a foot that moves, the robot without a code 3), a code 3 foot"""
    n = active.shape[0]
    kinds = {k: np.zeros(n, bool) for k in ("tied, fz free", "z code 1", "z code 2", "code 3")}
    for i in range(n):
        kinds["code 3"][i] = bool(flags[i] & 1)
        for code in active[i]:
            moves, sx, sy, cz = PT._foot_codes(code)
            if moves and not flags[i]:
                kinds["tied, fz free"][i] |= cz == 0 and (sx != 0 or sy != 0)
                kinds["z code 1"][i] |= cz == 1
                kinds["z code 2"][i] |= cz == 2
    return kinds


def test_pairing_identity_in_numpy(placed):
    """<grf_bar, grf_tan_k> = <param_bar_row, param_tan_k> per robot against sensitivity_params_restatement.param_cotangents, per
    group, and specifically on the robots with a tied x or y at a free fz, with a z code 1, with a z code 2 and with a code 3 foot -
    the batch holds all four.  The two sides share the face and the reduced matrix and nothing else: one differentiates the wrench
    law and the face forward, the other pulls the cotangent back.  The gap is measured in EPS x (the magnitudes of all terms on both
    sides) x the reduced condition number; the worst is the module's C_PAIR."""
    c = placed
    kinds = _kinds(c["t"]["active"], c["t"]["flags"])
    assert all(m.sum() >= 3 for m in kinds.values()), {k: int(m.sum()) for k, m in kinds.items()}
    assert np.array_equal(c["t"]["flags"], c["s"]["flags"]) and set(np.flatnonzero(kinds["code 3"])) == set(CODE3)
    worst = {}
    for k, group in enumerate(GROUPS):
        gap, lhs = PT.pairing_gap(c["gbar"], c["t"]["grf_tan"], c["pc"]["rows"], c["D"], k, c["t"]["cond"], c["pc"]["terms"])
        for kind, m in kinds.items():
            worst[group, kind] = float(gap[m].max())
        worst[group, "all"] = float(gap.max())
        moved = {"mu": kinds["tied, fz free"] | kinds["z code 1"] | kinds["z code 2"], "fzmin": kinds["z code 1"], "fzmax": kinds["z code 2"]}.get(group)
        if moved is not None:  # (not vacuous: the face's own parameters move the robots whose face depends on them)
            assert (np.abs(lhs[moved]) > 0).mean() > 0.9, group
        else:
            assert (np.abs(lhs) > 0).mean() > 0.8, group
    print("C_PAIR measured", max(worst.values()), worst)
    assert max(worst.values()) <= C_PAIR, worst


def test_flagged_and_empty_faces():
    """All swing: grf_tan 0 exactly, flags 0, b_tan = db all the same.  All-zero forces under four stance feet (a failed robot):
    grf_tan 0, bit 0."""
    from quadruped_control_amd import workloads

    P = q.cheetah_params(mu=0.6)
    b = workloads.slice_batch(workloads.config3(n=8), 0, 3)
    D = directions(P)
    b["stance"] = np.zeros((3, 4), np.uint8)
    t = PT.param_tangent(P, b, np.zeros((3, 12)), D)
    assert not t["flags"].any() and not t["grf_tan"].any() and np.abs(t["b_tan"][:3]).max() > 0
    b["stance"] = np.ones((3, 4), np.uint8)
    t = PT.param_tangent(P, b, np.zeros((3, 12)), D)
    assert (t["flags"] == 1).all() and not t["grf_tan"].any()


# ------------------------------------------------------------------ central differences of the oracle between two parameter sets
_CASES = {}


def _fd_case(changes):
    from oracle import c_oracle

    key = tuple(sorted(changes.items()))
    if key not in _CASES:
        P = dict(q.cheetah_params(mu=0.6), **changes)
        b = fd_batch()
        F0, st0, _ = c_oracle.control_batch(P, b)
        active = KR.certificate(P, b, F0)["active"]
        flags = np.array([1 if SR.face(a, P["mu"])[1] else 0 for a in active])
        _CASES[key] = dict(P=P, b=b, F0=F0, st0=st0, s=dict(active=active, flags=flags))
    return _CASES[key]


def oracle_quotients(c, d, h):
    """(keep, FD(h), FD(2h), the fourth difference / 2h) of the oracle's forces [n,12] between the parameter sets theta + k h d,
    k = -2 ... 2; keep: fd_support's rule - solved, no code 3, the working set the same at every point"""
    from oracle import c_oracle

    def at(s):
        Pp = PR.unpack(PR.pack(c["P"]) + s * d, c["P"])
        F, st, _ = c_oracle.control_batch(Pp, c["b"])
        return F, st, KR.certificate(Pp, c["b"], F)["active"]

    pts = {k: at(k * h) for k in (-2, -1, 1, 2)}
    keep = _kept(c, pts.values())
    fd1 = (pts[1][0] - pts[-1][0]) / (2 * h)
    fd2 = (pts[2][0] - pts[-2][0]) / (4 * h)
    d4 = (pts[-2][0] - 4 * pts[-1][0] + 6 * c["F0"] - 4 * pts[1][0] + pts[2][0]) / (2 * h)
    return keep, fd1, fd2, d4


@pytest.mark.parametrize("group", list(FD_GROUPS))
def test_tangent_against_oracle_differences(built, group):
    """grf_tan of the float64 restatement, entry by entry, against (F(theta + h d) - F(theta - h d)) / 2h of the C oracle run with
    the two parameter sets, one random direction inside each group, fd_batch()'s 480 robots.  Robots whose working set differs
    between the points are left out; the kept share must be at least 0.9 in every group (printed; profiles/param_tangent.md).  The
    bar per robot is made of the oracle's own quotients alone, as tests/test_sensitivity_params_cpu.py makes it: |FD(h) - FD(2h)|
    (three times FD(h)'s h^2 term, plus the rounding of both) + 3 x the fourth difference / 2h (which a smooth F leaves at O(h^4) / h
    and the rounding of the five solves does not), in the max norm over the 12 entries, + 1e-8 of the tangent's own size."""
    changes, h = FD_GROUPS[group]
    c = _fd_case(changes)
    d = PR.direction(np.random.default_rng(11), group, c["P"])
    t = PT.param_tangent(c["P"], c["b"], c["F0"], d[None])
    assert np.array_equal(t["flags"] & 1, c["s"]["flags"])
    keep, fd1, fd2, d4 = oracle_quotients(c, d, h)
    an = t["grf_tan"][0].reshape(N_FD, 12)
    err = np.abs(fd1 - an).max(axis=1)
    scale = np.abs(an).max(axis=1)
    bar = np.abs(fd1 - fd2).max(axis=1) + 3 * np.abs(d4).max(axis=1) + 1e-8 * scale
    nz = scale[keep] > 0
    print(group, "kept", float(keep.mean()), "worst error / bar", float((err[keep] / np.maximum(bar[keep], 1e-300)).max()), "worst error / |tangent|",
          float((err[keep][nz] / scale[keep][nz]).max()), "median bar / |tangent|", float(np.median(bar[keep][nz] / scale[keep][nz])), "moved", float(nz.mean()))
    assert keep.mean() >= 0.9, keep.mean()
    assert nz.mean() >= (0.3 if group in ("fzmin", "fzmax") else 0.9)                 # (not vacuous)
    assert np.median(bar[keep][nz] / scale[keep][nz]) < 1e-4                          # (the bar is tight)
    assert np.all(err[keep] <= bar[keep]), float((err[keep] / np.maximum(bar[keep], 1e-300)).max())


# ------------------------------------------------------------------ the C ABI without a device
IO_FIELDS = ["struct_size", "grf_body", "act_tol", "n_dir", "param_tan", "grf_tan_in", "b_tan_in", "grf_tan", "b_tan", "flags"]


def test_param_tangent_exists(built):
    """The two symbols are in the built library, the header declares them and says what is out of scope, the package exposes the
    functions - and none of it went into the pinned surfaces: _lib.EXPORTS, the ABI revision."""
    from quadruped_control_amd import _lib

    lib = ctypes.CDLL(os.path.join(ROOT, "quadruped_control_amd", "libqc_balance.so"))
    for name in ("qc_default_param_tangent", "qc_param_tangent_batch"):
        assert hasattr(lib, name) and name not in _lib.EXPORTS, name
    assert _lib.load().qc_abi_version() == 6
    T = q.tangent
    for fn in (T.param_tangent, T.plan_param_tangent, T.param_jacobian_batch):
        assert callable(fn) and fn.__doc__
    header = open(os.path.join(ROOT, "include", "qc_tangent.h")).read()
    assert "qc_default_param_tangent(" in header and "qc_param_tangent_batch(" in header
    block = header[header.index("/* qc_param_tangent_batch"):]
    for words in ("per-robot parameter directions", "tau_min / tau_max", "symmetrised dS / dW", "fusing this launch with qc_tangent_batch"):
        assert words in block[block.index("OUT OF SCOPE"):], words


def test_param_tangent_mirror_matches_the_header(built, tmp_path):
    """sizeof and the member offsets of qc_param_tangent_io as the C compiler lays the header's struct out, against the ctypes mirror;
    qc_default_param_tangent fills the io as documented and needs no device."""
    T = q.tangent
    T._library()
    fields = [f for f, _ in T.QcParamTangentIo._fields_]
    assert fields == IO_FIELDS
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qc_tangent.h"\nint main(void) {\n  printf("%zu", sizeof(qc_param_tangent_io));\n'
                   + "".join(f'  printf(" %zu", offsetof(qc_param_tangent_io, {f}));\n' for f in fields) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(T.QcParamTangentIo) == 80
    assert got[1:] == [getattr(T.QcParamTangentIo, f).offset for f in fields]
    io = T.QcParamTangentIo()
    io.grf_body, io.grf_tan, io.act_tol, io.struct_size, io.n_dir = 123, 456, -1.0, 7, 9
    T._library().qc_default_param_tangent(ctypes.byref(io))
    assert io.struct_size == 80 and io.act_tol == 1e-7 and io.n_dir == 1
    assert all(getattr(io, f) is None for f in fields if f not in ("struct_size", "act_tol", "n_dir"))


def test_param_tangent_argument_check_needs_no_device(built):
    """qc_param_tangent_batch refuses a bad call before it touches the device: the message is its own."""
    from quadruped_control_amd import _lib

    T = q.tangent
    lib = T._library()
    io = T.QcParamTangentIo()
    lib.qc_default_param_tangent(ctypes.byref(io))
    bi = _lib.QcBatchIn()
    assert lib.qc_param_tangent_batch(None, 1, ctypes.byref(bi), ctypes.byref(io), None) == -1
    assert _lib.last_error() == "qc_param_tangent_batch: null argument"
    assert lib.qc_param_tangent_batch(None, 0, ctypes.byref(bi), None, None) == -1 and _lib.last_error() == "qc_param_tangent_batch: null argument"


def test_param_jacobian_columns_and_seeds():
    """The columns of param_jacobian_batch(): the default leaves S and W out; a vector's and Ib's entries one by one; for S and W the
    upper triangle, and the seed of an off-diagonal column is the symmetric pair."""
    import torch

    T = q.tangent
    cols = T.param_jacobian_columns()
    assert [g for g, _ in cols].count("Ib") == 9 and len(cols) == 4 + 9 + 6 + 12 and not any(g in ("S", "W") for g, _ in cols)
    cols = T.param_jacobian_columns(("mu", "S", "W", "kff"))
    assert len(cols) == 1 + 21 + 78 + 6
    seeds = T.param_jacobian_seeds(cols, torch.device("cpu")).numpy()
    assert seeds.shape == (len(cols), 211)
    for c, (group, idx) in enumerate(cols):
        M = seeds[c][PR.LAYOUT[group][0]].reshape(PR.LAYOUT[group][1] or (1,))
        assert seeds[c].sum() == M.sum() == (2.0 if group in ("S", "W") and idx[0] != idx[1] else 1.0)
        if group in ("S", "W"):
            assert M[idx] == 1.0 and M[idx[::-1]] == 1.0 and np.array_equal(M, M.T)
    with pytest.raises(ValueError, match="unknown group"):
        T.param_jacobian_columns(("mu", "links"))


def test_param_tangent_host_logic_without_a_device():
    """check_param_tangent_args through every refusal and their order, param_tangent_constants, the launch grid past its cap and the
    layout of a row (csrc/qc_host.hpp, csrc/qc_param_tangent.hpp), in a stand-alone program built with the address and
    undefined-behaviour sanitizers (tests/cpp/param_tangent_host_test.cpp)."""
    import __graft_entry__ as g

    assert "param_tangent_host_test" in g.HOST_TESTS
    exe = g.build_host_test("param_tangent_host_test")
    assert exe is not None and os.path.exists(exe)
    libs = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "amdhip64" not in libs and "qc_balance" not in libs, libs
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "param tangent host logic ok" in r.stdout, r.stdout[-3000:]
