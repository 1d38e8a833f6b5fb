"""CPU: the parameter cotangents' numpy restatement (tests/sensitivity_params_restatement.py) against its own 50-digit variant and
against central differences of the C oracle run with perturbed parameter sets, and the C ABI of qc_sensitivity_param_batch as far
as it goes without a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import quadruped_control_amd as q
from tests import device_math_reference as DMR
from tests import kkt_certificate_restatement as KR
from tests import sensitivity_params_restatement as PR
from tests import sensitivity_restatement as SR
from tests.fd_support import GROUPS, N_FD, _check_kept, _kept, fd_batch, pinned_cases

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EPS = 2.0 ** -52

# fd_support.GROUPS, per group: (the parameter set's changes, the relative step h, the least share of kept robots with a non-zero
# contribution or None).  h from a sweep on the oracle alone, h = 1e-2 ... 1e-7 of the parameters' own size (direction() scales d by them), the worst
# |FD(h) - FD(2h)| / (|row| |d|) over the kept robots:
#   gains   8e-12, 2e-11, 5e-10, 3e-9, 5e-8, 3e-7     linear in b: rounding only, growing as 1 / h           -> 1e-3 (kept 0.97)
#   mass    9e-10, 5e-9, 1e-7, 2e-6, 8e-6, 9e-5       linear                                                 -> 1e-2 (kept 0.85)
#   Ib      2e-9, 4e-8, 2e-7, 1e-6, 2e-5, 3e-4        linear                                                 -> 1e-2 (kept 0.97)
#   S       3e-4, 1e-4, 3e-3, 2e-2, 8e-2, 1           median 5e-6, 5e-8, 5e-10: h^2 until rounding wins      -> 1e-3
#   W diag  6e-5, 1e-6, 2e-5, 1e-3, 1e-2, 4e-2        (the worst robots: a reduced Hessian carried by W)     -> 1e-3
#   W       7e-5, 3e-6, 2e-6, 9e-5, 2e-3, 3e-2                                                               -> 1e-3
#   mu      median 5e-5, 6e-7, 6e-9, 7e-11, 8e-11, 1e-9   h^2 down to 1e-5                                   -> 1e-4
#   fzmin   5e-12, 2e-11, 7e-10, 9e-9, 4e-8, 1e-7     f0 is linear in the limit: rounding only               -> 1e-3
#   fzmax   3e-11, 3e-10, 2e-9, 8e-9, 4e-7, 2e-7                                                             -> 1e-3
# fzmin is raised to 25 N and fzmax lowered to 60 N for their own groups, so that feet actually sit on them.


def solve_fd_case(changes):
    """the oracle's solve of fd_batch() under cheetah_params(mu=0.6) with `changes`, its adjoint and the restatement's rows"""
    from oracle import c_oracle

    P = dict(q.cheetah_params(mu=0.6), **changes)
    b = fd_batch()
    gbar = np.random.default_rng(5).normal(0.0, 1.0, (N_FD, 12))
    F0, st0, _ = c_oracle.control_batch(P, b)
    s = SR.sensitivity(P, b, F0, gbar)
    pc = PR.param_cotangents(P, b, F0, gbar, s["adjoint"], active=s["active"])
    return dict(P=P, b=b, gbar=gbar, F0=F0, st0=st0, s=s, rows=pc["rows"])


_CASES = {}


@pytest.fixture(scope="module")
def fd_case(built):
    def get(changes):
        key = tuple(sorted(changes.items()))
        if key not in _CASES:
            _CASES[key] = solve_fd_case(changes)
        return _CASES[key]

    return get


def oracle_at(c, d, h):
    from oracle import c_oracle

    Pp = PR.unpack(PR.pack(c["P"]) + h * d, c["P"])
    F, st, _ = c_oracle.control_batch(Pp, c["b"])
    return F, st, KR.certificate(Pp, c["b"], F)["active"]


def quotient_check(c, d, h, F_at, rows, share):
    """<row, d> against the central difference quotient of F_at(k h), k = -2 ... 2, per robot; returns (keep, err, bar, scale).
    The bar is made of the oracle's own quotients alone: t = |FD(h) - FD(2h)| (three times the h^2 term of FD(h), plus the rounding
    of both) and N = |<grf_bar, F(-2h) - 4 F(-h) + 6 F(0) - 4 F(h) + F(2h)>| / 2h, the fourth difference, which a smooth F leaves at
    O(h^4) / h and the rounding of the five solves does not: bar = t + 3 N + 1e-8 |row| |d|, the last term the b-type test's."""
    pts = {k: F_at(k * h) for k in (-2, -1, 1, 2)}
    keep = _kept(c, pts.values())
    print("kept", keep.mean())
    _check_kept(c, keep)
    g = c["gbar"]
    fd1 = (g * (pts[1][0] - pts[-1][0])).sum(axis=1) / (2 * h)
    fd2 = (g * (pts[2][0] - pts[-2][0])).sum(axis=1) / (4 * h)
    d4 = (g * (pts[-2][0] - 4 * pts[-1][0] + 6 * c["F0"] - 4 * pts[1][0] + pts[2][0])).sum(axis=1) / (2 * h)
    an = rows @ d
    scale = np.linalg.norm(rows * (d != 0), axis=1) * np.linalg.norm(d)
    err, bar = np.abs(fd1 - an), np.abs(fd1 - fd2) + 3 * np.abs(d4) + 1e-8 * scale
    nz = scale[keep] > 0
    print("worst error / (|row| |d|)", float((err[keep][nz] / scale[keep][nz]).max()), "worst error / bar", float((err[keep] / np.maximum(bar[keep], 1e-300)).max()),
          "median bar / (|row| |d|)", float(np.median(bar[keep][nz] / scale[keep][nz])), "non-zero share", float((an[keep] != 0).mean()))
    if share is not None:
        assert (an[keep] != 0).mean() >= share, (an[keep] != 0).mean()  # (the check is not vacuous)
    else:
        assert nz.mean() > 0.9
    assert np.median(bar[keep][nz] / scale[keep][nz]) < 1e-5  # (the bar is tight: the oracle's own estimate is small)
    return keep, err, bar, scale


@pytest.mark.parametrize("group", list(GROUPS))
def test_parameter_cotangents_against_oracle_differences(fd_case, group):
    """<param_bar_row, d> against <grf_bar, (F(theta + h d) - F(theta - h d)) / 2h> of the C oracle run with the perturbed parameter
    sets, for one random direction d inside each parameter group (direction(): symmetric for Ib, S and W, a diagonal and a dense one
    for W), 480 robots, every non-empty contact pattern 32 times, the keep rule of fd_support (the working set the same at
    0, +-h, +-2h; share >= 0.75, all 15 patterns).  h per group: GROUPS above, from the sweep recorded there.  The bar is
    quotient_check's, made of the oracle's quotients alone.  Gains, mass, Ib and the limits are linear on the face (no truncation);
    S, W and mu have O(h^2).  Measured worst error / (|row| |d|) on the committed seeds: profiles/sensitivity_params.md."""
    changes, h, share = GROUPS[group]
    c = fd_case(changes)
    d = PR.direction(np.random.default_rng(11), group, c["P"])
    keep, err, bar, _ = quotient_check(c, d, h, lambda s: oracle_at(c, d, s), c["rows"], share)
    assert np.all(err[keep] <= bar[keep]), float((err[keep] / np.maximum(bar[keep], 1e-300)).max())


def test_restatement_against_50_digits():
    """The float64 rows against param_cotangents_mp on pinned_cases() of fd_support - a tied axis, a foot pinned at fzmax
    with a tied y, a foot at fzmin, an interior foot, a swing foot; uniform weights and a general S with a dense W; feet from joint_q -
    both fed the float64 adjoint.  Bar per entry: 64 eps terms - the longest chain is about 60 roundings (the 12-term row of W z
    behind the 6-term row of S behind the 8 additions of A z behind the lever arms, then rho, mu's sum over four feet), each at most
    eps / 2 of its entry in `terms`, which sums the magnitudes of all contributions."""
    rng = np.random.default_rng(3)
    for name, P, b, grf, codes in pinned_cases():
        gbar = rng.normal(0.0, 1.0, (1, 12))
        s = SR.sensitivity(P, b, grf, gbar, act_tol=1e-9)
        assert s["active"][0].tolist() == codes, (name, s["active"][0])
        pc = PR.param_cotangents(P, b, grf, gbar, s["adjoint"], act_tol=1e-9)
        assert (pc["active"] == s["active"]).all()
        ref = PR.param_cotangents_mp(P, b, grf, gbar, s["adjoint"], 0, s["active"][0], kin=(DMR.HIP.reshape(-1), DMR.LINKS.reshape(-1)) if "joint_q" in b else None)
        dist = PR.distance(pc["rows"][0], ref)
        bar = 64 * EPS * pc["terms"][0]
        print(name, "worst error / bar", float((dist / np.maximum(bar, 1e-300)).max()))
        assert np.all(dist <= bar), (name, np.argmax(dist / np.maximum(bar, 1e-300)))
        row = pc["rows"][0]
        assert row[PR.LAYOUT["mu"][0]][0] != 0 and row[PR.LAYOUT["fzmax"][0]][0] != 0  # foot 0 is tied, foot 1 sits at fzmax
        assert (row[PR.LAYOUT["fzmin"][0]][0] != 0) == (codes[3] != KR.SWING)             # foot 3 sits at fzmin unless it swings
        assert np.abs(pc["terms"][0]).min() >= 0 and np.all(np.abs(row) <= pc["terms"][0] * (1 + 8 * EPS))


def test_flagged_and_empty_faces():
    """All swing: zero rows.  All-zero forces (a failed robot): every stance foot flagged, the adjoint 0 - zero rows.  A NaN
    adjoint: a NaN row."""
    from quadruped_control_amd import workloads

    P = q.cheetah_params(mu=0.6)
    b = workloads.slice_batch(workloads.config3(n=8), 0, 3)
    gbar = np.ones((3, 12))
    for stance in (np.zeros((3, 4), np.uint8), np.ones((3, 4), np.uint8)):
        b["stance"] = stance
        s = SR.sensitivity(P, b, np.zeros((3, 12)), gbar)
        pc = PR.param_cotangents(P, b, np.zeros((3, 12)), gbar, s["adjoint"])
        assert not pc["rows"].any()
    pc = PR.param_cotangents(P, b, np.zeros((3, 12)), gbar, np.full((3, 12), np.nan))
    assert np.isnan(pc["rows"]).all()


# ------------------------------------------------------------------ the C ABI without a device
IO_FIELDS = ["struct_size", "grf_body", "grf_bar", "adjoint", "act_tol", "param_bar_rows", "param_bar"]


def test_sensitivity_param_symbols_are_exported(built):
    from quadruped_control_amd import _lib

    lib = ctypes.CDLL(os.path.join(ROOT, "quadruped_control_amd", "libqc_balance.so"))
    for name in ("qc_default_sensitivity_param", "qc_sensitivity_param_batch"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert _lib.load().qc_abi_version() == 6  # new entry points, no change to what existed


def test_sensitivity_param_mirror_matches_the_header(built, tmp_path):
    """sizeof and the member offsets of qc_sensitivity_param_io as the C compiler lays the header's struct out, against the ctypes
    mirror; QC_PARAM_COUNT against the mirror of qc_params and PARAM_LAYOUT; qc_default_sensitivity_param needs no device."""
    from quadruped_control_amd import _lib
    from quadruped_control_amd.balance_controller import PARAM_LAYOUT

    assert [f for f, _ in _lib.QcSensitivityParamIo._fields_] == IO_FIELDS
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qc_balance.h"\nint main(void) {\n  printf("%d %zu %zu", QC_PARAM_COUNT, offsetof(qc_params, max_iter), sizeof(qc_sensitivity_param_io));\n'
                   + "".join(f'  printf(" %zu", offsetof(qc_sensitivity_param_io, {f}));\n' for f in IO_FIELDS)
                   + "".join(f'  printf(" %zu", offsetof(qc_params, {f}));\n' for f in PARAM_LAYOUT) + '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert got[0] == _lib.PARAM_COUNT == 211 and got[1] == 8 * 211 == _lib.QcParams.max_iter.offset
    assert got[2] == ctypes.sizeof(_lib.QcSensitivityParamIo) == 56
    assert got[3:3 + len(IO_FIELDS)] == [getattr(_lib.QcSensitivityParamIo, f).offset for f in IO_FIELDS]
    assert got[3 + len(IO_FIELDS):] == [8 * sl.start for sl, _ in PARAM_LAYOUT.values()] == [getattr(_lib.QcParams, f).offset for f in PARAM_LAYOUT]
    assert list(PARAM_LAYOUT) == list(PR.LAYOUT) and all(PARAM_LAYOUT[k] == PR.LAYOUT[k] for k in PR.LAYOUT)
    io = _lib.QcSensitivityParamIo()
    io.grf_body, io.param_bar, io.act_tol, io.struct_size = 123, 456, -1.0, 7
    _lib.load().qc_default_sensitivity_param(ctypes.byref(io))
    assert io.struct_size == 56 and io.act_tol == 1e-7
    assert all(getattr(io, f) is None for f in IO_FIELDS if f not in ("struct_size", "act_tol"))


def test_unpack_param_bar_names_the_pieces():
    from quadruped_control_amd.balance_controller import unpack_param_bar

    P = q.cheetah_params(mu=0.6)
    got = unpack_param_bar(PR.pack(P))
    assert set(got) == set(PR.LAYOUT)
    for k in PR.LAYOUT:
        assert np.array_equal(np.asarray(got[k]), np.asarray(P[k], float)), k
    rows = unpack_param_bar(np.arange(2 * 211, dtype=float).reshape(2, 211))
    assert rows["W"].shape == (2, 12, 12) and rows["mu"].shape == (2,) and rows["W"][1, 0, 1] == 211 + 49 + 1
    with pytest.raises(ValueError):
        unpack_param_bar(np.zeros(210))


def test_sensitivity_param_argument_check_needs_no_device(built):
    """qc_sensitivity_param_batch refuses a bad call before it touches the device: the message is its own."""
    from quadruped_control_amd import _lib

    lib = _lib.load()
    io = _lib.QcSensitivityParamIo()
    lib.qc_default_sensitivity_param(ctypes.byref(io))
    bi = _lib.QcBatchIn()
    assert lib.qc_sensitivity_param_batch(None, 1, ctypes.byref(bi), ctypes.byref(io), None) == -1
    assert _lib.last_error() == "qc_sensitivity_param_batch: null argument"
    assert lib.qc_sensitivity_param_batch(None, 0, ctypes.byref(bi), None, None) == -1 and _lib.last_error() == "qc_sensitivity_param_batch: null argument"


def test_sensitivity_param_host_logic_without_a_device():
    """check_sensitivity_param_args through every refusal, the launch grid and the table of the record's factors (csrc/qc_host.hpp,
    csrc/qc_sensitivity_params.hpp), in a stand-alone program built with the address and undefined-behaviour sanitizers
    (tests/cpp/sensitivity_params_host_test.cpp)."""
    import __graft_entry__ as g

    assert "sensitivity_params_host_test" in g.HOST_TESTS
    exe = g.build_host_test("sensitivity_params_host_test")
    assert exe is not None and os.path.exists(exe)
    libs = subprocess.run(["ldd", exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "amdhip64" not in libs and "qc_balance" not in libs, libs
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "sensitivity params host logic ok" in r.stdout, r.stdout[-3000:]
