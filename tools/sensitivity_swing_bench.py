"""Timings behind profiles/sensitivity_swing.md: qc_sensitivity_swing_batch alone on 4 096, 65 536 and 262 144 robots of config 3 with
joint angles and swing references inside reach, on a trot mask (the two diagonals in turn) and with all four legs swinging, and next
to it, in the same process and under the same protocol, qc_sensitivity_kin_batch (both halves) and the forward tick with swing
references (control_batch(want_torques=True)).

  python tools/sensitivity_swing_bench.py                                  # both masks and the two siblings
  python tools/sensitivity_swing_bench.py --which trot --launches 20 --no-siblings   # one case: the run to put under a kernel trace

Cold-cache protocol (tools/sensitivity_bench.py's): the launches rotate through `sets` distinct buffer sets of together at least
512 MiB - twice the 256 MiB last-level cache - so a set has left the cache when its turn comes again; every set is touched once
before timing (more than 25 ms of launches).  One HIP event pair per launch, median / min / 90th percentile: that figure INCLUDES
the launch itself.  Bytes are the algorithm's, per robot, for the call tick_autograd() makes (every output but gain_bar, the three
accumulators in place):
  read     Rwb 72, x 24, joint_q, joint_qdot, swing_pos, swing_vel, joint_tau_bar 5 x 96, stance 4, joint_q_bar_in 96, Rwb_bar_in 72,
           x_bar_in 24: 772 B
  written  swing_pos_bar, swing_vel_bar, joint_q_bar, joint_qdot_bar 4 x 96, Rwb_bar 72, x_bar 24: 480 B                      1252 B
The forward tick is given without a byte count: it is a solve, not a stream."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plant_bench import HBM_PEAK  # noqa: E402
from sensitivity_kinematics_bench import BYTES as KIN_BYTES  # noqa: E402
from sensitivity_rotation_bench import ROTATE_BYTES, timed_rotating  # noqa: E402

BYTES = 72 + 24 + 5 * 96 + 4 + 96 + 72 + 24 + 4 * 96 + 72 + 24


def swing_references(q, host):
    """swing_pos [n,12] that the tick reads back 0.02 m above every foot (p_b = Rwb^T pos - x, sic), from the default kinematics' FK"""
    from quadruped_control_amd import _lib

    k = _lib.QcKinematics()
    _lib.load().qc_default_kinematics(ctypes.byref(k))
    hip, links = np.array(k.hip[:]).reshape(4, 3), np.array(k.links[:]).reshape(4, 3)
    n = host["x"].shape[0]
    jq = host["joint_q"].reshape(n, 4, 3)
    s1, c1, s2, c2 = np.sin(jq[..., 0]), np.cos(jq[..., 0]), np.sin(jq[..., 1]), np.cos(jq[..., 1])
    s23, c23 = np.sin(jq[..., 1] + jq[..., 2]), np.cos(jq[..., 1] + jq[..., 2])
    l1, l2, l3 = links[:, 0], links[:, 1], links[:, 2]
    p = np.stack([l2 * s2 + l3 * s23, l1 * c1 - l2 * s1 * c2 - l3 * s1 * c23, l1 * s1 + l2 * c1 * c2 + l3 * c1 * c23], axis=-1) + hip
    p[..., 2] += 0.02
    R = host["Rwb"].reshape(n, 3, 3)
    return np.ascontiguousarray(np.einsum("nij,nlj->nli", R, p + host["x"][:, None, :]).reshape(n, 12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    ap.add_argument("--which", choices=["trot", "all-swing", "all"], default="all")
    ap.add_argument("--no-siblings", action="store_true")
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 262144])
    ap.add_argument("--launches", type=int, default=60)
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import torch

    import quadruped_control_amd as q
    from quadruped_control_amd import workloads

    assert torch.cuda.is_available(), "sensitivity_swing_bench needs the GPU: a timing taken elsewhere says nothing"
    ctl = q.BalanceController.from_params(q.cheetah_params(mu=0.6), device=0)
    masks = ["trot", "all-swing"] if args.which == "all" else [args.which]
    for n in args.sizes:
        sets = max(3, -(-ROTATE_BYTES // (n * KIN_BYTES["both"])))  # sized by the smallest footprint timed
        host = workloads.with_joint_angles(workloads.config3(n=n))
        host.pop("feet", None)
        host["swing_pos"], host["swing_vel"] = swing_references(q, host), np.zeros((n, 12))
        host["joint_qdot"] = np.zeros((n, 12))
        stance = {"trot": np.where((np.arange(n) % 2 == 0)[:, None], [1, 0, 0, 1], [0, 1, 1, 0]).astype(np.uint8), "all-swing": np.zeros((n, 4), np.uint8)}
        base = q.to_device(host)
        plans = {}
        rnd = lambda *shape: torch.randn(shape, dtype=torch.float64, device="cuda")
        for k in range(sets):  # distinct memory per set; the states of set k are the base batch's (the time does not depend on them)
            for m in masks:
                dev = dict({key: v.clone() for key, v in base.items()}, stance=torch.from_numpy(stance[m]).cuda())
                tb, qin, rin, xin = rnd(n, 12), rnd(n, 4, 3), rnd(n, 9), rnd(n, 3)
                out = {"swing_pos_bar": rnd(n, 4, 3), "swing_vel_bar": rnd(n, 4, 3), "joint_q_bar": qin, "joint_qdot_bar": rnd(n, 4, 3), "Rwb_bar": rin, "x_bar": xin}
                plans.setdefault("sensitivity_swing " + m, []).append(
                    ctl.plan_sensitivity_swing(dev, tb, out=out, joint_q_bar_in=qin, Rwb_bar_in=rin, x_bar_in=xin)[0])
                if not args.no_siblings:
                    launch, res = ctl.plan_batch(dev, want_torques=True)
                    launch()
                    plans.setdefault("control_batch with swing references " + m, []).append(launch)
                    if m == masks[0]:
                        plans.setdefault("sensitivity_kinematics both", []).append(ctl.plan_sensitivity_kinematics(
                            dev, res["grf_body"], res["status"], joint_tau_bar=tb, feet_bar=rnd(n, 12), grf_bar_in=rnd(n, 12), joint_q_bar_in=rnd(n, 12),
                            want=("grf_bar", "joint_q_bar"))[0])
        torch.cuda.synchronize()
        for name, launches in plans.items():
            nbytes = BYTES if name.startswith("sensitivity_swing") else (KIN_BYTES["both"] if name.startswith("sensitivity_kin") else None)
            r = timed_rotating(torch, launches, args.launches)
            rate = {} if nbytes is None else dict(bytes_per_robot=nbytes, fraction_of_hbm_peak_median=nbytes * n / (r["median_us"] * 1e-6) / HBM_PEAK,
                                                  fraction_of_hbm_peak_min_time=nbytes * n / (r["min_us"] * 1e-6) / HBM_PEAK)
            print(json.dumps(dict(what=name, n=n, sets=sets, launches=args.launches, **r, **rate, timed="event pair per launch (includes the launch)",
                                  package_root=args.package_root)), flush=True)
        del plans
    ctl.close()


if __name__ == "__main__":
    main()
