"""Timings behind profiles/sensitivity_kinematics.md: qc_sensitivity_kin_batch alone - the torque half, the kinematics half, and both
in one call - on 4 096, 65 536 and 262 144 robots of config 3 with joint angles, and next to it, in the same process and under the same
protocol, qc_sensitivity_rot_batch (the two entrywise outputs) and the plant kernel.

  python tools/sensitivity_kinematics_bench.py                     # the three variants and the two siblings
  python tools/sensitivity_kinematics_bench.py --which both --launches 20 --no-siblings   # one variant: the run to put under a kernel trace

control_batch and sensitivity_batch against the parent commit: tools/sensitivity_rotation_bench.py --others --package-root DIR,
alternately on this tree and on a checkout of the parent.

Cold-cache protocol (tools/sensitivity_bench.py's): the launches rotate through `sets` distinct buffer sets of together at least
512 MiB - twice the 256 MiB last-level cache - so a set has left the cache when its turn comes again; every set is touched once
before timing.  One HIP event pair per launch, median / min / 90th percentile: that figure INCLUDES the launch itself.  Bytes are
the algorithm's, per robot:
  torque      joint_q, grf_body, joint_tau_bar, grf_bar_in 4 x 96 B, status 4 B, stance 4 B read; grf_bar and joint_q_bar 2 x 96 B written: 584 B
  kinematics  joint_q, feet_bar, joint_q_bar_in 3 x 96 B read; joint_q_bar 96 B written (in place): 384 B
  both        the six arrays 576 B, status and stance 8 B read; 192 B written: 776 B"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plant_bench import HBM_PEAK, PLANT_BYTES, world_feet  # noqa: E402
from sensitivity_rotation_bench import IN_BYTES as ROT_IN, OUT_BYTES as ROT_OUT, ROTATE_BYTES, timed_rotating  # noqa: E402

BYTES = {"torque": 4 * 96 + 8 + 2 * 96, "kinematics": 3 * 96 + 96, "both": 6 * 96 + 8 + 2 * 96}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    ap.add_argument("--which", choices=["torque", "kinematics", "both", "all"], default="all")
    ap.add_argument("--no-siblings", action="store_true")
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 262144])
    ap.add_argument("--launches", type=int, default=60)
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import torch

    import quadruped_control_amd as q
    from quadruped_control_amd import workloads

    assert torch.cuda.is_available(), "sensitivity_kinematics_bench needs the GPU: a timing taken elsewhere says nothing"
    ctl = q.BalanceController.from_params(q.cheetah_params(mu=0.6), device=0)
    ctl.set_kinematics(tau_min=-4.0, tau_max=12.0)  # limits that clamp some of the torques: both sides of the mask are taken
    names = ["torque", "kinematics", "both"] if args.which == "all" else [args.which]
    for n in args.sizes:
        sets = max(3, -(-ROTATE_BYTES // (n * BYTES["kinematics"])))  # sized by the smallest footprint timed
        host = workloads.config3(n=n)
        base = q.to_device(workloads.with_joint_angles(host))
        feet_base = q.to_device(host)
        pw = torch.from_numpy(world_feet(np, host)).cuda()
        plans = {name: [] for name in names + ([] if args.no_siblings else ["sensitivity_rotation entrywise", "plant_step"])}
        rnd = lambda *shape: torch.randn(shape, dtype=torch.float64, device="cuda")
        for k in range(sets):  # distinct memory per set; the states of set k are the base batch's (the time does not depend on them)
            dev = {key: v.clone() for key, v in base.items()}
            out = ctl.control_batch(dev, want_torques=True)
            tb, fb, gin, qin = rnd(n, 12), rnd(n, 12), rnd(n, 12), rnd(n, 12)
            kin = ctl.plan_sensitivity_kinematics
            if "torque" in plans:
                plans["torque"].append(kin(dev, out["grf_body"], out["status"], joint_tau_bar=tb, grf_bar_in=gin, want=("grf_bar", "joint_q_bar"))[0])
            if "kinematics" in plans:
                plans["kinematics"].append(kin(dev, feet_bar=fb, joint_q_bar_in=qin, want=("joint_q_bar",), out={"joint_q_bar": qin})[0])
            if "both" in plans:
                plans["both"].append(kin(dev, out["grf_body"], out["status"], joint_tau_bar=tb, feet_bar=fb, grf_bar_in=gin, joint_q_bar_in=rnd(n, 12),
                                         want=("grf_bar", "joint_q_bar"))[0])
            if not args.no_siblings:
                devf = {key: v.clone() for key, v in feet_base.items()}
                of = ctl.control_batch(devf)
                s = ctl.sensitivity_batch(devf, of["grf_body"], gin, want=("b_bar", "feet_bar"))
                plans["sensitivity_rotation entrywise"].append(ctl.plan_sensitivity_rotation(devf, of["grf_body"], gin, s["b_bar"], s["feet_bar"],
                                                                                             want=("Rwb_bar", "Rwb_d_bar"))[0])
                state = {key: devf[key] for key in ("Rwb", "x", "xdot", "w")}
                plans["plant_step"].append(ctl.plan_plant(state, of["grf_body"], pw.clone(), 1.0 / 300.0, devf["feet"]))
        torch.cuda.synchronize()
        for name, launches in plans.items():
            nbytes = BYTES.get(name) or (PLANT_BYTES if name == "plant_step" else ROT_IN + ROT_OUT["entrywise"])
            r = timed_rotating(torch, launches, args.launches)
            print(json.dumps(dict(what=name if name not in BYTES else "sensitivity_kinematics " + name, n=n, sets=sets, launches=args.launches, **r,
                                  bytes_per_robot=nbytes, fraction_of_hbm_peak_median=nbytes * n / (r["median_us"] * 1e-6) / HBM_PEAK,
                                  fraction_of_hbm_peak_min_time=nbytes * n / (r["min_us"] * 1e-6) / HBM_PEAK,
                                  timed="event pair per launch (includes the launch)", package_root=args.package_root)), flush=True)
        del plans
    ctl.close()


if __name__ == "__main__":
    main()
