"""Timings behind profiles/support_polygon.md: qc_support_polygon_batch and qc_support_polygon_adjoint_batch alone on 4 096, 65 536
and 262 144 robots of a trot (feet in the body frame, the phase rule), with a shared and a per-robot schedule, in body and in world
mode - and next to them, in the same process and under the same protocol, the plant kernel (qc_plant_step_batch) for scale.

  python tools/support_polygon_bench.py
  python tools/support_polygon_bench.py --sizes 65536 --launches 20 --no-plant   # the run to put under a kernel trace

Cold-cache protocol (tools/swing_reference_bench.py's): the launches rotate through `sets` distinct buffer sets of together at least
512 MiB, every set is touched once before timing, one HIP event pair per launch - the figure INCLUDES the launch -, median / min / 90th
percentile.  Bytes are the algorithm's, per robot:
  forward  read feet 96, gait_phase 32, a per-robot schedule 128, in world mode Rwb 72 and x 24; written com_xy 16:   144 ... 368 B
  reverse  the forward's reads, com_xy_bar 16; written feet_bar 96, phase_bar 32, schedule_bar 128, in world mode Rwb_bar 72 and
           x_bar 24 (no accumulators):                                                                              400 ... 720 B"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plant_bench import HBM_PEAK, PLANT_BYTES, world_feet  # noqa: E402
from sensitivity_rotation_bench import ROTATE_BYTES, timed_rotating  # noqa: E402


def forward_bytes(world, shared):
    return 96 + 32 + (0 if shared else 128) + (96 if world else 0) + 16


def adjoint_bytes(world, shared):
    return forward_bytes(world, shared) + 96 + 32 + 128 + (96 if world else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    ap.add_argument("--no-plant", action="store_true")
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 262144])
    ap.add_argument("--launches", type=int, default=60)
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import torch

    import quadruped_control_amd as q
    from quadruped_control_amd import workloads

    assert torch.cuda.is_available(), "support_polygon_bench needs the GPU: a timing taken elsewhere says nothing"
    ctl = q.BalanceController.from_params(q.cheetah_params(mu=0.6), device=0)
    ctl.set_gait(0.3, 0.3)  # duty 0.5: a trot
    rnd = lambda *shape: torch.randn(shape, dtype=torch.float64, device="cuda")
    modes = [(world, shared) for world in (False, True) for shared in (True, False)]
    for n in args.sizes:
        sets = max(3, -(-ROTATE_BYTES // (n * forward_bytes(False, True))))  # sized by the smallest footprint timed
        host = workloads.config2(n=n)
        rng = np.random.default_rng(n)
        phase = np.mod(rng.uniform(0.0, 1.0, (n, 1)) + np.array([0.0, 0.5, 0.5, 0.0]), 1.0)
        base = {k: torch.from_numpy(np.ascontiguousarray(host[k])).cuda() for k in ("feet", "Rwb", "x")}
        base["gait_phase"] = torch.from_numpy(phase).cuda()
        widths = torch.from_numpy(rng.uniform(0.05, 0.5, (n, 4, 4))).cuda()
        plans = {}
        for k in range(sets):  # distinct memory per set
            dev = {key: v.clone() for key, v in base.items()}
            per_robot, one = widths.clone(), widths[0].clone()
            for world, shared in modes:
                b = dev if world else {key: dev[key] for key in ("feet", "gait_phase")}
                sched = one if shared else per_robot
                name = f"{'world' if world else 'body'} {'shared' if shared else 'per-robot'}"
                plans.setdefault("support_polygon " + name, []).append(ctl.plan_support_polygon(b, sched, world=world, out={"com_xy": rnd(n, 2)})[0])
                want = ("feet_bar", "phase_bar", "schedule_bar") + (("Rwb_bar", "x_bar") if world else ())
                out = {"feet_bar": rnd(n, 4, 3), "phase_bar": rnd(n, 4), "schedule_bar": rnd(n, 4, 4), "Rwb_bar": rnd(n, 9), "x_bar": rnd(n, 3)}
                plans.setdefault("support_polygon_adjoint " + name, []).append(
                    ctl.plan_support_polygon_adjoint(b, sched, rnd(n, 2), world=world, want=want, out={w: out[w] for w in want})[0])
            if not args.no_plant:
                full = q.to_device(host)
                grf = ctl.control_batch(full)["grf_body"] if k == 0 else grf.clone()
                state = {key: full[key] for key in ("Rwb", "x", "xdot", "w")}
                plans.setdefault("plant_step", []).append(ctl.plan_plant(state, grf, torch.from_numpy(world_feet(np, host)).cuda(), 1.0 / 300.0, full["feet"]))
        torch.cuda.synchronize()
        for name, launches in plans.items():
            world, shared = "world" in name, "shared" in name
            nbytes = PLANT_BYTES if name == "plant_step" else (adjoint_bytes if "adjoint" in name else forward_bytes)(world, shared)
            r = timed_rotating(torch, launches, args.launches)
            print(json.dumps(dict(what=name, n=n, sets=sets, launches=args.launches, **r, bytes_per_robot=nbytes,
                                  fraction_of_hbm_peak_median=nbytes * n / (r["median_us"] * 1e-6) / HBM_PEAK,
                                  fraction_of_hbm_peak_min_time=nbytes * n / (r["min_us"] * 1e-6) / HBM_PEAK,
                                  timed="event pair per launch (includes the launch)", package_root=args.package_root)), flush=True)
        del plans
    ctl.close()


if __name__ == "__main__":
    main()
