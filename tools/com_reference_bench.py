"""Timings behind profiles/com_reference.md: qc_com_reference_batch (both modes) and qc_com_reference_adjoint_batch (rows only, the sum
only, both) alone on 4 096, 65 536 and 262 144 robots of a trot (feet, world frame, a shared schedule, the phase rule) - and next to
them, in the same process and under the same protocol, the pieces they replace - support_polygon_batch(world=True) + torch.cat into
x_d, support_polygon_adjoint_batch's schedule_bar rows + torch.sum(dim=0) - and the plant kernel (qc_plant_step_batch) for scale.

  python tools/com_reference_bench.py
  python tools/com_reference_bench.py --sizes 65536 --launches 20 --no-plant   # the run to put under a kernel trace

Cold-cache protocol (tools/support_polygon_bench.py's): the launches rotate through `sets` distinct buffer sets of together at least
512 MiB, every set is touched once before timing, one HIP event pair per launch - the figure INCLUDES the launch (for a replaced
piece: both of its launches) -, median / min / 90th percentile.  Bytes are the algorithm's, per robot, with a shared schedule:
  forward  read feet 96, gait_phase 32, Rwb 72, x 24, x_d 24; written x_d 24:                                              272 B
  reverse  the forward's reads without x_d, x_d_bar 24; written x_d_in_bar 24, feet_bar 96, phase_bar 32 and - rows - schedule_bar
           128 (no accumulators); the sum adds 16 numbers per 64 robots:                                          400 (sum only) / 528 B"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plant_bench import HBM_PEAK, PLANT_BYTES, world_feet  # noqa: E402
from sensitivity_rotation_bench import ROTATE_BYTES, timed_rotating  # noqa: E402

FORWARD_BYTES = 96 + 32 + 96 + 24 + 24
ADJOINT_BYTES = {"rows": 96 + 32 + 96 + 24 + 24 + 96 + 32 + 128, "sum": 96 + 32 + 96 + 24 + 24 + 96 + 32, "rows+sum": 96 + 32 + 96 + 24 + 24 + 96 + 32 + 128}
POLYGON_CAT_BYTES = (96 + 32 + 96 + 16) + (16 + 24 + 24)       # the polygon, then cat reads com_xy and x_d and writes a new x_d
POLYGON_SUM_BYTES = (96 + 32 + 96 + 16 + 96 + 32 + 128) + 128  # the polygon's reverse pass with its rows, then torch reads the rows


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

    assert torch.cuda.is_available(), "com_reference_bench needs the GPU: a timing taken elsewhere says nothing"
    ctl = q.BalanceController.from_params(q.cheetah_params(mu=0.6), device=0)
    ctl.set_gait(0.3, 0.3)  # duty 0.5: a trot
    rnd = lambda *shape: torch.randn(shape, dtype=torch.float64, device="cuda")
    for n in args.sizes:
        sets = max(3, -(-ROTATE_BYTES // (n * FORWARD_BYTES)))
        host = workloads.config2(n=n)
        rng = np.random.default_rng(n)
        phase = np.mod(rng.uniform(0.0, 1.0, (n, 1)) + np.array([0.0, 0.5, 0.5, 0.0]), 1.0)
        base = {k: torch.from_numpy(np.ascontiguousarray(host[k])).cuda() for k in ("feet", "Rwb", "x")}
        base["gait_phase"] = torch.from_numpy(phase).cuda()
        shared = torch.from_numpy(rng.uniform(0.05, 0.5, (4, 4))).cuda()
        plans, nbytes = {}, {}

        def add(name, launch, size):
            plans.setdefault(name, []).append(launch)
            nbytes[name] = size

        for k in range(sets):  # distinct memory per set
            dev = {key: v.clone() for key, v in base.items()}
            sched, x_d, bar = shared.clone(), rnd(n, 3), rnd(n, 3)
            for mode in ("replace", "offset"):
                add("com_reference " + mode, ctl.plan_com_reference(dev, sched, x_d, mode, 0.7, out={"x_d": rnd(n, 3)})[0], FORWARD_BYTES)
            out = {"x_d_in_bar": rnd(n, 3), "feet_bar": rnd(n, 4, 3), "phase_bar": rnd(n, 4), "schedule_bar": rnd(n, 4, 4), "schedule_bar_sum": rnd(4, 4)}
            for what, extra in (("rows", ("schedule_bar",)), ("sum", ("schedule_bar_sum",)), ("rows+sum", ("schedule_bar", "schedule_bar_sum"))):
                want = ("x_d_in_bar", "feet_bar", "phase_bar") + extra
                add("com_reference_adjoint " + what, ctl.plan_com_reference_adjoint(dev, sched, bar, "replace", 1.0, want=want, out={w: out[w] for w in want})[0],
                    ADJOINT_BYTES[what])
            # the pieces replaced
            poly, pres = ctl.plan_support_polygon(dev, sched, world=True, out={"com_xy": rnd(n, 2)})

            def polygon_cat(poly=poly, com=pres["com_xy"], x_d=x_d):
                poly()
                return torch.cat([com, x_d[:, 2:]], 1)

            add("support_polygon + torch.cat", polygon_cat, POLYGON_CAT_BYTES)
            want = ("feet_bar", "phase_bar", "schedule_bar")
            adj, ares = ctl.plan_support_polygon_adjoint(dev, sched, rnd(n, 2), world=True, want=want, out={w: out[w] for w in want})

            def polygon_sum(adj=adj, rows=ares["schedule_bar"]):
                adj()
                return rows.sum(dim=0)

            add("support_polygon_adjoint rows + torch.sum", polygon_sum, POLYGON_SUM_BYTES)
            if not args.no_plant:
                full = q.to_device(host)
                grf = ctl.control_batch(full)["grf_body"] if k == 0 else grf.clone()
                state = {key: full[key] for key in ("Rwb", "x", "xdot", "w")}
                add("plant_step", ctl.plan_plant(state, grf, torch.from_numpy(world_feet(np, host)).cuda(), 1.0 / 300.0, full["feet"]), PLANT_BYTES)
        torch.cuda.synchronize()
        for name, launches in plans.items():
            r = timed_rotating(torch, launches, args.launches)
            print(json.dumps(dict(what=name, n=n, sets=sets, launches=args.launches, **r, bytes_per_robot=nbytes[name],
                                  fraction_of_hbm_peak_median=nbytes[name] * n / (r["median_us"] * 1e-6) / HBM_PEAK,
                                  fraction_of_hbm_peak_min_time=nbytes[name] * n / (r["min_us"] * 1e-6) / HBM_PEAK,
                                  timed="event pair per launch (includes the launch)", package_root=args.package_root)), flush=True)
        del plans
    ctl.close()


if __name__ == "__main__":
    main()
