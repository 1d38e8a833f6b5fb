"""Timings behind profiles/tangent.md: qc_tangent_batch with K = 1, 12 and 30 directions per launch on 4 096, 65 536 and 262 144
robots of config 3, and in the same process K single-direction launches, 12 launches of qc_sensitivity_batch (the route to a
Jacobian without this entry point) and the plant kernel as the bandwidth yardstick.

  python tools/tangent_bench.py
  python tools/tangent_bench.py --sizes 4096 --dirs 12 --launches 20     # one case, few launches: the run to put under a kernel trace

tools/sensitivity_bench.py's protocol: launch-inclusive (one HIP event pair around what is timed, median / min / 90th percentile),
cold cache - what is timed rotates through `sets` distinct buffer sets of together at least 512 MiB, twice the last-level cache,
every set touched once before timing.  Bytes are the algorithm's: the solve's inputs and the forces once per robot (484 B), and per
direction eight state tangents (192 B), feet_tan (96 B) in and grf_tan (96 B) out."""
import argparse
import json
import os
import sys

import numpy as np

ROTATE_BYTES = 512 << 20
FIXED_BYTES = (9 + 9 + 6 * 3 + 12) * 8 + 4 + 12 * 8  # state, feet, stance, grf_body
DIR_BYTES = (8 * 3 + 12 + 12) * 8                     # eight state tangents and feet_tan in, grf_tan out
SENS_BYTES = FIXED_BYTES + 96 + (12 + 6 + 12 + 6 * 3) * 8 + 4
PLANT_BYTES = (9 + 3 * 3 + 12 + 12) * 8 * 2 - 96      # plant step: state, forces and feet in, state and feet out
HBM_PEAK = 8.0e12                                      # B/s, the MI355X's


def timed(torch, fn, sets, launches):
    for k in range(sets):
        fn(k)
    torch.cuda.synchronize()
    times = []
    for it in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(it % sets)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    t = np.array(times)
    return dict(median_us=float(np.median(t)), min_us=float(t.min()), p90_us=float(np.percentile(t, 90)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 262144])
    ap.add_argument("--dirs", type=int, nargs="+", default=[1, 12, 30])
    ap.add_argument("--launches", type=int, default=30)
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import torch

    import quadruped_control_amd as q
    from quadruped_control_amd import workloads
    from quadruped_control_amd.tangent import TANGENTS, plan_tangent

    assert torch.cuda.is_available(), "tangent_bench needs the GPU: a timing taken elsewhere says nothing"
    ctl = q.BalanceController.from_params(q.cheetah_params(mu=0.6), device=0)
    names = [k for k in TANGENTS if k != "joint_q_tan"]

    def report(what, n, sets, stats, nbytes, **more):
        print(json.dumps(dict(what=what, n=n, sets=sets, launches=args.launches, **stats, bytes_per_robot=nbytes,
                              share_of_hbm_peak=n * nbytes / (stats["median_us"] * 1e-6) / HBM_PEAK, timed="event pair (includes the launches)", **more)), flush=True)

    for n in args.sizes:
        base = q.to_device(workloads.config3(n=n))
        for K in args.dirs:
            per_set = n * (FIXED_BYTES + K * DIR_BYTES)
            sets = max(3, -(-ROTATE_BYTES // per_set))
            many, singles, sens = [], [], []
            for _ in range(sets):
                dev = {key: v.clone() for key, v in base.items()}
                grf = ctl.control_batch(dev)["grf_body"]
                tans = {k: torch.randn((K, n, TANGENTS[k]), dtype=torch.float64, device="cuda") for k in names}
                many.append(plan_tangent(ctl, dev, grf, tans)[0])
                singles.append([plan_tangent(ctl, dev, grf, {k: v[j] for k, v in tans.items()})[0] for j in range(K)])
                if K == 12:
                    gbar = torch.randn((n, 12), dtype=torch.float64, device="cuda")
                    sens.append(ctl.plan_sensitivity(dev, grf, gbar, want=("adjoint", "b_bar", "feet_bar", "x_bar", "xdot_bar", "w_bar", "x_d_bar",
                                                                             "xdot_d_bar", "w_d_bar"))[0])
            torch.cuda.synchronize()
            report(f"tangent K={K}, one launch", n, sets, timed(torch, lambda s: many[s](), sets, args.launches), FIXED_BYTES + K * DIR_BYTES, K=K)

            def each(s):
                for l in singles[s]:
                    l()

            report(f"tangent K=1, {K} launches", n, sets, timed(torch, each, sets, args.launches), K * (FIXED_BYTES + DIR_BYTES), K=K)
            if sens:
                def twelve(s):
                    for _ in range(12):
                        sens[s]()

                report("sensitivity (every output), 12 launches", n, sets, timed(torch, twelve, sets, args.launches), 12 * SENS_BYTES)
            del many, singles, sens
            torch.cuda.empty_cache()
        # the bandwidth yardstick: the plant step on the same number of robots
        sets = max(3, -(-ROTATE_BYTES // (n * PLANT_BYTES)))
        plants = []
        for _ in range(sets):
            dev = {key: v.clone() for key, v in base.items()}
            grf = ctl.control_batch(dev)["grf_body"]
            fw = torch.zeros((n, 12), dtype=torch.float64, device="cuda")
            plants.append(ctl.plan_plant({k: dev[k] for k in ("Rwb", "x", "xdot", "w")}, grf, fw, 1.0 / 300.0, feet=dev["feet"]))
        torch.cuda.synchronize()
        report("plant step (yardstick)", n, sets, timed(torch, lambda s: plants[s](), sets, args.launches), PLANT_BYTES)
        del plants
        torch.cuda.empty_cache()
    ctl.close()


if __name__ == "__main__":
    main()
