"""Timings behind profiles/sensitivity_rotation.md: qc_sensitivity_rot_batch alone (the two entrywise outputs, and all four) on
4 096, 65 536 and 262 144 robots of config 3, and control_batch and sensitivity_batch alone for an A/B against the parent commit.

  python tools/sensitivity_rotation_bench.py                               # the rotation kernel, on the tree's own package
  python tools/sensitivity_rotation_bench.py --which all --launches 20     # one variant, few launches: the run to put under a kernel trace
  python tools/sensitivity_rotation_bench.py --others --package-root DIR   # control_batch and sensitivity_batch alone on another checkout's package

Cold-cache protocol (tools/sensitivity_bench.py's): the launches rotate through `sets` distinct buffer sets of together at least
512 MiB - twice the 256 MiB last-level cache - so a set has left the cache when its turn comes again; every set is touched once
before timing (code object, page tables).  One HIP event pair per launch, median / min / 90th percentile: that figure INCLUDES the
launch itself.  Bytes are the algorithm's: 696 B read per robot (Rwb and Rwb_d 144 B, the six state vectors 144 B, feet 96 B,
forces 96 B, cotangent 96 B, the angular half of b_bar 24 B, feet_bar 96 B; no contact mask) plus 144 B for the two entrywise outputs
or 192 B for all four.
--others: tools/plant_bench.py's solve_cases (config 2 cold, config 4 warm) and sensitivity_batch with every output under the
protocol above, on the package under --package-root: run it alternately on this tree and on a checkout of the parent commit."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plant_bench import solve_cases  # noqa: E402
from sensitivity_bench import ALL as SENSITIVITY_ALL  # noqa: E402
from sensitivity_bench import IN_BYTES as SENSITIVITY_IN, OUT_BYTES as SENSITIVITY_OUT  # noqa: E402

WANT = {"entrywise": ("Rwb_bar", "Rwb_d_bar"), "all": ("Rwb_bar", "Rwb_d_bar", "Rwb_rot_bar", "Rwb_d_rot_bar")}
IN_BYTES = (9 + 9 + 6 * 3 + 12) * 8 + 2 * 12 * 8 + 3 * 8 + 12 * 8  # state, feet, grf_body, grf_bar, b_bar[3:6], feet_bar
OUT_BYTES = {"entrywise": 144, "all": 192}
ROTATE_BYTES = 512 << 20


def timed_rotating(torch, launches, count):
    sets = len(launches)
    for l in launches:
        l()
    torch.cuda.synchronize()
    times = []
    for it in range(count):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launches[it % sets]()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    t = np.array(times)
    return dict(median_us=float(np.median(t)), min_us=float(t.min()), p90_us=float(np.percentile(t, 90)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--others", action="store_true")
    ap.add_argument("--package-root", default=os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    ap.add_argument("--which", choices=["entrywise", "all", "both"], default="both")
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 262144])
    ap.add_argument("--launches", type=int, default=60)
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import torch

    import quadruped_control_amd as q
    from quadruped_control_amd import workloads

    assert torch.cuda.is_available(), "sensitivity_rotation_bench needs the GPU: a timing taken elsewhere says nothing"
    if args.others:
        print(json.dumps(dict(package_root=args.package_root, **solve_cases(q, workloads, torch))), flush=True)
    ctl = q.BalanceController.from_params(q.cheetah_params(mu=0.6), device=0)
    names = ["entrywise", "all"] if args.which == "both" else [args.which]
    for n in args.sizes:
        per_set = n * ((SENSITIVITY_IN + SENSITIVITY_OUT["all"]) if args.others else (IN_BYTES + OUT_BYTES["all"]))
        sets = max(3, -(-ROTATE_BYTES // per_set))
        plans = {name: [] for name in (["sensitivity all"] if args.others else names)}
        base = q.to_device(workloads.config3(n=n))
        for k in range(sets):  # distinct memory per set; the states of set k are the base batch's (the time does not depend on them)
            dev = {key: v.clone() for key, v in base.items()}
            out = ctl.control_batch(dev)
            gbar = torch.randn((n, 12), dtype=torch.float64, device="cuda")
            if args.others:
                plans["sensitivity all"].append(ctl.plan_sensitivity(dev, out["grf_body"], gbar, want=SENSITIVITY_ALL)[0])
                continue
            s = ctl.sensitivity_batch(dev, out["grf_body"], gbar, want=("b_bar", "feet_bar"))
            for name in names:
                plans[name].append(ctl.plan_sensitivity_rotation(dev, out["grf_body"], gbar, s["b_bar"], s["feet_bar"], want=WANT[name])[0])
        torch.cuda.synchronize()
        for name, launches in plans.items():
            nbytes = SENSITIVITY_IN + SENSITIVITY_OUT["all"] if args.others else IN_BYTES + OUT_BYTES[name]
            print(json.dumps(dict(what=name if args.others else "sensitivity_rotation " + name, n=n, sets=sets, rotating_MiB=sets * per_set >> 20,
                                  launches=args.launches, **timed_rotating(torch, launches, args.launches), bytes_per_robot=nbytes,
                                  timed="event pair per launch (includes the launch)", package_root=args.package_root)), flush=True)
    ctl.close()


if __name__ == "__main__":
    main()
