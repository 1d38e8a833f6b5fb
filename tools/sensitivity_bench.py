"""Timings behind profiles/sensitivity.md: qc_sensitivity_batch alone (adjoint only, and every output) on 4 096, 65 536 and
262 144 robots of config 3, and control_batch alone for an A/B against the parent commit.

  python tools/sensitivity_bench.py                                     # the sensitivity kernel, on the tree's own package
  python tools/sensitivity_bench.py --which all --launches 20           # one variant, few launches: the run to put under a kernel trace
  python tools/sensitivity_bench.py --solve-only --package-root DIR     # control_batch alone on another checkout's package

Sensitivity, cold-cache protocol: the launches rotate through `sets` distinct buffer sets of together at least 512 MiB - twice
the 256 MiB last-level cache - so a set has left the cache when its turn comes again (135 / 9 / 3 sets at the three sizes); every
set is touched once before timing (code object, page tables), which leaves only the last ones resident and they are the last to
be reused.  One HIP event pair per launch, median / min / 90th percentile of the launches: that figure INCLUDES the launch itself;
the kernel's own time comes from a kernel trace of this tool, one run per variant.  Bytes are the algorithm's: 580 B read per robot
(Rwb and Rwb_d 144 B, the six state vectors 144 B, feet 96 B, stance 4 B, forces 96 B, cotangent 96 B) plus 96 B for the adjoint or
388 B for every output.
--solve-only is tools/plant_bench.py's solve_cases, the protocol of the earlier A/Bs (config 2 cold, config 4 warm)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plant_bench import solve_cases  # noqa: E402

ALL = ("adjoint", "b_bar", "feet_bar", "x_bar", "xdot_bar", "w_bar", "x_d_bar", "xdot_d_bar", "w_d_bar", "flags")
WANT = {"adjoint": ("adjoint",), "all": ALL}
IN_BYTES = (9 + 9 + 6 * 3 + 12) * 8 + 4 + 2 * 12 * 8  # state, feet, stance, grf_body, grf_bar
OUT_BYTES = {"adjoint": 96, "all": (12 + 6 + 12 + 6 * 3) * 8 + 4}
ROTATE_BYTES = 512 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--solve-only", action="store_true")
    ap.add_argument("--package-root", default=os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    ap.add_argument("--which", choices=["adjoint", "all", "both"], default="both")
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 262144])
    ap.add_argument("--launches", type=int, default=60)
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import torch

    import quadruped_control_amd as q
    from quadruped_control_amd import workloads

    assert torch.cuda.is_available(), "sensitivity_bench needs the GPU: a timing taken elsewhere says nothing"
    if args.solve_only:
        print(json.dumps(dict(package_root=args.package_root, **solve_cases(q, workloads, torch))), flush=True)
        return
    ctl = q.BalanceController.from_params(q.cheetah_params(mu=0.6), device=0)
    names = ["adjoint", "all"] if args.which == "both" else [args.which]
    for n in args.sizes:
        per_set = n * (IN_BYTES + OUT_BYTES["all"])
        sets = max(3, -(-ROTATE_BYTES // per_set))
        plans = {name: [] for name in names}
        base = q.to_device(workloads.config3(n=n))
        for k in range(sets):  # distinct memory per set; the states of set k are the base batch's (the time does not depend on them)
            dev = {key: v.clone() for key, v in base.items()}
            out = ctl.control_batch(dev)
            gbar = torch.randn((n, 12), dtype=torch.float64, device="cuda")
            for name in names:
                plans[name].append(ctl.plan_sensitivity(dev, out["grf_body"], gbar, want=WANT[name])[0])
        torch.cuda.synchronize()
        for name, launches in plans.items():
            for l in launches:
                l()
            torch.cuda.synchronize()
            times = []
            for it in range(args.launches):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launches[it % sets]()
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b) * 1e3)
            t = np.array(times)
            print(json.dumps(dict(what="sensitivity " + name, n=n, sets=sets, rotating_MiB=sets * per_set >> 20, launches=args.launches,
                                  median_us=float(np.median(t)), min_us=float(t.min()), p90_us=float(np.percentile(t, 90)),
                                  bytes_per_robot=IN_BYTES + OUT_BYTES[name], timed="event pair per launch (includes the launch)")), flush=True)
    ctl.close()


if __name__ == "__main__":
    main()
