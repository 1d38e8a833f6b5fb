"""Timings behind profiles/sensitivity_params.md: qc_sensitivity_param_batch alone - the batch sum only, the per-robot rows only, and
both - on 4 096, 65 536 and 262 144 robots of config 3, and the fused sum against rows-only followed by torch.sum(dim=0).

  python tools/sensitivity_params_bench.py                      # the three variants, then the fused-sum comparison
  python tools/sensitivity_params_bench.py --which sum --launches 20   # one variant, few launches: the run to put under a kernel trace

Cold-cache protocol (tools/sensitivity_rotation_bench.py's): the launches rotate through `sets` distinct buffer sets of together at
least 512 MiB - twice the 256 MiB last-level cache - so a set has left the cache when its turn comes again; every set is touched once
before timing.  One HIP event pair per launch, median / min / 90th percentile: that figure INCLUDES the launch itself (for the sum,
both kernels: the per-robot one and the one-workgroup finisher).  Bytes are the algorithm's: 672 B read per robot (Rwb and Rwb_d
144 B, the six state vectors 144 B, feet 96 B, forces 96 B, cotangent 96 B, adjoint 96 B; config 3 carries no contact mask) plus
1 688 B per robot for the rows; the sum writes 1 688 B per workgroup and 1 688 B in all.  The HBM fraction is against 8 TB/s.
The comparison: sum-only against rows-only followed by torch.sum(dim=0) on the same inputs, `--rounds` alternating runs of
`--launches` launches each under the same protocol; each run's median is printed, so the spread of the runs is visible."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sensitivity_rotation_bench import ROTATE_BYTES, timed_rotating  # noqa: E402

WANT = {"sum": ("param_bar",), "rows": ("param_bar_rows",), "both": ("param_bar", "param_bar_rows")}
IN_BYTES = (9 + 9 + 6 * 3 + 12) * 8 + 3 * 12 * 8  # state, feet, grf_body, grf_bar, adjoint
ROW_BYTES = 211 * 8
HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    ap.add_argument("--which", choices=["sum", "rows", "both", "all"], default="all")
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 262144])
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5, help="alternating runs of the fused-sum comparison (0: skip it)")
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import torch

    import quadruped_control_amd as q
    from quadruped_control_amd import workloads

    assert torch.cuda.is_available(), "sensitivity_params_bench needs the GPU: a timing taken elsewhere says nothing"
    ctl = q.BalanceController.from_params(q.cheetah_params(mu=0.6), device=0)
    names = ["sum", "rows", "both"] if args.which == "all" else [args.which]
    for n in args.sizes:
        per_set = n * (IN_BYTES + ROW_BYTES)
        sets = max(3, -(-ROTATE_BYTES // per_set))
        plans = {name: [] for name in names}
        unfused = []
        base = q.to_device(workloads.config3(n=n))
        for k in range(sets):  # distinct memory per set; the states of set k are the base batch's (the time does not depend on them)
            dev = {key: v.clone() for key, v in base.items()}
            out = ctl.control_batch(dev)
            gbar = torch.randn((n, 12), dtype=torch.float64, device="cuda")
            z = ctl.sensitivity_batch(dev, out["grf_body"], gbar, want=("adjoint",))["adjoint"]
            rows = None
            for name in names:
                launch, res = ctl.plan_sensitivity_params(dev, out["grf_body"], gbar, z, want=WANT[name])
                plans[name].append(launch)
                if name == "rows":
                    rows = (launch, res["param_bar_rows"])
            if rows is not None:
                total = torch.zeros(211, dtype=torch.float64, device="cuda")
                unfused.append(lambda rows=rows, total=total: (rows[0](), torch.sum(rows[1], dim=0, out=total)))
        torch.cuda.synchronize()
        for name, launches in plans.items():
            nbytes = IN_BYTES + (ROW_BYTES if name != "sum" else 0)
            t = timed_rotating(torch, launches, args.launches)
            print(json.dumps(dict(what="sensitivity_params " + name, n=n, sets=sets, rotating_MiB=sets * per_set >> 20, launches=args.launches, **t,
                                  bytes_per_robot=nbytes, hbm_fraction=round(n * nbytes / (t["median_us"] * 1e-6) / HBM_BYTES_PER_S, 4),
                                  timed="event pair per launch (includes the launch)", package_root=args.package_root)), flush=True)
        if args.rounds and "sum" in plans and unfused:
            fused, split = [], []
            for _ in range(args.rounds):
                fused.append(timed_rotating(torch, plans["sum"], args.launches)["median_us"])
                split.append(timed_rotating(torch, unfused, args.launches)["median_us"])
            print(json.dumps(dict(what="fused sum vs rows + torch.sum(dim=0)", n=n, rounds=args.rounds, launches=args.launches,
                                  fused_median_us=[round(v, 2) for v in fused], rows_then_torch_sum_median_us=[round(v, 2) for v in split],
                                  fused_spread_us=round(max(fused) - min(fused), 2), split_spread_us=round(max(split) - min(split), 2),
                                  ratio_of_medians=round(float(np.median(split) / np.median(fused)), 3))), flush=True)
    ctl.close()


if __name__ == "__main__":
    main()
