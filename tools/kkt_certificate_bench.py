"""Timings behind profiles/kkt_certificate.md: the certificate kernel alone (residuals only, and with every output), and
control_batch alone for an A/B against the parent commit in the same session.

  python tools/kkt_certificate_bench.py --out cert.json                  # everything, on the tree's own package
  python tools/kkt_certificate_bench.py --solve-only --package-root DIR  # control_batch alone on another checkout's package

HIP events around `reps` back-to-back launches after at least 25 ms of warm-up; `rounds` such windows per figure, median and
minimum reported (tools/plant_bench.py's protocol).  Bytes are the algorithm's: 484 B read per robot (state and desired state
240 B, feet 96 B, forces 96 B, stance 4 B ... as config 2 carries them) plus 16 B for the two residuals, or 220 B with every
output (lambda 96, grad 96, active 4, flags 4, residuals 16).  The timed launch includes the one-workgroup summary kernel when
--summary is given; by default it is the per-robot kernel alone."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plant_bench import HBM_PEAK, solve_cases, timed  # noqa: E402

BYTES_IN = 484
BYTES_OUT = {"residuals": 16, "all": 220}
WANT = {"residuals": ("primal", "stationarity"), "all": ("primal", "stationarity", "lambda", "grad", "active", "flags")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--solve-only", action="store_true")
    ap.add_argument("--summary", action="store_true", help="time the per-robot kernel together with the summary kernel")
    ap.add_argument("--package-root", default=os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 262144])
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import torch

    import quadruped_control_amd as q
    from quadruped_control_amd import workloads

    assert torch.cuda.is_available(), "kkt_certificate_bench needs the GPU: a timing taken elsewhere says nothing"
    res = {"package_root": args.package_root, "device": torch.cuda.get_device_name(0)}
    res.update(solve_cases(q, workloads, torch))
    if not args.solve_only:
        from quadruped_control_amd.balance_controller import certify_summary

        ctl = q.BalanceController.from_params(q.cheetah_params(), device=0)
        for n in args.sizes:  # the certificate alone, on the forces of a solve of that batch
            dev = q.to_device(workloads.config2(n=n))
            out = ctl.control_batch(dev)
            check = ctl.certify_batch(dev, out["grf_body"], want=())
            torch.cuda.synchronize()
            s = certify_summary(check["summary"])
            for name, want in WANT.items():
                launch, _ = ctl.plan_certify(dev, out["grf_body"], want=want, summary=args.summary)
                r = timed(torch, launch)
                nbytes = BYTES_IN + BYTES_OUT[name]
                r["bytes_per_robot"] = nbytes
                r["GBps_median"] = nbytes * n / r["median_us"] * 1e-3
                r["fraction_of_hbm_peak_median"] = nbytes * n / (r["median_us"] * 1e-6) / HBM_PEAK
                r["fraction_of_hbm_peak_min_time"] = nbytes * n / (r["min_us"] * 1e-6) / HBM_PEAK
                r["summary_timed"] = bool(args.summary)
                res[f"certify n={n} {name}"] = r
            res[f"certify n={n} verdict"] = s
        ctl.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
