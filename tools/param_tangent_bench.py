"""Timings behind profiles/param_tangent.md: qc_param_tangent_batch with K = 1 and 12 directions per launch, with and without
grf_tan_in, on 4 096, 65 536 and 262 144 robots of config 3, and in the same process qc_tangent_batch at the same K (the same
classification and factorisation: the ratio says what a fused call would save) and 12 pairs of qc_sensitivity_batch +
qc_sensitivity_param_batch with rows (what a parameter Jacobian of 12 rows costs without this entry point).  With --rollout, one
closed rollout_tangent() step with 12 parameter tangents against one rollout_autograd(params=...) step forward + backward.

  python tools/param_tangent_bench.py
  python tools/param_tangent_bench.py --sizes 4096 --dirs 12 --launches 20     # one case, few launches: the run to put under a kernel trace

tools/tangent_bench.py's protocol: launch-inclusive (one HIP event pair around what is timed, median / min / 90th percentile), cold
cache - what is timed rotates through `sets` distinct buffer sets of together at least 512 MiB, twice the last-level cache, every set
touched once before timing.  Bytes are the algorithm's: the solve's inputs and the forces once per robot (484 B), per direction
grf_tan out (96 B) and with grf_tan_in the same again in; the K x 211 doubles of param_tan are shared by the batch."""
import argparse
import json
import os
import sys

import numpy as np

ROTATE_BYTES = 512 << 20
FIXED_BYTES = (9 + 9 + 6 * 3 + 12) * 8 + 4 + 12 * 8  # state, feet, stance, grf_body
TAN_DIR_BYTES = (8 * 3 + 12 + 12) * 8                 # qc_tangent_batch: eight state tangents and feet_tan in, grf_tan out
SENS_BYTES = FIXED_BYTES + 96 + 12 * 8 + 4            # qc_sensitivity_batch: grf_bar in, the adjoint and flags out
ROWS_BYTES = FIXED_BYTES + 96 + 96 + 211 * 8          # qc_sensitivity_param_batch: grf_bar and the adjoint in, a row out
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
    ap.add_argument("--dirs", type=int, nargs="+", default=[1, 12])
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--rollout", action="store_true", help="also time one closed-loop step: rollout_tangent(params_tan: 12) against rollout_autograd(params=...)")
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import torch

    import quadruped_control_amd as q
    from quadruped_control_amd import workloads
    from quadruped_control_amd.tangent import TANGENTS, plan_param_tangent, plan_tangent, rollout_tangent

    assert torch.cuda.is_available(), "param_tangent_bench needs the GPU: a timing taken elsewhere says nothing"
    ctl = q.BalanceController.from_params(q.cheetah_params(mu=0.6), device=0)
    names = [k for k in TANGENTS if k != "joint_q_tan"]

    def report(what, n, sets, stats, nbytes, **more):
        print(json.dumps(dict(what=what, n=n, sets=sets, launches=args.launches, **stats, bytes_per_robot=nbytes,
                              share_of_hbm_peak=n * nbytes / (stats["median_us"] * 1e-6) / HBM_PEAK, timed="event pair (includes the launches)", **more)), flush=True)

    for n in args.sizes:
        base = q.to_device(workloads.config3(n=n))
        for K in args.dirs:
            per_set = n * (FIXED_BYTES + K * TAN_DIR_BYTES)
            sets = max(3, -(-ROTATE_BYTES // per_set))
            plain, added, state, pairs = [], [], [], []
            D = torch.randn((K, 211), dtype=torch.float64, device="cuda")
            for _ in range(sets):
                dev = {key: v.clone() for key, v in base.items()}
                grf = ctl.control_batch(dev)["grf_body"]
                tans = {k: torch.randn((K, n, TANGENTS[k]), dtype=torch.float64, device="cuda") for k in names}
                launch, out, _ = plan_tangent(ctl, dev, grf, tans)
                state.append(launch)
                plain.append(plan_param_tangent(ctl, dev, grf, D)[0])
                added.append(plan_param_tangent(ctl, dev, grf, D, add_to={"grf_tan": out["grf_tan"]})[0])
                if K == 12:
                    gbar = torch.randn((n, 12), dtype=torch.float64, device="cuda")
                    l1, s = ctl.plan_sensitivity(dev, grf, gbar, want=("adjoint",))
                    l2, _ = ctl.plan_sensitivity_params(dev, grf, gbar, s["adjoint"], want=("param_bar_rows",))
                    pairs.append((l1, l2))
            torch.cuda.synchronize()
            t_plain = timed(torch, lambda s: plain[s](), sets, args.launches)
            report(f"param_tangent K={K}", n, sets, t_plain, FIXED_BYTES + K * 96, K=K)
            report(f"param_tangent K={K}, grf_tan_in in place", n, sets, timed(torch, lambda s: added[s](), sets, args.launches), FIXED_BYTES + K * 192, K=K)
            t_state = timed(torch, lambda s: state[s](), sets, args.launches)
            report(f"tangent K={K} (the same factorisation)", n, sets, t_state, FIXED_BYTES + K * TAN_DIR_BYTES, K=K,
                   param_over_state=t_plain["median_us"] / t_state["median_us"])
            if pairs:
                def twelve(s):
                    for _ in range(12):
                        pairs[s][0]()
                        pairs[s][1]()

                t_rows = timed(torch, twelve, sets, args.launches)
                report("sensitivity + sensitivity_params (rows), 12 pairs", n, sets, t_rows, 12 * (SENS_BYTES + ROWS_BYTES),
                       over_param_tangent_K12=t_rows["median_us"] / t_plain["median_us"])
            del plain, added, state, pairs
            torch.cuda.empty_cache()
        if args.rollout:
            dt = 1.0 / 300.0
            fw = torch.zeros((n, 12), dtype=torch.float64, device="cuda")
            D = torch.randn((12, 211), dtype=torch.float64, device="cuda")

            def forward_mode(_):
                rollout_tangent(ctl, {key: v.clone() for key, v in base.items()}, fw, 1, dt, {}, params_tan=D)

            def reverse_mode(_):
                theta = ctl.parameter_tensor().requires_grad_(True)
                state, _ = ctl.rollout_autograd({key: v.clone() for key, v in base.items()}, fw, 1, dt, params=theta)
                sum(state[k].sum() for k in ("x", "xdot", "w")).backward()

            report("rollout_tangent, 1 step, 12 parameter tangents (planning included)", n, 1, timed(torch, forward_mode, 1, args.launches), 0)
            report("rollout_autograd(params), 1 step, forward + backward (one scalar loss)", n, 1, timed(torch, reverse_mode, 1, args.launches), 0)
    ctl.close()


if __name__ == "__main__":
    main()
