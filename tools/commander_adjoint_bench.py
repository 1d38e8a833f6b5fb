"""Timings behind profiles/commander_adjoint.md: qc_commander_step_batch and qc_commander_step_adjoint_batch alone on 4 096, 65 536 and
262 144 robots (the poses of config 3, every record standing and running) in two cases -
  applied  every robot gets a fresh command in EVERY launch and applies it (the records are updated in place: Vb, the desired state)
  idle     no command is fresh and none is pending: nothing is applied, the records pass through
- and next to them, in the same process and under the same protocol, qc_plant_step_batch (the stream kernel these are measured against).

  python tools/commander_adjoint_bench.py
  python tools/commander_adjoint_bench.py --which applied --launches 20 --no-siblings   # one case: the run to put under a kernel trace

Cold-cache protocol (tools/sensitivity_swing_bench.py's): the launches rotate through `sets` distinct buffer sets of together at least
512 MiB, every set is touched once before timing, one HIP event pair per launch - the figure INCLUDES the launch -, median / min / 90th
percentile.  Bytes are the algorithm's, per robot:
  forward  read Rwb 72, x 24, twist 48, fresh 1, the record 208; written the four desired arrays 144, run and applied 2 and, where a
           command is applied, the record's cmd_pending 4, Vb 48 and desired state 144:                          695 B (applied), 499 B
  reverse  read Rwb 72, x 24, twist 48, fresh 1, the record's words and Vb 64, five cotangents 192, two accumulators 96; written eight
           outputs 336, flags 4:                                                                                 837 B
  plant    tools/plant_bench.py's 576 B"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plant_bench import HBM_PEAK, PLANT_BYTES, world_feet  # noqa: E402
from sensitivity_rotation_bench import ROTATE_BYTES, timed_rotating  # noqa: E402

FORWARD_BYTES = {"applied": 72 + 24 + 48 + 1 + 208 + 144 + 2 + 4 + 48 + 144, "idle": 72 + 24 + 48 + 1 + 208 + 144 + 2}
ADJOINT_BYTES = 72 + 24 + 48 + 1 + 64 + 192 + 96 + 336 + 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    ap.add_argument("--which", choices=["applied", "idle", "all"], default="all")
    ap.add_argument("--no-siblings", action="store_true")
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 262144])
    ap.add_argument("--launches", type=int, default=60)
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import torch

    import quadruped_control_amd as q
    from quadruped_control_amd import workloads
    from quadruped_control_amd.balance_controller import new_commander_states

    assert torch.cuda.is_available(), "commander_adjoint_bench needs the GPU: a timing taken elsewhere says nothing"
    ctl = q.BalanceController.from_params(q.cheetah_params(mu=0.6), device=0)
    cases = ["applied", "idle"] if args.which == "all" else [args.which]
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rnd = lambda *shape: torch.randn(shape, dtype=torch.float64, device="cuda")
    for n in args.sizes:
        sets = max(3, -(-ROTATE_BYTES // (n * FORWARD_BYTES["idle"])))  # sized by the smallest footprint timed
        host = workloads.config3(n=n)
        base = q.to_device({k: host[k] for k in ("Rwb", "x")})

        def records():
            s = new_commander_states(n)
            s["standing"], s["gait_running"] = 1, 1
            return cuda(s.view(np.uint8).reshape(n, -1))

        plans = {}
        for k in range(sets):  # distinct memory per set; the poses of set k are the base batch's (the time does not depend on them)
            for case in cases:
                dev = {key: v.clone() for key, v in base.items()}
                fresh = torch.full((n,), 1 if case == "applied" else 0, dtype=torch.uint8, device="cuda")
                cmd = {"state": records(), "twist": 0.3 * rnd(n, 6), "fresh": fresh}
                out = {"Rwb_d": rnd(n, 9), "x_d": rnd(n, 3), "xdot_d": rnd(n, 3), "w_d": rnd(n, 3), "run": torch.zeros(n, dtype=torch.uint8, device="cuda"),
                       "applied": torch.zeros(n, dtype=torch.uint8, device="cuda")}
                plans.setdefault("commander_step " + case, []).append(ctl.plan_commander_step(dev, cmd, want=tuple(out), out=out)[0])
                cot = {"Rwb_d": rnd(n, 9), "x_d": rnd(n, 3), "xdot_d": rnd(n, 3), "w_d": rnd(n, 3), "Vb": rnd(n, 6)}
                ins = {"Rwb_bar_in": rnd(n, 9), "x_bar_in": rnd(n, 3)}
                aout = {"twist_bar": rnd(n, 6), "Vb_bar": cot["Vb"], "Rwb_bar": ins["Rwb_bar_in"], "x_bar": ins["x_bar_in"], "Rwb_d_prev_bar": cot["Rwb_d"],
                        "x_d_prev_bar": cot["x_d"], "xdot_d_prev_bar": cot["xdot_d"], "w_d_prev_bar": cot["w_d"]}
                plans.setdefault("commander_step_adjoint " + case, []).append(
                    ctl.plan_commander_step_adjoint(dev, cmd, records(), cot, want=tuple(aout), out=aout, **ins)[0])
            if not args.no_siblings:
                b = workloads.config2(n=n)
                pdev = q.to_device(b)
                grf = 10.0 * rnd(n, 12)
                state = {key: pdev[key] for key in ("Rwb", "x", "xdot", "w")}
                plans.setdefault("plant_step", []).append(ctl.plan_plant(state, grf, cuda(world_feet(np, b)), 1.0 / 300.0, pdev["feet"]))
        torch.cuda.synchronize()
        for name, launches in plans.items():
            nbytes = (FORWARD_BYTES[name.split()[-1]] if name.startswith("commander_step ") else
                      ADJOINT_BYTES if name.startswith("commander_step_adjoint") else PLANT_BYTES)
            r = timed_rotating(torch, launches, args.launches)
            rate = dict(bytes_per_robot=nbytes, fraction_of_hbm_peak_median=nbytes * n / (r["median_us"] * 1e-6) / HBM_PEAK,
                        fraction_of_hbm_peak_min_time=nbytes * n / (r["min_us"] * 1e-6) / HBM_PEAK)
            print(json.dumps(dict(what=name, n=n, sets=sets, launches=args.launches, **r, **rate, timed="event pair per launch (includes the launch)",
                                  package_root=args.package_root)), flush=True)
        del plans
    ctl.close()


if __name__ == "__main__":
    main()
