"""Timings behind profiles/swing_reference.md: qc_swing_reference_batch and qc_swing_reference_adjoint_batch alone on 4 096, 65 536 and
262 144 robots of config 3 with joint angles, on a trot mask (stance bytes, the two diagonals in turn) in two cases -
  edge     every robot crosses a stance -> swing edge on two legs in EVERY launch: the forward launches of a buffer set alternate between
           the two diagonals (the records are updated in place, so the legs that stood last time swing now); the reverse pass reads
           records whose legs all stood
  no-edge  the records already hold the mask and a trajectory for every swinging leg: nothing is planned, the records pass through
- and next to them, in the same process and under the same protocol, qc_sensitivity_swing_batch and the tick itself
(control_batch(want_torques=True) with swing_state and gait_dt).

  python tools/swing_reference_bench.py
  python tools/swing_reference_bench.py --which edge --launches 20 --no-siblings   # one case: the run to put under a kernel trace

Cold-cache protocol (tools/sensitivity_swing_bench.py's): the launches rotate through `sets` distinct buffer sets of together at least
512 MiB, every set is touched once before timing (more than 25 ms of launches), one HIP event pair per launch - the figure INCLUDES the
launch -, median / min / 90th percentile.  Bytes are the algorithm's, per robot:
  forward  read Rwb 72, x, xdot, w, xdot_d 96, joint_q 96, gait_phase 32, stance 4, the record 224; written swing_pos, swing_vel 192,
           planned 1, the record's eight words 32 and, on an edge, two legs' end points 96:                       845 B (edge), 749 B
  reverse  read Rwb 72, x, xdot, w 72, joint_q 96, gait_phase 32, stance 4, the record's words 32, four cotangents 384, five accumulators
           240; written eight outputs 456, flags 4:                                                              1392 B
The tick is given without a byte count: it is a solve, not a stream."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plant_bench import HBM_PEAK  # noqa: E402
from sensitivity_rotation_bench import ROTATE_BYTES, timed_rotating  # noqa: E402
from sensitivity_swing_bench import BYTES as SWING_BYTES  # noqa: E402
from sensitivity_swing_bench import swing_references  # noqa: E402

FORWARD_BYTES = {"edge": 72 + 96 + 96 + 32 + 4 + 224 + 192 + 1 + 32 + 96, "no-edge": 72 + 96 + 96 + 32 + 4 + 224 + 192 + 1 + 32}
ADJOINT_BYTES = 72 + 72 + 96 + 32 + 4 + 32 + 384 + 240 + 456 + 4
DIAGONALS = ([1, 0, 0, 1], [0, 1, 1, 0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    ap.add_argument("--which", choices=["edge", "no-edge", "all"], default="all")
    ap.add_argument("--no-siblings", action="store_true")
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 262144])
    ap.add_argument("--launches", type=int, default=60)
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import torch

    import quadruped_control_amd as q
    from quadruped_control_amd import workloads
    from quadruped_control_amd.balance_controller import new_swing_states

    assert torch.cuda.is_available(), "swing_reference_bench needs the GPU: a timing taken elsewhere says nothing"
    ctl = q.BalanceController.from_params(q.cheetah_params(mu=0.6), device=0)
    cases = ["edge", "no-edge"] if args.which == "all" else [args.which]
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rnd = lambda *shape: torch.randn(shape, dtype=torch.float64, device="cuda")
    for n in args.sizes:
        sets = max(3, -(-ROTATE_BYTES // (n * FORWARD_BYTES["no-edge"])))  # sized by the smallest footprint timed
        host = workloads.with_joint_angles(workloads.config3(n=n))
        host.pop("feet", None)
        host.pop("stance", None)
        host["joint_qdot"] = np.zeros((n, 12))
        masks = [np.where((np.arange(n) % 2 == 0)[:, None], DIAGONALS[0], DIAGONALS[1]).astype(np.uint8),
                 np.where((np.arange(n) % 2 == 0)[:, None], DIAGONALS[1], DIAGONALS[0]).astype(np.uint8)]
        held = swing_references(q, host)  # world points 0.02 m above every foot: trajectories that stay inside reach

        def records(case, mask):
            s = new_swing_states(n)
            s["leg_state"] = 1 if case == "edge" else mask
            s["has_traj"] = 0 if case == "edge" else 1 - mask
            s["p_start"], s["p_final"] = held, held
            return cuda(s.view(np.uint8).reshape(n, -1))

        base = q.to_device(host)
        base["gait_phase"] = torch.full((n, 4), 0.9, dtype=torch.float64, device="cuda")
        plans = {}
        for k in range(sets):  # distinct memory per set; the states of set k are the base batch's (the time does not depend on them)
            for case in cases:
                dev = {key: v.clone() for key, v in base.items()}
                rec = records(case, masks[0])
                out = {"swing_pos": rnd(n, 4, 3), "swing_vel": rnd(n, 4, 3), "planned": torch.zeros(n, dtype=torch.uint8, device="cuda")}
                stances = [cuda(m) for m in (masks if case == "edge" else masks[:1])]
                turns = [ctl.plan_swing_reference(dict(dev, stance=s, swing_state=rec), want=tuple(out), out=out)[0] for s in stances]

                def forward(turns=turns, at=[0]):  # an edge in every launch: the diagonals take turns on the same records
                    turns[at[0] % len(turns)]()
                    at[0] += 1

                plans.setdefault("swing_reference " + case, []).append(forward)
                cot = {name: rnd(n, 12) for name in ("swing_pos", "swing_vel", "p_start", "p_final")}
                ins = {"Rwb_bar_in": rnd(n, 9), "x_bar_in": rnd(n, 3), "xdot_bar_in": rnd(n, 3), "w_bar_in": rnd(n, 3), "joint_q_bar_in": rnd(n, 4, 3)}
                aout = dict({name[:-3]: t for name, t in ins.items()}, xdot_d_bar=rnd(n, 3), p_start_bar=cot["p_start"], p_final_bar=cot["p_final"])
                plans.setdefault("swing_reference_adjoint " + case, []).append(
                    ctl.plan_swing_reference_adjoint(dict(dev, stance=stances[0]), records(case, masks[0]), cot, out=aout, **ins)[0])
            if not args.no_siblings:
                dev = {key: v.clone() for key, v in base.items()}
                tick = dict(dev, swing_state=records("no-edge", masks[0]), gait_dt=torch.full((n,), 1.0 / 300.0, dtype=torch.float64, device="cuda"))
                plans.setdefault("the tick (control_batch with swing_state and gait_dt)", []).append(ctl.plan_batch(tick, want_torques=True)[0])
                sw = dict(dev, stance=cuda(masks[0]), swing_pos=cuda(held), swing_vel=torch.zeros((n, 12), dtype=torch.float64, device="cuda"))
                qin, rin, xin = rnd(n, 4, 3), rnd(n, 9), rnd(n, 3)
                sout = {"swing_pos_bar": rnd(n, 4, 3), "swing_vel_bar": rnd(n, 4, 3), "joint_q_bar": qin, "joint_qdot_bar": rnd(n, 4, 3), "Rwb_bar": rin, "x_bar": xin}
                plans.setdefault("sensitivity_swing trot", []).append(
                    ctl.plan_sensitivity_swing(sw, rnd(n, 12), out=sout, joint_q_bar_in=qin, Rwb_bar_in=rin, x_bar_in=xin)[0])
        torch.cuda.synchronize()
        for name, launches in plans.items():
            nbytes = (FORWARD_BYTES[name.split()[-1]] if name.startswith("swing_reference ") else
                      ADJOINT_BYTES if name.startswith("swing_reference_adjoint") else SWING_BYTES if name.startswith("sensitivity_swing") else None)
            r = timed_rotating(torch, launches, args.launches)
            rate = {} if nbytes is None else dict(bytes_per_robot=nbytes, fraction_of_hbm_peak_median=nbytes * n / (r["median_us"] * 1e-6) / HBM_PEAK,
                                                  fraction_of_hbm_peak_min_time=nbytes * n / (r["min_us"] * 1e-6) / HBM_PEAK)
            print(json.dumps(dict(what=name, n=n, sets=sets, launches=args.launches, **r, **rate, timed="event pair per launch (includes the launch)",
                                  package_root=args.package_root)), flush=True)
        del plans
    ctl.close()


if __name__ == "__main__":
    main()
