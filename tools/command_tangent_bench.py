"""Timings behind profiles/command_tangent.md: qc_commander_step_tangent_batch and qc_com_reference_tangent_batch at K = 1 and K = 12
on 4 096, 65 536 and 262 144 robots; next to each, in the same process and under the same protocol, 12 launches of its adjoint;
and one closed commander step with the 6 twist tangents of a command Jacobian, and one closed leaned step with the 16 tangents of a
shared schedule, each next to one step of its reverse-mode twin, forward plus backward.

  python tools/command_tangent_bench.py --out command_tangent.json

Cold-cache protocol (tools/sensitivity_swing_bench.py's): the launches rotate through distinct buffer sets of together at least
512 MiB - twice the 256 MiB last-level cache -, every set is touched once before timing; one HIP event pair per launch, so the figure
INCLUDES the launch itself.  Bytes are the algorithm's, per (direction, robot) PAIR, every tangent given and every output written:
  commander step  base Rwb 72, x 24, twist 48, fresh 1, the record 208: 353 B (from L2 for every direction but the first);
                  tangents two [6] and six [3] rows 240 B; written four [3] rows and one [6] row 144 B                          737 B
                  the adjoint, per robot: the same base, five cotangents 216 B, eight outputs 336 B: 905 B
  com reference   base feet 96, gait_phase 32, Rwb 72, x 24, schedule 128: 352 B; tangents x_d_in 24, feet 96, Rwb_rot 24, x 24,
                  phase 32, schedule 128: 328 B; written x_d_out_tan 24, com_xy_tan 16                                          720 B
                  the adjoint, per robot: the same base, x_d_out_bar 24, six outputs 448 B: 824 B
The closed-loop figures are whole calls of rollout_commander_tangent() / rollout_lean_tangent() on a fresh copy of the batch, planning
and buffers included, at steps = 1 and steps = 11: a tenth of the difference is one step's launches.  The reverse-mode figures are one
step of rollout_commander_autograd() / rollout_gait_autograd(lean=...), forward plus backward, Python's autograd included.
All robots apply a fresh command (the commander's expensive branch); the polygon is a trot mid-stride with widths of 0.2."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plant_bench import HBM_PEAK, timed  # noqa: E402
from sensitivity_rotation_bench import ROTATE_BYTES, timed_rotating  # noqa: E402

CMD_PAIR, CMD_ADJOINT = 353 + 240 + 144, 353 + 216 + 336
COM_PAIR, COM_ADJOINT = 352 + 328 + 40, 352 + 24 + 448


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 262144])
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--max-sets", type=int, default=256)
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import torch

    import quadruped_control_amd as q
    from quadruped_control_amd import tangent as T
    from quadruped_control_amd import workloads
    from quadruped_control_amd.balance_controller import new_commander_states, new_swing_states

    assert torch.cuda.is_available(), "command_tangent_bench needs the GPU: a timing taken elsewhere says nothing"
    ctl = q.BalanceController.from_params(q.cheetah_params(mu=0.6), device=0)
    res = {"device": torch.cuda.get_device_name(0), "commander_pair_bytes": CMD_PAIR, "commander_adjoint_bytes": CMD_ADJOINT, "com_pair_bytes": COM_PAIR,
           "com_adjoint_bytes": COM_ADJOINT}
    rnd = lambda *shape: torch.randn(shape, dtype=torch.float64, device="cuda")
    for n in args.sizes:
        host = workloads.config3(n=n)
        pose = q.to_device({"Rwb": host["Rwb"], "x": np.c_[host["x"][:, :2], np.full(n, 0.26)]})
        rec = new_commander_states(n)
        rec["standing"], rec["gait_running"] = 1, 1
        records = torch.from_numpy(rec.view(np.uint8).reshape(n, -1)).cuda()
        fresh = torch.ones(n, dtype=torch.uint8, device="cuda")
        poly = q.to_device({"feet": host["feet"], "Rwb": host["Rwb"], "x": host["x"], "gait_phase": np.ascontiguousarray(np.tile([0.2, 0.7, 0.7, 0.2], (n, 1)))})
        plans = {}
        for K in (1, 12):
            for _ in range(int(min(args.max_sets, max(3, -(-ROTATE_BYTES // (n * K * CMD_PAIR)))))):
                dev = {k: v.clone() for k, v in pose.items()}
                tans = {k: rnd(K, n, w) for k, w in T.COMMANDER_STEP_TANGENTS.items()}
                out = {"Rwb_d_rot_tan": tans["Rwb_d_rot_prev_tan"], "x_d_tan": tans["x_d_prev_tan"], "xdot_d_tan": tans["xdot_d_prev_tan"],
                       "w_d_tan": tans["w_d_prev_tan"], "Vb_next_tan": tans["Vb_tan"]}
                plans.setdefault((f"commander_step_tangent K={K}", K * CMD_PAIR), []).append(
                    T.plan_commander_step_tangent(ctl, dev, dict(twist=0.3 * rnd(n, 6), fresh=fresh.clone()), records.clone(), tans, out=out)[0])
            for _ in range(int(min(args.max_sets, max(3, -(-ROTATE_BYTES // (n * K * COM_PAIR)))))):
                dev = {k: v.clone() for k, v in poly.items()}
                tans = {k: rnd(K, n, w) for k, w in T.COM_REFERENCE_TANGENTS.items() if k != "joint_q_tan"}
                plans.setdefault((f"com_reference_tangent K={K}", K * COM_PAIR), []).append(
                    T.plan_com_reference_tangent(ctl, dev, torch.full((n, 4, 4), 0.2, dtype=torch.float64, device="cuda"), None, tans, "offset", 0.7,
                                                 want=("x_d_out_tan", "com_xy_tan"))[0])
        for _ in range(int(min(args.max_sets, max(3, -(-ROTATE_BYTES // (n * CMD_ADJOINT)))))):
            dev = {k: v.clone() for k, v in pose.items()}
            cot = {"Rwb_d": rnd(n, 9), "x_d": rnd(n, 3), "xdot_d": rnd(n, 3), "w_d": rnd(n, 3), "Vb": rnd(n, 6)}
            one = ctl.plan_commander_step_adjoint(dev, dict(twist=0.3 * rnd(n, 6), fresh=fresh.clone()), records.clone(), cot)[0]
            plans.setdefault(("12 x commander_step_adjoint", 12 * CMD_ADJOINT), []).append(lambda one=one: [one() for _ in range(12)])
        for _ in range(int(min(args.max_sets, max(3, -(-ROTATE_BYTES // (n * COM_ADJOINT)))))):
            dev = {k: v.clone() for k, v in poly.items()}
            one = ctl.plan_com_reference_adjoint(dev, torch.full((n, 4, 4), 0.2, dtype=torch.float64, device="cuda"), rnd(n, 3), "offset", 0.7,
                                                 want=("x_d_in_bar", "feet_bar", "Rwb_bar", "x_bar", "phase_bar", "schedule_bar"))[0]
            plans.setdefault(("12 x com_reference_adjoint", 12 * COM_ADJOINT), []).append(lambda one=one: [one() for _ in range(12)])
        torch.cuda.synchronize()
        for (name, nbytes), launches in plans.items():
            r = timed_rotating(torch, launches, args.launches)
            r.update(sets=len(launches), bytes_per_robot=nbytes, fraction_of_hbm_peak_median=nbytes * n / (r["median_us"] * 1e-6) / HBM_PEAK)
            res[f"{name} n={n}"] = r
            print(json.dumps({f"{name} n={n}": r}), flush=True)
        del plans
        torch.cuda.empty_cache()
        # the closed steps: whole calls on a fresh copy of a standing batch at the start of a trot
        dt, inertia = 1.0 / 300.0, 0.02
        start = workloads.with_joint_angles(workloads.config3(n=n))
        start.pop("feet", None)
        start.pop("stance", None)
        start["joint_qdot"] = np.zeros((n, 12))
        start["gait_phase"] = np.ascontiguousarray(np.tile([0.1, 0.3, 0.3, 0.1], (n, 1)))
        start = dict(q.to_device(start), swing_state=torch.from_numpy(new_swing_states(n).view(np.uint8).reshape(n, -1)).cuda())
        state_names = ("Rwb", "x", "xdot", "w", "joint_q", "joint_qdot")
        lean_batch = lambda: {k: v.clone() for k, v in start.items()}
        cmd_batch = lambda: {k: v.clone() for k, v in start.items() if k not in ("Rwb_d", "x_d", "xdot_d", "w_d")}
        twist = 0.3 * rnd(n, 6)
        command = lambda tw=twist: dict(state=records.clone(), twist=tw, fresh=fresh)
        twist_seeds = torch.eye(6, dtype=torch.float64, device="cuda")[:, None, :].repeat(1, n, 1).contiguous()
        schedule = torch.full((4, 4), 0.2, dtype=torch.float64, device="cuda")
        schedule_seeds = torch.eye(16, dtype=torch.float64, device="cuda").reshape(16, 4, 4).contiguous()

        def commander_reverse():
            tw = twist.clone().requires_grad_(True)
            final, _ = ctl.rollout_commander_autograd(cmd_batch(), command(tw), 1, dt, inertia, dt, warm=False)
            sum(final[k].sum() for k in state_names).backward()

        def lean_reverse():
            sch = schedule.clone().requires_grad_(True)
            final, _ = ctl.rollout_gait_autograd(lean_batch(), 1, dt, inertia, dt, warm=False, lean=dict(schedule=sch))
            sum(final[k].sum() for k in state_names).backward()

        closed = ((f"rollout_commander_tangent K=6 steps=1 n={n}", lambda: T.rollout_commander_tangent(ctl, cmd_batch(), command(), 1, dt, inertia, dt, {"twist_tan": twist_seeds})),
                  (f"rollout_commander_tangent K=6 steps=11 n={n}", lambda: T.rollout_commander_tangent(ctl, cmd_batch(), command(), 11, dt, inertia, dt, {"twist_tan": twist_seeds})),
                  (f"rollout_commander_autograd, one step forward + backward n={n}", commander_reverse),
                  (f"rollout_lean_tangent K=16 steps=1 n={n}", lambda: T.rollout_lean_tangent(ctl, lean_batch(), 1, dt, inertia, dt, dict(schedule=schedule), {"schedule_tan": schedule_seeds})),
                  (f"rollout_lean_tangent K=16 steps=11 n={n}", lambda: T.rollout_lean_tangent(ctl, lean_batch(), 11, dt, inertia, dt, dict(schedule=schedule), {"schedule_tan": schedule_seeds})),
                  (f"rollout_gait_autograd(lean), one step forward + backward n={n}", lean_reverse))
        for name, fn in closed:
            res[name] = timed(torch, fn)
            print(json.dumps({name: res[name]}), flush=True)
        del start
        torch.cuda.empty_cache()
    ctl.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
