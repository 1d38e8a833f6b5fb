"""Timings behind profiles/plant_model.md: every instantiation of the plant steps with a model (qc_plant_step_model_batch,
qc_leg_plant_step_model_batch, qc_plant_step_model_adjoint_batch; include/qc_plant_model.h) next to the base kernel it extends, in one
process.

  python tools/plant_model_bench.py --out plant_model.json

tools/plant_adjoint_bench.py's protocol: HIP events around back-to-back launches after a warm-up (launch-inclusive), `rounds` windows,
median and minimum, over a ROTATION of independent copies of the arrays whose footprint is at least --footprint bytes (512 MiB), so a
launch never finds its inputs in the last-level cache: HBM figures at every batch size.  The forward kernels step each copy once per
rotation and are not reset.  Bytes are the algorithm's: the base kernel's plus 8 (mass), 72 (Ib), 48 (wrench) per robot read and 4
(flags) written; the reverse pass with every output asked for adds 48 + 8 + 72 B of stores.
ctl.rollout's step against another checkout: tools/plant_bench.py --package-root DIR."""
import argparse
import json
import os
import sys

HBM_PEAK = 8.0e12  # B/s, the MI355X's specified peak
BASE_BYTES = {"plant_step": 336 + 240, "leg_plant_step": 9 * 8 + 9 * 8 + 3 * 96 + 9 * 8 + 9 * 8 + 2 * 96 + 96 + 4, "plant_step_adjoint": 336 + 240 + 336}
MODEL_BYTES = (8, 72, 48)  # mass, Ib, wrench


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536, 262144])
    ap.add_argument("--footprint", type=float, default=512.0 * 2 ** 20, help="bytes all rotated copies together must exceed")
    ap.add_argument("--max-copies", type=int, default=512)
    args = ap.parse_args()
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    sys.path.insert(0, root)
    import numpy as np
    import torch

    import quadruped_control_amd as q
    from quadruped_control_amd import workloads
    from tools.plant_bench import timed, world_feet

    pm = q.plant_model
    assert torch.cuda.is_available(), "plant_model_bench needs the GPU: a timing taken elsewhere says nothing"
    res = {"device": torch.cuda.get_device_name(0), "footprint_bytes": args.footprint}
    P = q.cheetah_params()
    ctl = q.BalanceController.from_params(P, device=0)
    dt, inertia = 1.0 / 300.0, (0.02, 0.03, 0.025)
    combos = [(bool(v & 1), bool(v & 2), bool(v & 4)) for v in range(1, 8)]
    for n in args.sizes:
        b = workloads.config2(n=n)
        dev = q.to_device(b)
        grf = ctl.control_batch(dev)["grf_body"]
        pw = torch.from_numpy(world_feet(np, b)).cuda()
        gen = torch.Generator(device="cuda").manual_seed(n)
        rnd = lambda *shape: torch.rand(shape, dtype=torch.float64, device="cuda", generator=gen)
        full = {"mass": P["mass"] * (0.8 + 0.4 * rnd(n)), "Ib": (torch.from_numpy(np.asarray(P["Ib"]).reshape(1, 9)).cuda() * (0.8 + 0.4 * rnd(n, 1))).contiguous(),
                "wrench": 20.0 * (rnd(n, 6) - 0.5)}
        stand = torch.tensor([0.0, 0.8, -1.6] * 4, dtype=torch.float64, device="cuda").reshape(1, 12).repeat(n, 1)
        copies = int(min(args.max_copies, max(2, -(-args.footprint // (BASE_BYTES["plant_step"] * n)))))

        def state():
            return {k: dev[k].clone() for k in ("Rwb", "x", "xdot", "w")}

        def leg_state():
            return dict(state(), joint_q=stand.clone(), joint_qdot=torch.zeros_like(stand))

        def model(combo):
            m = {k: full[k].clone() for k, there in zip(("mass", "Ib", "wrench"), combo) if there}
            m["flags"] = torch.zeros((n,), dtype=torch.int32, device="cuda")
            return m

        def cots():
            return {k: torch.randn((n, m), dtype=torch.float64, device="cuda", generator=gen) for k, m in (("Rwb", 9), ("x", 3), ("xdot", 3), ("w", 3), ("feet", 12))}

        tau = 2.0 * (rnd(n, 12) - 0.5)
        cases = [("plant_step", None, lambda: ctl.plan_plant(state(), grf.clone(), pw.clone(), dt, torch.zeros_like(pw))),
                 ("leg_plant_step", None, lambda: ctl.plan_leg_plant(leg_state(), tau.clone(), dt, inertia, foot_world=torch.zeros_like(pw),
                                                                     flags=torch.zeros((n,), dtype=torch.int32, device="cuda"))),
                 ("plant_step_adjoint", None, lambda: ctl.plan_plant_adjoint(state(), grf.clone(), pw.clone(), dt, cots())[0])]
        for combo in combos:
            cases += [("plant_step", combo, lambda combo=combo: pm.plan_plant_step(ctl, state(), grf.clone(), pw.clone(), dt, model(combo), torch.zeros_like(pw))),
                      ("leg_plant_step", combo, lambda combo=combo: pm.plan_leg_plant_step(ctl, leg_state(), tau.clone(), dt, inertia, model(combo),
                                                                                           foot_world=torch.zeros_like(pw),
                                                                                           flags=torch.zeros((n,), dtype=torch.int32, device="cuda"))),
                      ("plant_step_adjoint", combo, lambda combo=combo: pm.plan_plant_step_adjoint(ctl, state(), grf.clone(), pw.clone(), dt,
                                                                                                   {k: v for k, v in model(combo).items() if k != "flags"}, cots())[0])]
        for name, combo, make in cases:
            launches = [make() for _ in range(copies)]
            turn = [0]

            def launch():
                launches[turn[0] % copies]()
                turn[0] += 1

            nbytes = BASE_BYTES[name]
            if combo is not None:
                nbytes += sum(m for m, there in zip(MODEL_BYTES, combo) if there) + (48 + 8 + 72 if name == "plant_step_adjoint" else 4)
            r = timed(torch, launch)
            r.update(copies=copies, bytes_per_robot=nbytes, GBps_median=nbytes * n / r["median_us"] * 1e-3,
                     fraction_of_hbm_peak_median=nbytes * n / (r["median_us"] * 1e-6) / HBM_PEAK)
            label = name if combo is None else name + "_model<" + ",".join(k for k, there in zip(("mass", "Ib", "wrench"), combo) if there) + ">"
            res[f"{label} n={n}"] = r
            del launches
            torch.cuda.empty_cache()
    ctl.close()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
