// qc_leg_plant_tangent.hpp - forward mode of the legged plant step (qc_leg_plant.hpp): qc_leg_plant_step_tangent_batch
// (include/qc_tangent.h), the kernel that follows qc_torque_tangent_batch in the forward-mode loop around the tick.  Given the state
// BEFORE a step, the torques and the contact inputs the step read, and K tangents on them, it writes the K tangents of what the step
// wrote (Rwb', x', xdot', w', joint_q', joint_qdot').  Rotations move along world-frame left tangents, as in qc_plant_tangent.hpp.
// Nothing is saved by the forward launch: the step is recomputed - force pass, body, IK - as qc_leg_plant_adjoint.hpp recomputes it.
//
// Per direction, in the notation of qc_leg_plant.hpp and its adjoint (G(g) = sum_r g_r H_r, leg_fk_hessian_apply):
//   stance leg    dp = J dq,  dg = J^-T (dtau - G(g) dq),  df = delta x f - R dg,  dr = delta x r + R dp,  dc = dx + dr
//   body          qc_plant_tangent.hpp's block from (df_l, dr_l): dfs, dtau = sum (dr x f + r x df), dh, dc, dwdot, the semi-implicit
//                 Euler lines, delta' = Jl(phi) dt dw' + Exp(phi) delta (left_jacobian_coefficients: series / quotients / limit)
//   stance leg, after the body has moved:  dp' = Rn^T (dc - dx' - delta' x (c - x')),  dqn = J(qn)^-1 dp',  dq' = dqn,
//                 dqd' = (dqn - dq) / dt   (wrap_PI has slope 1; inside reach leg_ik inverts leg_fk, so its derivative is the inverse
//                 Jacobian AT THE ANGLES IT RETURNED, as in the adjoint)
//   swing leg     dqd' = dqd + dt (dtau / I),  dq' = dq + dt dqd'
// The body's block is RESTATED from qc_plant_tangent.hpp, which stays as it is: there r = foot_world - x and dr = dp - dx, here
// r = R p and dr comes from the joints, and the forward half forms E and Rn as rigid_body_step does (the IK reads Rn).
//
// UNDEFINED TANGENTS: the adjoint's flags under the adjoint's rules.  Bit l: J(q_l) of a stance leg is outside
// leg_force_from_torque's band.  Bit 4 + l: the forward IK reported the foot out of reach, or J(qn_l) is outside the band.  A robot
// with any bit set gets NaN in every output row of every direction.  Other non-finite inputs propagate; nothing is clamped.
//
// Kernel: one lane per (direction, robot), the robot index fastest - pair j = k n + i, as plant_step_tangent_kernel -, FP64,
// workgroups of one wave, a grid stride once the grid is capped (LEG_PLANT_TANGENT_MAX_BLOCKS), no LDS, no scratch, the four legs
// unrolled.  A leg's angles, torques and tangents are loaded inside the force pass and only nine doubles per leg live across the
// body's block (stance: c, dc, dq; swing: dq', dqd'), as in leg_plant_step_kernel.  A pair reads ALL of its inputs before it writes
// anything and touches only its own rows, so every `_next_tan` may be the input tangent of its layout and joint_qdot_next_tan may
// be joint_tau_tan.  flags[i] is written by direction 0's lane.
#pragma once
#include "qc_leg_plant_adjoint.hpp"  // leg_fk_hessian_apply, leg_jacobian_solve, leg_force_from_torque, leg_ik
#include "qc_plant_tangent.hpp"      // left_jacobian_coefficients, world_apply, exp_apply

namespace qc {

struct LegPlantTangentArgs : BodyConst {
  double leg_inertia[3];
  const double *Rwb, *x, *xdot, *w;                 // [n][9], [n][3] x 3: the state BEFORE the step
  const double *joint_q, *joint_qdot, *joint_tau;   // [n][4][3]
  const uint8_t* stance;                            // the contact inputs of the forward call, optional
  const double* gait_phase;
  const double* gait_duty;
  const CmdState* cmd_state;
  long n_dir;                                       // K
  const double *Rwb_rot_tan, *x_tan, *xdot_tan, *w_tan;        // [K][n][3], nullptr: zero
  const double *joint_q_tan, *joint_qdot_tan, *joint_tau_tan;  // [K][n][4][3], nullptr: zero
  double *Rwb_rot_next_tan, *x_next_tan, *xdot_next_tan, *w_next_tan, *joint_q_next_tan, *joint_qdot_next_tan;  // optional OUT
  int32_t* flags;                                   // optional OUT
};

constexpr int LEG_PLANT_TANGENT_BLOCK = 64;  // one wave
constexpr int LEG_PLANT_TANGENT_MAX_BLOCKS = 4096;

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

// The nine entries of the leg Jacobian at t (as leg_force_from_torque and leg_jacobian_solve spell them), o = J v.
QC_DEV void leg_jacobian_apply(const LegGeom& lg, const LegTrig& t, const double (&v)[3], double (&o)[3]) {
  const double a = lg.L2 * t.c2 + lg.L3 * t.c23, b = lg.L2 * t.s2 + lg.L3 * t.s23;
  o[0] = a * v[1] + (lg.L3 * t.c23) * v[2];
  o[1] = (-lg.L1 * t.s1 - a * t.c1) * v[0] + (b * t.s1) * v[1] + (lg.L3 * t.s1 * t.s23) * v[2];
  o[2] = (lg.L1 * t.c1 - a * t.s1) * v[0] + (-b * t.c1) * v[1] + (-lg.L3 * t.s23 * t.c1) * v[2];
}

// leg_force_from_torque's band rule on the determinant of the leg Jacobian at t, alone: true when |det| is outside lo <= |det| <= 2^52
// (a NaN determinant is inside, as there).  leg_jacobian_solve has no band rule of its own; this is the bit that goes with it.
QC_DEV bool leg_jacobian_outside_band(const LegGeom& lg, const LegTrig& t) {
  const double L1 = lg.L1, L2 = lg.L2, L3 = lg.L3;
  const double a = L2 * t.c2 + L3 * t.c23, b = L2 * t.s2 + L3 * t.s23;
  const double J[9] = {0.0, a, L3 * t.c23, -L1 * t.s1 - a * t.c1, b * t.s1, L3 * t.s1 * t.s23, L1 * t.c1 - a * t.s1, -b * t.c1, -L3 * t.s23 * t.c1};
  const double c00 = J[4] * J[8] - J[5] * J[7], c01 = J[5] * J[6] - J[3] * J[8], c02 = J[3] * J[7] - J[4] * J[6];
  const double ad = fabs(J[0] * c00 + J[1] * c01 + J[2] * c02), lsum = fabs(L1) + fabs(L2) + fabs(L3);
  const double lo = fmax(2.220446049250313e-16, 1.4210854715202004e-14 * lsum * lsum * lsum);
  return (ad < lo) || (ad > 4503599627370496.0);
}

__global__ __launch_bounds__(LEG_PLANT_TANGENT_BLOCK) void leg_plant_step_tangent_kernel(const DevParams* __restrict__ Pg, const long n, const LegPlantTangentArgs a) {
  const long total = n * a.n_dir;
  for (long j = (long)blockIdx.x * LEG_PLANT_TANGENT_BLOCK + threadIdx.x; j < total; j += (long)gridDim.x * LEG_PLANT_TANGENT_BLOCK) {
    const long i = j % n;  // pair j = k n + i: the row of direction k and robot i in a [K][n][m] array is j itself
    CParams& P = *QC_PARAMS_HERE(Pg);
    double R[9], x[3], v[3], w[3];
    load9(a.Rwb, i, R);
    load3(a.x, i, x);
    load3(a.xdot, i, v);
    load3(a.w, i, w);
    double dl[3], dx[3], dv[3], dw[3];
    load3_or_zero(a.Rwb_rot_tan, j, dl);
    load3_or_zero(a.x_tan, j, dx);
    load3_or_zero(a.xdot_tan, j, dv);
    load3_or_zero(a.w_tan, j, dw);
    const uint32_t mask = load_contact_mask(&P, a.stance, a.gait_phase, a.gait_duty, i, a.cmd_state ? a.cmd_state[i].gait_running != 0 : true);

    // ---- force pass: the step's forces and moments and their tangents; the swing joints integrate
    double fs[3] = {0.0, 0.0, 0.0}, tau[3] = {0.0, 0.0, 0.0}, dfs[3] = {0.0, 0.0, 0.0}, dtau[3] = {0.0, 0.0, 0.0};
    // per leg across the body's block - stance: c (the pinned point), dcp (its tangent), dq0 (dq); swing: dq', dqd' in dcp, dq0
    double c[4][3], dcp[4][3], dq0[4][3];
    int flags = 0;
#pragma unroll
    for (int l = 0; l < 4; l++) {
      double q[3], tq[3], dq[3], dtq[3];
      load3(a.joint_q, 4 * i + l, q);
      load3(a.joint_tau, 4 * i + l, tq);
      load3_or_zero(a.joint_q_tan, 4 * j + l, dq);
      load3_or_zero(a.joint_tau_tan, 4 * j + l, dtq);
      if (mask & (1u << l)) {
        const LegGeom lg = {P.links[3 * l], P.links[3 * l + 1], P.links[3 * l + 2], P.hip[3 * l], P.hip[3 * l + 1], P.hip[3 * l + 2]};
        const LegTrig t = leg_trig(q);
        double p[3], r[3], g[3], rg[3], f[3], m[3];
        leg_fk(P, l, t, p);
        mat_vec(R, p, r);
        if (leg_force_from_torque(lg, t, tq, g)) flags |= 1 << l;
        mat_vec(R, g, rg);
#pragma unroll
        for (int k = 0; k < 3; k++) {
          c[l][k] = x[k] + r[k];
          f[k] = -rg[k];
        }
        cross3(r, f, m);
        // the tangents
        double dp[3], gy[3], rhs[3], dg[3], rdp[3], rdg[3], cr[3], cf[3], dr[3], df[3], m1[3], m2[3];
        leg_jacobian_apply(lg, t, dq, dp);
        leg_fk_hessian_apply(lg, t, g, dq, gy);
#pragma unroll
        for (int k = 0; k < 3; k++) rhs[k] = dtq[k] - gy[k];
        leg_force_from_torque(lg, t, rhs, dg);  // (the band is the leg's bit above)
        mat_vec(R, dp, rdp);
        mat_vec(R, dg, rdg);
        cross3(dl, r, cr);
        cross3(dl, f, cf);
#pragma unroll
        for (int k = 0; k < 3; k++) {
          dr[k] = cr[k] + rdp[k];
          df[k] = cf[k] - rdg[k];
          dcp[l][k] = dx[k] + dr[k];
          dq0[l][k] = dq[k];
        }
        cross3(dr, f, m1);
        cross3(r, df, m2);
#pragma unroll
        for (int k = 0; k < 3; k++) {
          fs[k] += f[k];
          tau[k] += m[k];
          dfs[k] += df[k];
          dtau[k] += m1[k] + m2[k];
        }
      } else {
        double dqd[3];
        load3_or_zero(a.joint_qdot_tan, 4 * j + l, dqd);
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const double s = dqd[k] + a.dt * (dtq[k] / a.leg_inertia[k]);
          dq0[l][k] = s;                   // dqd'
          dcp[l][k] = dq[k] + a.dt * s;    // dq'
          c[l][k] = 0.0;
        }
      }
    }
    // ---- wdot = Iw^-1 cc, cc = tau - w x h, h = Iw w, and their tangents (qc_plant_tangent.hpp)
    double h[3], gyro[3], cc[3], wdot[3];
    world_apply(R, a.Ib, w, h);
    cross3(w, h, gyro);
#pragma unroll
    for (int k = 0; k < 3; k++) cc[k] = tau[k] - gyro[k];
    world_apply(R, a.Ib_inv, cc, wdot);
    double dwdot[3];
    {
      double dh[3], dc[3], t0[3], t1[3], t2[3], t3[3], t4[3], t5[3], t6[3], t7[3];
      cross3(dl, w, t0);
#pragma unroll
      for (int k = 0; k < 3; k++) t0[k] = dw[k] - t0[k];
      world_apply(R, a.Ib, t0, t1);
      cross3(dl, h, t2);
#pragma unroll
      for (int k = 0; k < 3; k++) dh[k] = t2[k] + t1[k];
      cross3(dw, h, t3);
      cross3(w, dh, t4);
      cross3(dl, cc, t5);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        dc[k] = dtau[k] - t3[k] - t4[k];
        t5[k] = dc[k] - t5[k];
      }
      world_apply(R, a.Ib_inv, t5, t6);
      cross3(dl, wdot, t7);
#pragma unroll
      for (int k = 0; k < 3; k++) dwdot[k] = t6[k] + t7[k];
    }
    // ---- semi-implicit Euler
    double x1[3], phi[3], dv1[3], dx1[3], dw1[3], dphi[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double acc = fs[k] / a.mass - (k == 2 ? a.g : 0.0);
      const double v1 = v[k] + a.dt * acc;
      x1[k] = x[k] + a.dt * v1;
      phi[k] = a.dt * (w[k] + a.dt * wdot[k]);
      dv1[k] = dv[k] + a.dt * (dfs[k] / a.mass);
      dx1[k] = dx[k] + a.dt * dv1[k];
      dw1[k] = dw[k] + a.dt * dwdot[k];
      dphi[k] = a.dt * dw1[k];
    }
    // ---- Rn = Exp(phi) R, formed as rigid_body_step forms it (the IK reads it); delta' = Jl(phi) dphi + Exp(phi) delta
    const double xx = phi[0] * phi[0], yy = phi[1] * phi[1], zz = phi[2] * phi[2];
    const double th2 = xx + yy + zz;
    const double hh = 0.5 * sqrt(th2);
    double sh, ch;
    sincos_joint(hh, &sh, &ch);
    const double sc = hh > 0.0 ? sh / hh : 1.0;
    const double A = sc * ch, B = 0.5 * (sc * sc);
    double Rn[9];
    {
      const double E[9] = {1.0 - B * (yy + zz),                 B * (phi[0] * phi[1]) - A * phi[2], B * (phi[0] * phi[2]) + A * phi[1],
                           B * (phi[0] * phi[1]) + A * phi[2], 1.0 - B * (xx + zz),                 B * (phi[1] * phi[2]) - A * phi[0],
                           B * (phi[0] * phi[2]) - A * phi[1], B * (phi[1] * phi[2]) + A * phi[0], 1.0 - B * (xx + yy)};
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) Rn[3 * r + k] = E[3 * r] * R[k] + E[3 * r + 1] * R[3 + k] + E[3 * r + 2] * R[6 + k];
    }
    double Bj, Cj, jd[3], ed[3], dl1[3];
    left_jacobian_coefficients(th2, A, B, &Bj, &Cj);
    exp_apply(phi, Bj, Cj, dphi, jd);
    exp_apply(phi, A, B, dl, ed);
#pragma unroll
    for (int k = 0; k < 3; k++) dl1[k] = jd[k] + ed[k];
    // ---- IK pass: the stance feet stay where they were.  (The legs' constants are fetched again: held from the force pass on, the
    // 24 of them overflow the scalar registers, as in the adjoint.)
    CParams& P2 = *QC_PARAMS_HERE(Pg);
#pragma unroll
    for (int l = 0; l < 4; l++) {
      if (mask & (1u << l)) {
        const LegGeom lg = {P2.links[3 * l], P2.links[3 * l + 1], P2.links[3 * l + 2], P2.hip[3 * l], P2.hip[3 * l + 1], P2.hip[3 * l + 2]};
        const double d[3] = {c[l][0] - x1[0], c[l][1] - x1[1], c[l][2] - x1[2]};
        double pb[3], qn[3], cd[3], u[3], dpb[3], dqn[3];
        mat_t_vec(Rn, d, pb);
        if (leg_ik(lg, pb, qn)) flags |= 16 << l;
        cross3(dl1, d, cd);
#pragma unroll
        for (int k = 0; k < 3; k++) u[k] = dcp[l][k] - dx1[k] - cd[k];
        mat_t_vec(Rn, u, dpb);
        const LegTrig tn = leg_trig(qn);
        if (leg_jacobian_outside_band(lg, tn)) flags |= 16 << l;
        leg_jacobian_solve(lg, tn, dpb, dqn);
#pragma unroll
        for (int k = 0; k < 3; k++) {
          dcp[l][k] = dqn[k];                        // dq'
          dq0[l][k] = (dqn[k] - dq0[l][k]) / a.dt;   // dqd'
        }
      }
    }
    // every input of this pair has been read: an output may overwrite an input tangent.  A flagged robot has no tangent.
    const double nan = __builtin_nan("");
    const bool bad = flags != 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      dl1[k] = bad ? nan : dl1[k];
      dx1[k] = bad ? nan : dx1[k];
      dv1[k] = bad ? nan : dv1[k];
      dw1[k] = bad ? nan : dw1[k];
    }
    if (a.Rwb_rot_next_tan) store3(a.Rwb_rot_next_tan, j, dl1);
    if (a.x_next_tan) store3(a.x_next_tan, j, dx1);
    if (a.xdot_next_tan) store3(a.xdot_next_tan, j, dv1);
    if (a.w_next_tan) store3(a.w_next_tan, j, dw1);
#pragma unroll
    for (int l = 0; l < 4; l++) {
#pragma unroll
      for (int k = 0; k < 3; k++) {
        dcp[l][k] = bad ? nan : dcp[l][k];
        dq0[l][k] = bad ? nan : dq0[l][k];
      }
      if (a.joint_q_next_tan) store3(a.joint_q_next_tan, 4 * j + l, dcp[l]);
      if (a.joint_qdot_next_tan) store3(a.joint_qdot_next_tan, 4 * j + l, dq0[l]);
    }
    if (a.flags && j < n) a.flags[i] = flags;
  }
}

}  // namespace qc
#endif  // __HIPCC__
