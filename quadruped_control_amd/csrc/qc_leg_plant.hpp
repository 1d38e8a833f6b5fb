// qc_leg_plant.hpp - the plant behind the COMPLETE tick, stepped on the device: a single rigid body on four massless legs, driven
// by the joint torques qc_control_batch (joint_q / joint_tau) and qc_tick_batch write.  qc_leg_plant_step_batch
// (include/qc_balance.h) alternates with the tick on one stream, so stand, gait start and twist tracking run without a host in the loop.
//
// Per robot (conventions of qc_plant.hpp; leg kinematics of qc_device.hpp):
//   contact mask   contact_mask (qc_device.hpp): the rule of qc_control_batch on the phases as the tick left them
//   stance leg i   t = leg_trig(q_i), p_i = leg_fk, J_i (the nine entries of swing_pd);  g_i = J_i^-T tau_i is the force the torque
//                  encodes (the tick wrote tau = J^T grf_body, clamped: the clamp is the plant's actuator limit), by the cofactors
//                  inside swing_pd's band lo <= |det| <= 2^52 and by pinv3_apply on J^T outside it (flags bit i);
//                  f_i = -Rwb g_i acts at r_i = Rwb p_i, and the foot is pinned at c_i = x + r_i
//   swing leg      no force on the body; three decoupled double integrators: qdot' = qdot + dt (tau / I), q' = q + dt qdot'
//   body           rigid_body_step (qc_plant.hpp): plant_step_kernel's own step from fs, tau on
//   stance leg, after the body has moved:  p_i' = Rwb'^T (c_i - x'),  q_i' = leg_ik(p_i'),  qdot_i' = wrap_PI(q_i' - q_i) / dt;
//                  a clamped (d > 1) or NaN (d < -1) leg sets flags bit 4 + i
// There is no ground, no leg mass, no gravity on the joints ("Closing the loop around the tick").
//
// Kernel: ONE LANE PER ROBOT, FP64, no LDS, no scratch; the four legs are unrolled, so every per-leg value has a compile-time
// register.  Between the force pass and the IK pass a lane holds, per leg, c_i, q_i (stance) or q_i', qdot_i' (swing) - 9 doubles -
// next to the body's 18 + 9: ~130 VGPRs of state under an IK working set of ~40, which the compiler keeps in registers
// (profiles/leg_plant_kernel_resources.txt has the count; the per-(robot, leg) layout with group_sum<4> was not needed).  The
// kernel is instruction-bound (twelve sincos_joint, twenty atan2, 4 + 12 divisions per robot), so the lower occupancy of a
// 200-VGPR kernel costs little: there is no memory latency of note to hide.  Each lane reads all of its inputs before it
// writes, and touches only its own rows.
#pragma once
#include "qc_plant.hpp"

namespace qc {

// The kernel's argument struct (by value in the kernarg segment).
struct LegPlantArgs : BodyConst {
  double leg_inertia[3];
  double *Rwb, *x, *xdot, *w;     // IN/OUT
  double *joint_q, *joint_qdot;   // [n][4][3] IN/OUT
  const double* joint_tau;        // [n][4][3]
  const uint8_t* stance;          // optional
  const double* gait_phase;       // optional
  const double* gait_duty;        // optional
  const CmdState* cmd_state;      // optional
  double* foot_world;             // optional OUT
  int32_t* flags;                 // optional OUT
};

constexpr int LEG_PLANT_BLOCK = 256;

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

// legInverseKinematics (kinematics.cpp:117-160), stand-alone and reference-shaped (the evaluation leg_swing_torque keeps as its
// fallback): unsigned link lengths, d > 1 clamped to 1, d < -1 not clamped (sqrt of a negative number: q2 and q3 NaN, as in the
// reference).  Returns true when the foot is out of reach: d was clamped, or d is not >= -1.  q3 <= 0: the reference's knee branch.
QC_DEV bool leg_ik(const LegGeom& g, const double (&pb)[3], double (&q)[3]) {
  const double l1 = fabs(g.L1), l2 = fabs(g.L2), l3 = fabs(g.L3);
  const bool right = g.L1 < 0.0;
  const double x = pb[0] - g.hx, y = pb[1] - g.hy, z = pb[2] - g.hz;
  double d = ik_knee_num(x, y, z, l1, l2, l3) / (2.0 * l2 * l3);
  const bool out = !(d <= 1.0 && d >= -1.0);
  if (d > 1.0) d = 1.0;
  double sc = y * y + z * z - l1 * l1;
  if (sc < 0.0) sc = 0.0;
  const double rt = sqrt(sc);
  q[0] = right ? atan2(z, y) + atan2(rt, -l1) : -(atan2(z, -y) + atan2(rt, -l1));
  q[2] = atan2(-sqrt(1.0 - d * d), d);
  double s3, c3;
  sincos_joint(q[2], &s3, &c3);
  q[1] = -atan2(x, rt) - atan2(l3 * s3, l2 + l3 * c3);
  return out;
}

// g = J^-T tau for the leg Jacobian at t (entries as in swing_pd), with swing_pd's singularity rule: the cofactors over det inside
// lo <= |det| <= 2^52, pinv3_apply on J^T otherwise (returns true: the leg's singular bit).  A NaN determinant takes the closed form.
QC_DEV bool leg_force_from_torque(const LegGeom& lg, const LegTrig& t, const double (&tau)[3], double (&g)[3]) {
  const double L1 = lg.L1, L2 = lg.L2, L3 = lg.L3;
  const double a = L2 * t.c2 + L3 * t.c23, b = L2 * t.s2 + L3 * t.s23;
  const double J[9] = {0.0, a, L3 * t.c23, -L1 * t.s1 - a * t.c1, b * t.s1, L3 * t.s1 * t.s23, L1 * t.c1 - a * t.s1, -b * t.c1, -L3 * t.s23 * t.c1};
  const double c00 = J[4] * J[8] - J[5] * J[7], c01 = J[5] * J[6] - J[3] * J[8], c02 = J[3] * J[7] - J[4] * J[6];
  const double det = J[0] * c00 + J[1] * c01 + J[2] * c02;
  const double ad = fabs(det), lsum = fabs(L1) + fabs(L2) + fabs(L3);
  const double lo = fmax(2.220446049250313e-16, 1.4210854715202004e-14 * lsum * lsum * lsum);
  if (!(ad < lo) && !(ad > 4503599627370496.0)) {
    const double id = 1.0 / det;
    // J^-T = cof(J) / det: row r of the cofactor matrix dotted with tau
    g[0] = id * (c00 * tau[0] + c01 * tau[1] + c02 * tau[2]);
    g[1] = id * ((J[2] * J[7] - J[1] * J[8]) * tau[0] + (J[0] * J[8] - J[2] * J[6]) * tau[1] + (J[1] * J[6] - J[0] * J[7]) * tau[2]);
    g[2] = id * ((J[1] * J[5] - J[2] * J[4]) * tau[0] + (J[2] * J[3] - J[0] * J[5]) * tau[1] + (J[0] * J[4] - J[1] * J[3]) * tau[2]);
    return false;
  }
  const double JT[9] = {J[0], J[3], J[6], J[1], J[4], J[7], J[2], J[5], J[8]};
  pinv3_apply(JT, tau, g);
  return true;
}

__global__ __launch_bounds__(LEG_PLANT_BLOCK) void leg_plant_step_kernel(const DevParams* __restrict__ Pg, const long n, const LegPlantArgs a) {
  const long i = (long)blockIdx.x * LEG_PLANT_BLOCK + threadIdx.x;
  if (i >= n) return;  // tail lanes
  CParams& P = *QC_PARAMS_HERE(Pg);
  double R[9], x[3], v[3], w[3], q[4][3], qd[4][3], tq[4][3];
  load9(a.Rwb, i, R);
  load3(a.x, i, x);
  load3(a.xdot, i, v);
  load3(a.w, i, w);
#pragma unroll
  for (int l = 0; l < 4; l++) {
    load3(a.joint_q, 4 * i + l, q[l]);
    load3(a.joint_qdot, 4 * i + l, qd[l]);
    load3(a.joint_tau, 4 * i + l, tq[l]);
  }
  // (the gather of load_contact_mask, spelled out: through the function this kernel's scalar code came out differently - its pointers
  // are fetched from the kernarg segment up front - and 0.1 to 0.3 us slower at 65 536 and 262 144 robots; this text compiles to the parent's)
  double ph[4] = {0.0, 0.0, 0.0, 0.0};
  if (a.gait_phase && !a.stance) {
#pragma unroll
    for (int l = 0; l < 4; l++) ph[l] = a.gait_phase[4 * i + l];
  }
  const uint32_t sw = a.stance ? *reinterpret_cast<const uint32_t*>(a.stance + 4 * i) : 0u;
  const double duty = a.gait_duty ? a.gait_duty[i] : P.stance_phase;
  const bool running = a.cmd_state ? a.cmd_state[i].gait_running != 0 : true;
  const uint32_t mask = contact_mask(a.stance != nullptr, sw, a.gait_phase != nullptr, ph, duty, running);

  // force pass: net force and moment about the centre of mass (world frame); swing joints integrate
  double fs[3] = {0.0, 0.0, 0.0}, tau[3] = {0.0, 0.0, 0.0};
  double c[4][3];  // x + Rwb FK(q): the pinned contact point of a stance leg
  int flags = 0;
#pragma unroll
  for (int l = 0; l < 4; l++) {
    const LegGeom lg = {P.links[3 * l], P.links[3 * l + 1], P.links[3 * l + 2], P.hip[3 * l], P.hip[3 * l + 1], P.hip[3 * l + 2]};
    const LegTrig t = leg_trig(q[l]);
    double p[3], r[3];
    leg_fk(P, l, t, p);
    mat_vec(R, p, r);
#pragma unroll
    for (int k = 0; k < 3; k++) c[l][k] = x[k] + r[k];
    if (mask & (1u << l)) {
      double g[3], rg[3], f[3], m[3];
      if (leg_force_from_torque(lg, t, tq[l], g)) flags |= 1 << l;
      mat_vec(R, g, rg);
#pragma unroll
      for (int k = 0; k < 3; k++) f[k] = -rg[k];
      cross3(r, f, m);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        fs[k] += f[k];
        tau[k] += m[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 3; k++) {
        qd[l][k] += a.dt * (tq[l][k] / a.leg_inertia[k]);
        q[l][k] += a.dt * qd[l][k];
      }
    }
  }
  double Rn[9];
  rigid_body_step(a, R, x, v, w, fs, tau, Rn);
  // IK pass: the stance feet stay where they were
#pragma unroll
  for (int l = 0; l < 4; l++) {
    if (mask & (1u << l)) {
      const LegGeom lg = {P.links[3 * l], P.links[3 * l + 1], P.links[3 * l + 2], P.hip[3 * l], P.hip[3 * l + 1], P.hip[3 * l + 2]};
      const double d[3] = {c[l][0] - x[0], c[l][1] - x[1], c[l][2] - x[2]};
      double pb[3], qn[3];
      mat_t_vec(Rn, d, pb);
      if (leg_ik(lg, pb, qn)) flags |= 16 << l;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        qd[l][k] = wrap_PI(qn[k] - q[l][k]) / a.dt;
        q[l][k] = qn[k];
      }
    }
  }
  // every input of this robot has been read: the outputs may overwrite them
  {
    double* o = a.Rwb + 9 * i;
#pragma unroll
    for (int k = 0; k < 9; k++) o[k] = Rn[k];
  }
  store3(a.x, i, x);
  store3(a.xdot, i, v);
  store3(a.w, i, w);
#pragma unroll
  for (int l = 0; l < 4; l++) {
    store3(a.joint_q, 4 * i + l, q[l]);
    store3(a.joint_qdot, 4 * i + l, qd[l]);
    if (a.foot_world) store3(a.foot_world, 4 * i + l, c[l]);
  }
  if (a.flags) a.flags[i] = flags;
}

}  // namespace qc
#endif  // __HIPCC__
