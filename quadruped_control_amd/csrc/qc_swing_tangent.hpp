// qc_swing_tangent.hpp - forward mode of the swing legs' PD torques: qc_swing_torque_tangent_batch (include/qc_tangent.h), the kernel
// chained IN PLACE behind qc_torque_tangent_batch (which writes exact zeros in the swing rows) so that joint_tau_tan is the tangent
// of the tick's complete joint_tau.  It is the map qc_sensitivity_swing.hpp transposes: per (direction, robot, SWING leg), in that
// header's notation (p_b = Rwb^T pos - x (sic), v_b = Rwb^T vel, q_ref = IK(p_b), qd = J(q_ref)^-1 v_b, H_r = d^2 FK_r / dq^2 at
// q_ref), with delta the world-frame left tangent of Rwb (Rwb <- exp([delta]x) Rwb):
//   dp_b   = Rwb^T (dpos - delta x pos) - dx
//   dv_b   = Rwb^T (dvel - delta x vel)
//   dq_ref = J(q_ref)^-1 dp_b                      inside reach the IK inverts the FK
//   dqd    = J(q_ref)^-1 (dv_b - B),  B_r = dq_ref^T H_r qd
//   dtau   = m o ( kp o (dq_ref - dq) + kd o (dqd - dqdot) ) + joint_tau_tan_in
// m is the adjoint's mask: tau_raw from leg_swing_torque ITSELF on the same inputs, m_c = !(tau_raw_c < tau_min) && !(tau_raw_c >
// tau_max), the forward tick's bit for bit; the wraps have slope 1; the QP's status plays no part.  A STANCE leg's row is
// joint_tau_tan_in (0 where that is NULL).  flags bit l: swing leg l is outside the smooth domain of the chain, by the adjoint's
// rules and its device functions (swing_reference, leg_jacobian_inverse); a flagged leg's row is NaN in every direction, whatever the
// mask and joint_tau_tan_in, the other legs of the robot are untouched.  Other non-finite inputs propagate; nothing else is clamped.
// OUT OF SCOPE: tangents of the gains, of tau_min / tau_max and of the kinematic constants; swing_state's planner and the gait clock
// (the call refuses both); commander mode.
//
// Kernel: one lane per (direction, robot, leg) ROW, the (robot, leg) row fastest - row j = k 4n + r is row j of a [K][n][4][3]
// array -, torque_tangent_kernel's layout.  The forward chain (the torque for the mask, IK, three atan2, J^-1) does not depend on the
// direction and is RECOMPUTED per direction: that buys a K-fold parallelism at small n (4 096 robots at K = 12 fill 3 072 waves
// where a direction loop inside a lane would fill 256) for arithmetic the adjoint's layout pays anyway, and keeps one leg's chain -
// not K tangents beside it - in the registers.  profiles/swing_tangent_kernel_resources.txt holds the registers and the scratch,
// profiles/swing_tangent.md the time at K = 1 against K = 12.  The vector B comes from leg_fk_hessian_apply on the three unit vectors
// (the compiler folds the zeros).  The robot's flag word is the OR over its quad, written once by leg 0 of direction 0: 4 n is a
// multiple of 4, so quads stay whole in a wave and are live or dead as one.  FP64, workgroups of one wave, a grid stride once the grid
// is capped (SWING_TANGENT_MAX_BLOCKS), the siblings' tail-lane convention (the index clamped, nothing stored), no LDS, no scratch.
// A NULL tangent is zero.  A row reads all of its inputs before it writes and touches only its own row: joint_tau_tan may be
// joint_tau_tan_in or any other [K][n][4][3] input tangent.
#pragma once
#include "qc_sensitivity_swing.hpp"  // swing_reference, leg_jacobian_inverse, jacobian_inverse_apply; leg_fk_hessian_apply, load3_or_zero

namespace qc {

struct SwingTangentArgs {
  const double *Rwb, *x;                                       // [n][9], [n][3]
  const double *joint_q, *joint_qdot, *swing_pos, *swing_vel;  // [n][4][3]
  const uint8_t* stance;                                       // the contact mask, as qc_sensitivity_swing_batch resolves it: [n][4] bytes, else
  const double* gait_phase;                                    // [n][4] the phase rule, else all stance
  const double* gait_duty;                                     // [n] or NULL: the handle's
  long n_dir;                                                  // K (1 for a call that asks for the flags alone)
  const double *Rwb_rot_tan, *x_tan;                           // [K][n][3], nullptr: zero
  const double *swing_pos_tan, *swing_vel_tan, *joint_q_tan, *joint_qdot_tan, *joint_tau_tan_in;  // [K][n][4][3], nullptr: zero
  double* joint_tau_tan;                                       // [K][n][4][3] optional OUT
  int32_t* flags;                                              // [n] optional OUT
};

constexpr int SWING_TANGENT_BLOCK = 64;  // one wave
constexpr int SWING_TANGENT_MAX_BLOCKS = 4096;

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

// o = R^T (d - delta x p): a world-frame tangent of a point p under the left tangent delta of R, brought into the body frame
QC_DEV void body_frame_tangent(const double (&R)[9], const double (&delta)[3], const double (&p)[3], const double (&d)[3], double (&o)[3]) {
  const double a[3] = {d[0] - (delta[1] * p[2] - delta[2] * p[1]), d[1] - (delta[2] * p[0] - delta[0] * p[2]), d[2] - (delta[0] * p[1] - delta[1] * p[0])};
#pragma unroll
  for (int r = 0; r < 3; r++) o[r] = R[r] * a[0] + R[3 + r] * a[1] + R[6 + r] * a[2];
}

// B_r = a^T H_r y, r = 0..2: leg_fk_hessian_apply on the unit vectors
QC_DEV void leg_fk_hessian_bilinear(const LegGeom& lg, const LegTrig& t, const double (&a)[3], const double (&y)[3], double (&B)[3]) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const double e[3] = {r == 0 ? 1.0 : 0.0, r == 1 ? 1.0 : 0.0, r == 2 ? 1.0 : 0.0};
    double h[3];
    leg_fk_hessian_apply(lg, t, e, y, h);
    B[r] = a[0] * h[0] + a[1] * h[1] + a[2] * h[2];
  }
}

__global__ __launch_bounds__(SWING_TANGENT_BLOCK) void swing_tangent_kernel(const DevParams* __restrict__ Pg, const long rows, const SwingTangentArgs a) {
  const long total = rows * a.n_dir;
  for (long base = (long)blockIdx.x * SWING_TANGENT_BLOCK; base < total; base += (long)gridDim.x * SWING_TANGENT_BLOCK) {
    const long me = base + threadIdx.x;
    const bool live = me < total;
    const long j = live ? me : total - 1;  // tail lanes: the last row again, nothing stored
    const long k = j / rows, i = j - k * rows;  // the direction and the (robot, leg) row
    const long rb = i >> 2;                     // the robot
    const long rk = k * (rows >> 2) + rb;       // its row in a [K][n][3] array
    const int leg = (int)(i & 3);
    CParams& P = *QC_PARAMS_HERE(Pg);
    double o[3];
    load3_or_zero(a.joint_tau_tan_in, j, o);
    bool swing;  // (qc_sensitivity_swing.hpp's rule)
    if (a.stance) swing = a.stance[i] == 0;
    else if (!a.gait_phase) swing = false;
    else swing = !phase_in_stance(a.gait_phase[i], a.gait_duty ? a.gait_duty[rb] : P.stance_phase);
    bool flag = false;
    if (swing) {
      double R[9], x[3], pos[3], vel[3], q[3], qdot[3];
      load9(a.Rwb, rb, R);
      load3(a.x, rb, x);
      load3(a.swing_pos, i, pos);
      load3(a.swing_vel, i, vel);
      load3(a.joint_q, i, q);
      load3(a.joint_qdot, i, qdot);
      double delta[3], dx[3], dpos[3], dvel[3], dq[3], dqdot[3];
      load3_or_zero(a.Rwb_rot_tan, rk, delta);
      load3_or_zero(a.x_tan, rk, dx);
      load3_or_zero(a.swing_pos_tan, j, dpos);
      load3_or_zero(a.swing_vel_tan, j, dvel);
      load3_or_zero(a.joint_q_tan, j, dq);
      load3_or_zero(a.joint_qdot_tan, j, dqdot);
      const LegGeom lg = leg_geom(P, leg);
      double pb[3], vb[3], tau[3];
#pragma unroll
      for (int r = 0; r < 3; r++) {
        pb[r] = R[r] * pos[0] + R[3 + r] * pos[1] + R[6 + r] * pos[2] - x[r];  // as swing_leg_task forms them
        vb[r] = R[r] * vel[0] + R[3 + r] * vel[1] + R[6 + r] * vel[2];
      }
      leg_swing_torque(P, lg, pb, vb, q, qdot, tau);  // tau_raw, as the forward pass evaluates it
      LegTrig t;
      LegJacobianInverse I;
      double qr[3], qd[3], dpb[3], dvb[3], dqr[3], B[3], dqd[3];
      flag = swing_reference(lg, pb, t, qr);
      if (leg_jacobian_inverse(lg, t, I)) flag = true;
      jacobian_inverse_apply(I, vb, qd);
      body_frame_tangent(R, delta, pos, dpos, dpb);
      body_frame_tangent(R, delta, vel, dvel, dvb);
#pragma unroll
      for (int r = 0; r < 3; r++) dpb[r] -= dx[r];
      jacobian_inverse_apply(I, dpb, dqr);
      leg_fk_hessian_bilinear(lg, t, dqr, qd, B);
#pragma unroll
      for (int r = 0; r < 3; r++) dvb[r] -= B[r];
      jacobian_inverse_apply(I, dvb, dqd);
      const double nan = __builtin_nan("");
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const double d = P.jc_kp[c] * (dqr[c] - dq[c]) + P.jc_kd[c] * (dqd[c] - dqdot[c]);
        if (!(tau[c] < P.tau_min) && !(tau[c] > P.tau_max)) o[c] = d + o[c];
        if (flag) o[c] = nan;  // no derivative: the leg's row, whatever the mask
      }
    }
    int fl = flag ? (1 << leg) : 0;
    if (a.flags) {  // (wave-uniform)
      fl |= __shfl_xor(fl, 1);
      fl |= __shfl_xor(fl, 2);
    }
    if (live) {
      if (a.joint_tau_tan) store3(a.joint_tau_tan, j, o);
      if (a.flags && k == 0 && leg == 0) a.flags[rb] = fl;
    }
  }
}

}  // namespace qc
#endif  // __HIPCC__
