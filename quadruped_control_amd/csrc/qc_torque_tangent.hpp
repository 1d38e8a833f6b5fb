// qc_torque_tangent.hpp - forward mode of the clamped J^T torque map: qc_torque_tangent_batch (include/qc_tangent.h), the kernel
// between qc_tangent_batch and qc_leg_plant_step_tangent_batch in the forward-mode loop around the tick.  It is the map
// qc_sensitivity_kin.hpp transposes: per (direction, robot, leg), with q = joint_q_l, t = leg_trig(q), J the leg Jacobian,
// g = grf_body_l, tau_raw = J^T g, G = sum_r g_r H_r (the six entries of qc_sensitivity_kin.hpp, leg_fk_hessian_apply),
//   joint_tau_tan_l = m o ( J^T grf_tan_l + G joint_q_tan_l )
// m_c = 1 where !(tau_raw_c < tau_min) && !(tau_raw_c > tau_max) - equality passes, a NaN passes and propagates -, m = 0 for a swing
// leg and for a robot with status != 0: exactly that kernel's mask, the contact mask resolved by its rule (stance bytes, else the
// phase rule, else all stance).  A masked entry is exactly 0 whatever the tangents hold.
// A swing leg's row is exactly 0: its PD torque has its own kernel (qc_swing_tangent.hpp), chained in place behind this one.
// OUT OF SCOPE: tangents of the kinematic constants and of tau_min / tau_max.
//
// Kernel: one lane per (direction, robot, leg) ROW, the (robot, leg) row fastest - row j = k 4n + r is row j of a [K][n][4][3]
// array -, as qc_sensitivity_kin.hpp is one lane per (robot, leg): a wave's loads of one direction are contiguous, and K multiplies
// the parallelism.  grf_body, joint_q, status and the mask are re-read per direction (from L2), the trigonometry recomputed: three
// sincos_joint per row, nothing to share across directions that is worth a second pass.  FP64, workgroups of one wave, a grid
// stride once the grid is capped (TORQUE_TANGENT_MAX_BLOCKS), no LDS, no scratch.  A NULL tangent is zero.  A row reads all of its
// inputs before it writes and touches only its own row: joint_tau_tan may be grf_tan or joint_q_tan.
#pragma once
#include "qc_leg_plant_adjoint.hpp"  // leg_fk_hessian_apply, load3_or_zero

namespace qc {

struct TorqueTangentArgs {
  const double* joint_q;        // [n][4][3]
  const uint8_t* stance;        // the contact mask, as qc_certify_batch resolves it: [n][4] bytes, else
  const double* gait_phase;     // [n][4] the phase rule, else all stance
  const double* gait_duty;      // [n] or NULL: the handle's
  const double* grf_body;       // [n][4][3]
  const int32_t* status;        // [n]
  long n_dir;                   // K
  const double *grf_tan, *joint_q_tan;  // [K][n][4][3], nullptr: zero
  double* joint_tau_tan;                // [K][n][4][3] OUT
};

constexpr int TORQUE_TANGENT_BLOCK = 64;  // one wave
constexpr int TORQUE_TANGENT_MAX_BLOCKS = 4096;

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

__global__ __launch_bounds__(TORQUE_TANGENT_BLOCK) void torque_tangent_kernel(const DevParams* __restrict__ Pg, const long rows, const TorqueTangentArgs a) {
  const long total = rows * a.n_dir;
  for (long j = (long)blockIdx.x * TORQUE_TANGENT_BLOCK + threadIdx.x; j < total; j += (long)gridDim.x * TORQUE_TANGENT_BLOCK) {
    const long i = j % rows;  // the (robot, leg) row; j itself is the row of direction k = j / rows in a [K][n][4][3] array
    CParams& P = *QC_PARAMS_HERE(Pg);
    double q[3], g[3], dg[3], dq[3];
    load3(a.joint_q, i, q);
    load3(a.grf_body, i, g);
    load3_or_zero(a.grf_tan, j, dg);
    load3_or_zero(a.joint_q_tan, j, dq);
    // one leg's bit of the contact mask (leg_in_stance's rule, qc_sensitivity_kin.hpp)
    bool stance = true;
    if (a.stance) stance = a.stance[i] != 0;
    else if (a.gait_phase) stance = phase_in_stance(a.gait_phase[i], a.gait_duty ? a.gait_duty[i >> 2] : P.stance_phase);
    const bool emit = a.status[i >> 2] == 0 && stance;
    const LegGeom lg = leg_geom(P, (int)(i & 3));
    const LegTrig t = leg_trig(q);
    double tau[3], jt[3], gy[3], o[3];
    leg_jt_force(lg, t, g, tau);  // tau_raw, as the forward pass evaluates it
    leg_jt_force(lg, t, dg, jt);  // J^T grf_tan
    leg_fk_hessian_apply(lg, t, g, dq, gy);  // G joint_q_tan
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = (emit && !(tau[c] < P.tau_min) && !(tau[c] > P.tau_max)) ? jt[c] + gy[c] : 0.0;
    store3(a.joint_tau_tan, j, o);
  }
}

}  // namespace qc
#endif  // __HIPCC__
