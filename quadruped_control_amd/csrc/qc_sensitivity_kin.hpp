// qc_sensitivity_kin.hpp - the two ends of the fused tick's reverse pass (qc_sensitivity_kin_batch, include/qc_balance.h): the
// cotangent of joint_q through the forward kinematics, and the reverse pass of the clamped J^T torque map.  A small kernel in front
// of and behind the adjoint: it reads joint_q and the contact mask of the BatchIn the tick read - none of the state arrays -, the
// forces, the status and the cotangents, and repeats no solve.
//
// Per robot and leg l, with q = joint_q_l, t = leg_trig(q), p = leg_fk, J[r][c] = d p_r / d q_c (the nine entries leg_jt_force
// spells out: the exact Jacobian of leg_fk), g = grf_body_l, H_r = d^2 p_r / d q^2 (symmetric):
//   forward          tau_raw = J^T g, tau = tau_raw clamped by two compares to [tau_min, tau_max] (store_tau), emitted for a stance
//                    leg of a robot with status 0, 0 otherwise
//   mask             m_c = 1 where !(tau_raw_c < tau_min) && !(tau_raw_c > tau_max): equality passes, a NaN passes and propagates;
//                    m = 0 for a swing leg and for a robot with status != 0;  s = m o joint_tau_bar_l
//   the forces       grf_bar_l = grf_bar_in_l + J s                                  (body frame: what qc_sensitivity_batch takes)
//   the angles       joint_q_bar_l = joint_q_bar_in_l + G s + J^T feet_bar_l,  G = sum_r g_r H_r
// With a = l2 c2 + l3 c23, b = l2 s2 + l3 s23, d = l3 c23, e = l3 s23, u = g1 c1 + g2 s1, v = g1 s1 - g2 c1 the six entries of G are
//   G00 = a v - l1 u,  G01 = b u,  G02 = e u,  G11 = a v - g0 b,  G12 = G22 = d v - g0 e.
// The J^T feet_bar term is UNMASKED: a swing leg's feet_bar from the QP is zero already, and a caller's own loss on a foot position
// must pass.  A missing optional input counts as zero.  Non-finite inputs propagate; nothing is clamped.
// OUT OF SCOPE: the swing legs' PD torques (with swing references the joint_tau_bar of a swing leg is ignored), commander mode, and
// the cotangents of the kinematic constants and of tau_min / tau_max.
//
// Kernel: the legs are independent here, so one lane per (robot, leg) ROW, not per robot: a row of an [n][4][3] array is 24
// contiguous bytes, a wave's rows 1536 contiguous bytes (every byte of every line it touches is used; a row is 8-byte aligned
// only, so the loads are 8-byte ones), status and the mask byte are indexed by row >> 2 and row & 3, the leg's constants come
// through leg_geom.  FP64, workgroups of one wave, a grid stride once the grid is capped, the siblings' tail-lane convention (the
// index clamped, nothing stored).  No LDS, no scratch.  Templated on the halves present - TAU: joint_tau_bar, FK: feet_bar -, so
// that neither pays for the other's loads; grf_bar_in and joint_q_bar_in are wave-uniform branches.  Every input of a row is read
// before any output of it is written and a lane touches its own row only: an output may be the same array as its `_in`.
#pragma once
#include "qc_sensitivity.hpp"

namespace qc {

struct SensitivityKinArgs {
  const double* joint_q;        // [n][4][3]
  const uint8_t* stance;        // the contact mask, as qc_certify_batch resolves it: [n][4] bytes, else
  const double* gait_phase;     // [n][4] the phase rule, else all stance
  const double* gait_duty;      // [n] or NULL: the handle's
  const double* grf_body;       // [n][4][3]
  const int32_t* status;        // [n]
  const double *joint_tau_bar, *feet_bar, *grf_bar_in, *joint_q_bar_in;  // [n][4][3] each, optional
  double *grf_bar, *joint_q_bar;                                         // [n][4][3] each, optional OUT
};

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

// one leg's bit of the contact mask (contact_mask's rule on a single byte or phase)
QC_DEV bool leg_in_stance(CParams* P, const SensitivityKinArgs& a, long row) {
  if (a.stance) return a.stance[row] != 0;
  if (!a.gait_phase) return true;
  const double duty = a.gait_duty ? a.gait_duty[row >> 2] : P->stance_phase;
  return phase_in_stance(a.gait_phase[row], duty);
}

template <bool TAU, bool FK>
__global__ __launch_bounds__(SENSITIVITY_BLOCK) void sensitivity_kin_kernel(const DevParams* __restrict__ Pg, const long rows, const SensitivityKinArgs a) {
  for (long base = (long)blockIdx.x * SENSITIVITY_BLOCK; base < rows; base += (long)gridDim.x * SENSITIVITY_BLOCK) {
    const long me = base + threadIdx.x;
    const bool live = me < rows;
    const long i = live ? me : rows - 1;  // tail lanes: the last row again, nothing stored
    CParams& P = *QC_PARAMS_HERE(Pg);
    double gq[3] = {0.0, 0.0, 0.0}, gg[3] = {0.0, 0.0, 0.0};
    if (a.joint_q_bar_in) load3(a.joint_q_bar_in, i, gq);
    if (TAU && a.grf_bar_in) load3(a.grf_bar_in, i, gg);
    if constexpr (TAU || FK) {
      double q[3];
      load3(a.joint_q, i, q);
      const LegGeom lg = leg_geom(P, (int)(i & 3));
      const LegTrig t = leg_trig(q);
      if constexpr (TAU) {
        double g[3], s[3], tau[3];
        load3(a.grf_body, i, g);
        load3(a.joint_tau_bar, i, s);
        const bool emit = a.status[i >> 2] == 0 && leg_in_stance(&P, a, i);
        leg_jt_force(lg, t, g, tau);  // tau_raw, as the forward pass evaluates it
#pragma unroll
        for (int c = 0; c < 3; c++) s[c] = (emit && !(tau[c] < P.tau_min) && !(tau[c] > P.tau_max)) ? s[c] : 0.0;
        const double ja = lg.L2 * t.c2 + lg.L3 * t.c23, jb = lg.L2 * t.s2 + lg.L3 * t.s23;
        const double jd = lg.L3 * t.c23, je = lg.L3 * t.s23;
        // J s
        gg[0] += ja * s[1] + jd * s[2];
        gg[1] += (-lg.L1 * t.s1 - ja * t.c1) * s[0] + (jb * t.s1) * s[1] + (je * t.s1) * s[2];
        gg[2] += (lg.L1 * t.c1 - ja * t.s1) * s[0] + (-jb * t.c1) * s[1] + (-je * t.c1) * s[2];
        // G s
        const double u = g[1] * t.c1 + g[2] * t.s1, v = g[1] * t.s1 - g[2] * t.c1;
        const double G00 = ja * v - lg.L1 * u, G01 = jb * u, G02 = je * u, G11 = ja * v - g[0] * jb, G12 = jd * v - g[0] * je;
        gq[0] += G00 * s[0] + G01 * s[1] + G02 * s[2];
        gq[1] += G01 * s[0] + G11 * s[1] + G12 * s[2];
        gq[2] += G02 * s[0] + G12 * s[1] + G12 * s[2];
      }
      if constexpr (FK) {
        double fb[3], jt[3];
        load3(a.feet_bar, i, fb);
        leg_jt_force(lg, t, fb, jt);  // J^T feet_bar, unmasked
#pragma unroll
        for (int c = 0; c < 3; c++) gq[c] += jt[c];
      }
    }
    if (live) {
      if (TAU && a.grf_bar) store3(a.grf_bar, i, gg);
      if (a.joint_q_bar) store3(a.joint_q_bar, i, gq);
    }
  }
}

}  // namespace qc
#endif  // __HIPCC__
