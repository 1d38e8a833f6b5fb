// qc_sensitivity_swing.hpp - the reverse pass of the swing legs' PD torques (qc_sensitivity_swing_batch, include/qc_balance.h): the
// link between the leg plant's joint_tau_bar of a swing leg and the tick's inputs, which qc_sensitivity_kin.hpp leaves out.
//
// Per robot and SWING leg l, in the notation of leg_swing_torque / swing_pd (qc_device.hpp), a cotangent of v written vb:
//   forward   p_b = Rwb^T pos - x (sic),  v_b = Rwb^T vel,  q_ref = IK(p_b),  qd = J(q_ref)^-1 v_b,
//             e = wrapPI(wrap2PI(q_ref) - wrap2PI(q)) (slope +1 in q_ref, -1 in q),
//             tau_raw = kp o e + kd o (qd - qdot) + kff, clamped by two compares to [tau_min, tau_max], whatever the QP's status
//   mask      tau_raw from leg_swing_torque ITSELF, the function the tick calls on the same inputs: m_c = !(tau_raw_c < tau_min) &&
//             !(tau_raw_c > tau_max) is the forward pass's bit for bit;  s = m o joint_tau_bar_l
//   joints    joint_q_bar_l = -kp o s (+ joint_q_bar_in_l),  joint_qdot_bar_l = -kd o s
//   gains     gain_bar_l = (s o e, s o (qd - qdot), s): kp, kd, kff
//   velocity  g = J(q_ref)^-T (kd o s) = v_b_bar
//   angles    q_ref_bar = kp o s - (sum_r g_r H_r(q_ref)) qd                  (H_r = d^2 FK_r / dq^2: leg_fk_hessian_apply)
//   position  p_b_bar = J(q_ref)^-T q_ref_bar: inside reach the IK inverts the FK, so dIK / dp = J(q_ref)^-1
//             (tests/test_sensitivity_swing_cpu.py holds that against the 50-digit derivative of the atan2 chain as written)
//   world     swing_pos_bar_l = Rwb p_b_bar,  swing_vel_bar_l = Rwb g
//   robot     Rwb_bar[r][i] += pos_r p_b_bar_i + vel_r g_i (entrywise, row-major),  x_bar -= p_b_bar, summed over the swing legs
// A STANCE leg contributes nothing: its rows are zero (+ joint_q_bar_in).  e and qd are evaluated again here, from the same
// formulas as the forward pass (swing_reference below restates the trig-free chain of leg_swing_torque: the sines and cosines of
// q_ref from the lengths the IK computes, the angles by one atan2 each); only the clamp mask has to be the forward pass's exactly.
//
// UNDEFINED GRADIENTS.  flags bit l: swing leg l's reference is outside the smooth domain of the chain - the knee cosine d >= 1
// (clamped: no slope) or d < -1 (NaN), y^2 + z^2 - l1^2 < 0 (clamped), a target that is not finite (or not after squaring: the
// forward pass's own test), or det J(q_ref) outside swing_pd's closed-form band (the forward pass took the pseudo-inverse, which
// this pass does not differentiate).  A flagged leg has NaN in its rows of the per-leg outputs and, through the sums, in the robot's
// Rwb_bar and x_bar, whatever the mask.  Other non-finite inputs propagate; nothing else is clamped.
// OUT OF SCOPE: the cotangents of the kinematic constants and of tau_min / tau_max; swing_state's planner and the gait clock (the
// call refuses both); commander mode.
//
// Kernel: ONE LANE PER (robot, leg) ROW with a fixed-order quad reduction, not one lane per robot.  The resource file decides it
// (profiles/sensitivity_swing_kernel_resources.txt): the chain of ONE leg - the forward torque for the mask, IK, three atan2, two
// wraps per joint, J^-1 once and J^-T twice, the Hessian - takes 185 VGPRs at 0 B scratch, two waves per SIMD; four of them unrolled
// in one lane would sit where the leg plant adjoint sits (328 registers, one wave per SIMD), and in a batch of mixed contact states
// every leg swings in SOME lane, so a lane per robot walks all four chains anyway.  Per row the same four passes are spread over four times the waves.  The bytes are the siblings': a row
// of an [n][4][3] array is 24 contiguous bytes, a wave's rows 1536; Rwb and x of a robot are read by the four lanes of its quad at
// the same addresses (one request per line).  The two per-robot sums are the only exchange: twelve doubles summed over the quad by
// two butterfly steps, (l0 + l1) + (l2 + l3) in every lane - a fixed order, no atomics, no LDS -, and the quad then stores the
// record in four parts (lane l < 3: row l of Rwb_bar, lane 3: x_bar), each lane having read its part of the `_in` arrays first.
// rows = 4 n and a wave holds 16 whole quads, so a quad is live or dead as one.  FP64, workgroups of one wave, a grid stride once the
// grid is capped, the siblings' tail-lane convention (the index clamped, nothing stored), no scratch.  Templated on the output
// groups - LEG: any of the five per-leg outputs, BODY: Rwb_bar / x_bar - so that an absent group pays neither for its `_in` loads
// nor, for BODY, for the exchange; the six inputs are read by every variant, because the mask and the flags come from the forward
// chain.  Every input of a row is read before any output is written and a lane writes its own part only: an output may be the same
// array as its `_in`.
#pragma once
#include "qc_leg_plant_adjoint.hpp"
#include "qc_sensitivity.hpp"

namespace qc {

struct SensitivitySwingArgs {
  const double *Rwb, *x;                                   // [n][9], [n][3]
  const double *joint_q, *joint_qdot, *swing_pos, *swing_vel;  // [n][4][3]
  const uint8_t* stance;                                   // the contact mask, as qc_sensitivity_kin_batch resolves it: [n][4] bytes, else
  const double* gait_phase;                                // [n][4] the phase rule, else all stance
  const double* gait_duty;                                 // [n] or NULL: the handle's
  const double* joint_tau_bar;                             // [n][4][3]
  const double *joint_q_bar_in, *Rwb_bar_in, *x_bar_in;    // [n][4][3], [n][9], [n][3]: optional
  double *swing_pos_bar, *swing_vel_bar, *joint_q_bar, *joint_qdot_bar;  // [n][4][3] each, optional OUT
  double* gain_bar;                                        // [n][4][9] optional OUT
  double *Rwb_bar, *x_bar;                                 // [n][9], [n][3] optional OUT
  int32_t* flags;                                          // [n] optional OUT
};

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

// The reference angles of a swing leg and their sines and cosines, as the trig-free path of leg_swing_torque forms them from the
// body-frame target pb.  Returns true when pb is outside the smooth domain of legInverseKinematics (the first three flag conditions
// above); t and qr are then not to be used.
QC_DEV bool swing_reference(const LegGeom& g, const double (&pb)[3], LegTrig& t, double (&qr)[3]) {
  const double l1 = fabs(g.L1), l2 = fabs(g.L2), l3 = fabs(g.L3);
  const bool right = g.L1 < 0.0;
  const double x = pb[0] - g.hx, y = pb[1] - g.hy, z = pb[2] - g.hz;
  const double num = ik_knee_num(x, y, z, l1, l2, l3);
  double sc = y * y + z * z - l1 * l1;
  const bool inside = sc < 0.0;
  if (inside) sc = 0.0;
  const double rho2 = y * y + z * z;
  const double rt2 = sc;
  const double sig2 = x * x + rt2;
  const bool finite = (__builtin_fma(num, 0.0, __builtin_fma(sig2, 0.0, rho2 * 0.0)) == 0.0);
  const double d = num / (2.0 * l2 * l3);
  const bool out = !finite || inside || !(d < 1.0) || !(d >= -1.0);
  const double u = __builtin_fma(-d, d, 1.0);
  const double s3 = u == 0.0 ? -0.0 : -(u * rsqrt_nr(u)), c3 = d;
  const double rt = rt2 == 0.0 ? 0.0 : rt2 * rsqrt_nr(rt2);
  const double ir = rsqrt_nr(rho2);
  const double ib = rsqrt_nr(rt2 + l1 * l1);
  const double is = rsqrt_nr(sig2);
  const double kx = __builtin_fma(l3, c3, l2), ky = l3 * s3;
  const double k2 = kx * kx + ky * ky;
  const double ik = rsqrt_nr(k2);
  const double cA = (right ? y : -y) * ir, sA = z * ir;
  const double cB = -l1 * ib, sB = rt * ib;
  const double sAB = sA * cB + cA * sB, cAB = cA * cB - sA * sB;
  const double cC = rt * is, sC = x * is;
  const double cD = k2 > 0.0 ? kx * ik : 1.0, sD = k2 > 0.0 ? ky * ik : 0.0;
  const double sCD = sC * cD + cC * sD, cCD = cC * cD - sC * sD;
  t.s1 = right ? sAB : -sAB; t.c1 = cAB;
  t.s2 = -sCD; t.c2 = cCD;
  t.s23 = t.s2 * c3 + t.c2 * s3;
  t.c23 = t.c2 * c3 - t.s2 * s3;
  qr[0] = atan2(t.s1, t.c1);
  qr[1] = atan2(t.s2, t.c2);
  qr[2] = atan2(s3, c3);
  return out;
}

// The cofactors of the leg Jacobian at t (row-major: cof[3 r + k] belongs to J[r][k]) and 1 / det: J^-1 and J^-T from one set.
// Returns true when det is outside swing_pd's closed-form band (a NaN determinant is inside, as there).
struct LegJacobianInverse {
  double cof[9], id;
};
QC_DEV bool leg_jacobian_inverse(const LegGeom& lg, const LegTrig& t, LegJacobianInverse& I) {
  const double L1 = lg.L1, L2 = lg.L2, L3 = lg.L3;
  const double a = L2 * t.c2 + L3 * t.c23, b = L2 * t.s2 + L3 * t.s23;
  const double J[9] = {0.0, a, L3 * t.c23, -L1 * t.s1 - a * t.c1, b * t.s1, L3 * t.s1 * t.s23, L1 * t.c1 - a * t.s1, -b * t.c1, -L3 * t.s23 * t.c1};
  I.cof[0] = J[4] * J[8] - J[5] * J[7]; I.cof[1] = J[5] * J[6] - J[3] * J[8]; I.cof[2] = J[3] * J[7] - J[4] * J[6];
  I.cof[3] = J[2] * J[7] - J[1] * J[8]; I.cof[4] = J[0] * J[8] - J[2] * J[6]; I.cof[5] = J[1] * J[6] - J[0] * J[7];
  I.cof[6] = J[1] * J[5] - J[2] * J[4]; I.cof[7] = J[2] * J[3] - J[0] * J[5]; I.cof[8] = J[0] * J[4] - J[1] * J[3];
  const double det = J[0] * I.cof[0] + J[1] * I.cof[1] + J[2] * I.cof[2];
  const double ad = fabs(det), lsum = fabs(L1) + fabs(L2) + fabs(L3);
  const double lo = fmax(2.220446049250313e-16, 1.4210854715202004e-14 * lsum * lsum * lsum);
  I.id = 1.0 / det;
  return (ad < lo) || (ad > 4503599627370496.0);
}
// o = J^-1 v: column k of the cofactor matrix dotted with v
QC_DEV void jacobian_inverse_apply(const LegJacobianInverse& I, const double (&v)[3], double (&o)[3]) {
#pragma unroll
  for (int k = 0; k < 3; k++) o[k] = I.id * (I.cof[k] * v[0] + I.cof[3 + k] * v[1] + I.cof[6 + k] * v[2]);
}
// o = J^-T v: row r of the cofactor matrix dotted with v
QC_DEV void jacobian_inverse_t_apply(const LegJacobianInverse& I, const double (&v)[3], double (&o)[3]) {
#pragma unroll
  for (int r = 0; r < 3; r++) o[r] = I.id * (I.cof[3 * r] * v[0] + I.cof[3 * r + 1] * v[1] + I.cof[3 * r + 2] * v[2]);
}

// the sum of v over the four lanes of a quad, (l0 + l1) + (l2 + l3) in every lane
QC_DEV double quad_sum(double v) {
  v += __shfl_xor(v, 1);
  return v + __shfl_xor(v, 2);
}

template <bool LEG, bool BODY>
__global__ __launch_bounds__(SENSITIVITY_BLOCK) void sensitivity_swing_kernel(const DevParams* __restrict__ Pg, const long rows, const SensitivitySwingArgs a) {
  for (long base = (long)blockIdx.x * SENSITIVITY_BLOCK; base < rows; base += (long)gridDim.x * SENSITIVITY_BLOCK) {
    const long me = base + threadIdx.x;
    const bool live = me < rows;
    const long i = live ? me : rows - 1;  // tail lanes: the last row again, nothing stored
    const long rb = i >> 2;               // the robot
    const int leg = (int)(i & 3);
    CParams& P = *QC_PARAMS_HERE(Pg);
    double R[9], x[3], pos[3], vel[3], q[3], qdot[3], s[3];
    load9(a.Rwb, rb, R);
    load3(a.x, rb, x);
    load3(a.swing_pos, i, pos);
    load3(a.swing_vel, i, vel);
    load3(a.joint_q, i, q);
    load3(a.joint_qdot, i, qdot);
    load3(a.joint_tau_bar, i, s);
    bool swing;
    if (a.stance) swing = a.stance[i] == 0;
    else if (!a.gait_phase) swing = false;
    else swing = !phase_in_stance(a.gait_phase[i], a.gait_duty ? a.gait_duty[rb] : P.stance_phase);
    double gq[3] = {0.0, 0.0, 0.0}, part[3] = {0.0, 0.0, 0.0};  // part: this lane's quarter of the robot's record (Rwb_bar | x_bar)
    if (LEG && a.joint_q_bar_in) load3(a.joint_q_bar_in, i, gq);
    if constexpr (BODY) {
      if (leg < 3) {
        if (a.Rwb_bar_in) load3(a.Rwb_bar_in, 3 * rb + leg, part);
      } else if (a.x_bar_in) {
        load3(a.x_bar_in, rb, part);
      }
    }
    double pw[3] = {0.0, 0.0, 0.0}, vw[3] = {0.0, 0.0, 0.0}, gqd[3] = {0.0, 0.0, 0.0};
    double gain[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double Rc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, xc[3] = {0.0, 0.0, 0.0};
    bool flag = false;
    if (swing) {
      const LegGeom lg = leg_geom(P, leg);
      double pb[3], vb[3], tau[3];
#pragma unroll
      for (int r = 0; r < 3; r++) {
        pb[r] = R[r] * pos[0] + R[3 + r] * pos[1] + R[6 + r] * pos[2] - x[r];  // as swing_leg_task forms them
        vb[r] = R[r] * vel[0] + R[3 + r] * vel[1] + R[6 + r] * vel[2];
      }
      leg_swing_torque(P, lg, pb, vb, q, qdot, tau);  // tau_raw, as the forward pass evaluates it
#pragma unroll
      for (int c = 0; c < 3; c++) s[c] = (!(tau[c] < P.tau_min) && !(tau[c] > P.tau_max)) ? s[c] : 0.0;
      LegTrig t;
      LegJacobianInverse I;
      double qr[3], qd[3], ks[3], g[3], hq[3], qrb[3], pbb[3];
      flag = swing_reference(lg, pb, t, qr);
      if (leg_jacobian_inverse(lg, t, I)) flag = true;
      jacobian_inverse_apply(I, vb, qd);
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const double e = wrap_PI(wrap_2PI(qr[c]) - wrap_2PI(q[c]));
        gain[c] = s[c] * e;
        gain[3 + c] = s[c] * (qd[c] - qdot[c]);
        gain[6 + c] = s[c];
        ks[c] = P.jc_kd[c] * s[c];
        gq[c] -= P.jc_kp[c] * s[c];
        gqd[c] = -ks[c];
      }
      jacobian_inverse_t_apply(I, ks, g);
      leg_fk_hessian_apply(lg, t, g, qd, hq);
#pragma unroll
      for (int c = 0; c < 3; c++) qrb[c] = P.jc_kp[c] * s[c] - hq[c];
      jacobian_inverse_t_apply(I, qrb, pbb);
      mat_vec(R, pbb, pw);
      mat_vec(R, g, vw);
#pragma unroll
      for (int r = 0; r < 3; r++) {
        xc[r] = -pbb[r];
#pragma unroll
        for (int k = 0; k < 3; k++) Rc[3 * r + k] = pos[r] * pbb[k] + vel[r] * g[k];
      }
      if (flag) {  // no gradient: the leg's rows and, through the sums, the robot's record
        const double nan = __builtin_nan("");
#pragma unroll
        for (int k = 0; k < 3; k++) pw[k] = vw[k] = gq[k] = gqd[k] = xc[k] = nan;
#pragma unroll
        for (int k = 0; k < 9; k++) gain[k] = Rc[k] = nan;
      }
    }
    if constexpr (BODY) {
      // the robot's sums, then this lane's quarter of them
#pragma unroll
      for (int k = 0; k < 9; k++) Rc[k] = quad_sum(Rc[k]);
#pragma unroll
      for (int k = 0; k < 3; k++) xc[k] = quad_sum(xc[k]);
#pragma unroll
      for (int k = 0; k < 3; k++) part[k] += leg == 0 ? Rc[k] : (leg == 1 ? Rc[3 + k] : (leg == 2 ? Rc[6 + k] : xc[k]));
    }
    int fl = flag ? (1 << leg) : 0;
    if (a.flags) {  // (wave-uniform)
      fl |= __shfl_xor(fl, 1);
      fl |= __shfl_xor(fl, 2);
    }
    if (live) {
      if constexpr (LEG) {
        if (a.swing_pos_bar) store3(a.swing_pos_bar, i, pw);
        if (a.swing_vel_bar) store3(a.swing_vel_bar, i, vw);
        if (a.joint_q_bar) store3(a.joint_q_bar, i, gq);
        if (a.joint_qdot_bar) store3(a.joint_qdot_bar, i, gqd);
        if (a.gain_bar) {
          double* o = a.gain_bar + 9 * i;
#pragma unroll
          for (int k = 0; k < 9; k++) o[k] = gain[k];
        }
      }
      if constexpr (BODY) {
        if (leg < 3) {
          if (a.Rwb_bar) store3(a.Rwb_bar, 3 * rb + leg, part);
        } else if (a.x_bar) {
          store3(a.x_bar, rb, part);
        }
      }
      if (a.flags && leg == 0) a.flags[rb] = fl;
    }
  }
}

}  // namespace qc
#endif  // __HIPCC__
