// qc_swing_reference.hpp - the front half of the tick as a launch of its own (qc_swing_reference_batch, include/qc_balance.h) and its
// reverse pass (qc_swing_reference_adjoint_batch): the gait clock, the contact mask, the foothold planner and the sextic swing
// trajectory - the stage every other differentiable entry point refuses by name.
//
// FORWARD, per robot, what the tick does before the QP when swing_state is given, in its order and with ITS device functions
// (qc_device.hpp: gait_clock_step / advance_phase, contact_mask, leg_replans, leg_fk, plan_foothold, track_swing; the lever arm r =
// Rwb FK(q) by mat_vec, the expression wrench_from_state writes):
//   clock     gait_dt given: the four phases advance and are written back to gait_phase
//   mask      `stance` bytes, else the phase rule on the advanced phases (gait_duty or the handle's value)
//   plan      leg l is replanned on a stance -> swing edge, or whenever it swings on the first call (leg_state = -1):
//             p_start_l = r_l + x, p_final_l = plan_foothold(...); if ANY leg is replanned every other leg's has_traj is cleared
//             (FootTrajectoryManager::referenceStates), else has_traj is kept; leg_state = the mask
//   track     swing leg with a trajectory: (swing_pos_l, swing_vel_l) = track_swing(phase_l, p_start_l, p_final_l); every other leg: zeros
// `planned` bit l: leg l was replanned by this call.  The values are the tick's bit for bit (tests/test_gpu_swing_reference.py).
//
// REVERSE.  Nothing is saved by the forward launch: the caller passes `in` with gait_phase as the forward call left it and the records
// from BEFORE it (state_before), from whose leg_state / has_traj and the mask the plan decision is recomputed.  A cotangent of v is vb.
// Per leg l, with (h, h') = swing_basis(phase_l) - track_swing's own loop - if the leg swings and has a trajectory after the call,
// else zero:
//   a_r = (h0 + h2 / 2) pos_bar_r + (h0' + h2' / 2) vel_bar_r,  c_r = (h1 + h2 / 2) pos_bar_r + (h1' + h2' / 2) vel_bar_r      r = 0, 1
//   a_2 = h0 pos_bar_2 + h0' vel_bar_2,                         c_2 = h1 pos_bar_2 + h1' vel_bar_2  (the centre's z is swing_height)
//   A = a + p_start_next_bar_l,  C = c + p_final_next_bar_l     the total on the record after the call
//   not replanned:  p_start_bar_l = A, p_final_bar_l = C        the record passed through
//   replanned:      p_start_bar_l = p_final_bar_l = 0 (the record was overwritten),  C_2 := 0 (fh[2] = 0 is a constant), and with
//                   p = FK(q_l), r = Rwb p, half = t_stance / 2, k = planner_k, lip = sqrt(x_z / 9.81) / 2:
//     x_bar += A + C,  x_bar[2] += 0.25 / (9.81 sqrt(x_z / 9.81)) <C, xdot>,  xdot_bar += (half + k + lip) C,  xdot_d_bar += -k C,
//     w_bar += half (r x C),  r_bar = A + half (C x w),  Rwb_bar += r_bar p^T + C hip^T (entrywise, row-major; hip = planner_hip[l]),
//     joint_q_bar_l += J(q_l)^T Rwb^T r_bar
// The legs are summed in the order 0, 1, 2, 3.  The `_in` arrays are added in; each may be its output.  NO cotangent of the phase, of
// gait_dt, of the gait's periods, of swing_height or of the kinematic constants: the clock and the mask are held, as in
// qc_leg_plant_step_adjoint_batch.
// UNDEFINED GRADIENT: `flags` bit l - leg l is replanned and x_z is not finite and > 0 (the LIP square root has no derivative there);
// every row of that robot is NaN.  Other non-finite inputs propagate; nothing is clamped.
//
// Kernels: ONE LANE PER ROBOT, FP64, no LDS, no atomics, 0 B scratch (profiles/swing_reference_kernel_resources.txt); the four legs
// are unrolled so that every per-leg array is indexed by constants.  Launch geometry, the "n beyond one launch" refusal and the tail
// lanes (the index clamped, nothing stored) are qc_sensitivity_swing.hpp's.  Both read every input of a robot before they write any of
// its outputs, and a lane writes its own robot only: an output may be the same array as its `_in` / `_next_` input.
#pragma once
#include "qc_sensitivity.hpp"

namespace qc {

struct SwingReferenceArgs {
  const double *Rwb, *x, *xdot, *w, *xdot_d;  // [n][9], [n][3] ...
  const double* joint_q;                      // [n][4][3]
  double* gait_phase;                         // [n][4], written when gait_dt is given
  const uint8_t* stance;                      // [n][4] or NULL: the phase rule
  const double *gait_duty, *gait_dt;          // [n] or NULL
  SwingState* state;                          // [n] IN/OUT
  double *swing_pos, *swing_vel;              // [n][4][3] optional OUT
  uint8_t* planned;                           // [n] optional OUT
};

struct SwingReferenceAdjointArgs {
  const double *Rwb, *x, *xdot, *w, *joint_q, *gait_phase;
  const uint8_t* stance;
  const double* gait_duty;
  const SwingState* before;                                         // [n] the records before the forward call
  const double *swing_pos_bar, *swing_vel_bar;                      // [n][4][3] optional
  const double *p_start_next_bar, *p_final_next_bar;                // [n][12] optional
  const double *Rwb_bar_in, *x_bar_in, *xdot_bar_in, *w_bar_in, *joint_q_bar_in;  // optional
  double *Rwb_bar, *x_bar, *xdot_bar, *w_bar, *xdot_d_bar, *joint_q_bar, *p_start_bar, *p_final_bar;  // optional OUT
  int32_t* flags;                                                   // [n] optional OUT
};

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

QC_DEV void load12(const double* __restrict__ p, long idx, double (&v)[12]) {
  const double* q = p + 12 * idx;
#pragma unroll
  for (int k = 0; k < 12; k++) v[k] = q[k];
}
// an optional array of 12 * N doubles per robot: zeros when absent
template <int N>
QC_DEV void load_or_zero(const double* p, long idx, double (&v)[N]) {
#pragma unroll
  for (int k = 0; k < N; k++) v[k] = p ? p[N * idx + k] : 0.0;
}
template <int N>
QC_DEV void store_n(double* p, long idx, const double (&v)[N], bool nan) {
#pragma unroll
  for (int k = 0; k < N; k++) p[N * idx + k] = nan ? __builtin_nan("") : v[k];
}

__global__ __launch_bounds__(SENSITIVITY_BLOCK) void swing_reference_kernel(const DevParams* __restrict__ Pg, const long n, const SwingReferenceArgs a) {
  for (long base = (long)blockIdx.x * SENSITIVITY_BLOCK; base < n; base += (long)gridDim.x * SENSITIVITY_BLOCK) {
    const long me = base + threadIdx.x;
    const bool live = me < n;
    const long i = live ? me : n - 1;  // tail lanes: the last robot again, nothing stored
    CParams& P = *QC_PARAMS_HERE(Pg);
    // everything the robot reads, back to back
    double R[9], x[3], xdot[3], w[3], xdd[3], q[12], ph[4], ps[12], pf[12];
    int prev[4], had[4];
    load9(a.Rwb, i, R);
    load3(a.x, i, x);
    load3(a.xdot, i, xdot);
    load3(a.w, i, w);
    load3(a.xdot_d, i, xdd);
    load12(a.joint_q, i, q);
    SwingState* S = a.state + i;
#pragma unroll
    for (int l = 0; l < 4; l++) {
      ph[l] = a.gait_phase[4 * i + l];
      prev[l] = S->leg_state[l];
      had[l] = S->has_traj[l];
    }
#pragma unroll
    for (int k = 0; k < 12; k++) {
      ps[k] = S->p_start[k];
      pf[k] = S->p_final[k];
    }
    const uint32_t sw = a.stance ? *reinterpret_cast<const uint32_t*>(a.stance + 4 * i) : 0u;
    const double duty = a.gait_duty ? a.gait_duty[i] : P.stance_phase;
    if (a.gait_dt) {  // the clock of this robot advances first
      const double step = gait_clock_step(P, a.gait_dt[i]);
#pragma unroll
      for (int l = 0; l < 4; l++) ph[l] = advance_phase(ph[l], step);
    }
    const uint32_t stance = contact_mask(a.stance != nullptr, sw, true, ph, duty, true);
    const bool first = prev[0] < 0;  // state_map_.empty()
    uint32_t plan = 0u;
#pragma unroll
    for (int l = 0; l < 4; l++)
      if (leg_replans(!((stance >> l) & 1u), first, prev[l])) plan |= 1u << l;
    const bool any = plan != 0u;
    double pos[12], vel[12];
    int has[4];
#pragma unroll
    for (int l = 0; l < 4; l++) {
      const bool swing = !((stance >> l) & 1u);
      if ((plan >> l) & 1u) {
        const double ql[3] = {q[3 * l], q[3 * l + 1], q[3 * l + 2]};
        double pb[3], r[3], fh[3];
        leg_fk(P, l, leg_trig(ql), pb);
        mat_vec(R, pb, r);  // Rwb foot_body: the lever arm, the expression of wrench_from_state
        plan_foothold(P, l, R, x, xdot, w, xdd, r, fh);
#pragma unroll
        for (int k = 0; k < 3; k++) {
          ps[3 * l + k] = r[k] + x[k];  // Rwb foot + x
          pf[3 * l + k] = fh[k];
        }
      }
      has[l] = any ? (int)((plan >> l) & 1u) : had[l];
      double sp[3] = {0.0, 0.0, 0.0}, sv[3] = {0.0, 0.0, 0.0};  // FootState(): a stance leg, or a swing leg without a trajectory
      if (swing && has[l]) {
        const double p0[3] = {ps[3 * l], ps[3 * l + 1], ps[3 * l + 2]}, p1[3] = {pf[3 * l], pf[3 * l + 1], pf[3 * l + 2]};
        track_swing(P, ph[l], p0, p1, sp, sv);
      }
#pragma unroll
      for (int k = 0; k < 3; k++) {
        pos[3 * l + k] = sp[k];
        vel[3 * l + k] = sv[k];
      }
    }
    if (live) {
#pragma unroll
      for (int l = 0; l < 4; l++) {
        if (a.gait_dt) a.gait_phase[4 * i + l] = ph[l];
        S->leg_state[l] = (int)((stance >> l) & 1u);
        S->has_traj[l] = has[l];
        if ((plan >> l) & 1u) {
#pragma unroll
          for (int k = 0; k < 3; k++) {
            S->p_start[3 * l + k] = ps[3 * l + k];
            S->p_final[3 * l + k] = pf[3 * l + k];
          }
        }
      }
      if (a.swing_pos) store_n(a.swing_pos, i, pos, false);
      if (a.swing_vel) store_n(a.swing_vel, i, vel, false);
      if (a.planned) a.planned[i] = (uint8_t)plan;
    }
  }
}

__global__ __launch_bounds__(SENSITIVITY_BLOCK) void swing_reference_adjoint_kernel(const DevParams* __restrict__ Pg, const long n,
                                                                                    const SwingReferenceAdjointArgs a) {
  for (long base = (long)blockIdx.x * SENSITIVITY_BLOCK; base < n; base += (long)gridDim.x * SENSITIVITY_BLOCK) {
    const long me = base + threadIdx.x;
    const bool live = me < n;
    const long i = live ? me : n - 1;  // tail lanes: the last robot again, nothing stored
    CParams& P = *QC_PARAMS_HERE(Pg);
    // every input of the robot first: an output may be one of these arrays
    double R[9], x[3], xdot[3], w[3], q[12], ph[4];
    double sA[12], sC[12], pbar[12], vbar[12];          // the cotangents on the record after the call, on swing_pos and on swing_vel
    double Rb[9], xb[3], xdb[3], wb[3], xddb[3] = {0.0, 0.0, 0.0}, qb[12];
    int prev[4], had[4];
    load9(a.Rwb, i, R);
    load3(a.x, i, x);
    load3(a.xdot, i, xdot);
    load3(a.w, i, w);
    load12(a.joint_q, i, q);
    const SwingState* S = a.before + i;
#pragma unroll
    for (int l = 0; l < 4; l++) {
      ph[l] = a.gait_phase[4 * i + l];
      prev[l] = S->leg_state[l];
      had[l] = S->has_traj[l];
    }
    load_or_zero(a.p_start_next_bar, i, sA);
    load_or_zero(a.p_final_next_bar, i, sC);
    load_or_zero(a.swing_pos_bar, i, pbar);
    load_or_zero(a.swing_vel_bar, i, vbar);
    load_or_zero(a.Rwb_bar_in, i, Rb);
    load_or_zero(a.x_bar_in, i, xb);
    load_or_zero(a.xdot_bar_in, i, xdb);
    load_or_zero(a.w_bar_in, i, wb);
    load_or_zero(a.joint_q_bar_in, i, qb);
    const uint32_t sw = a.stance ? *reinterpret_cast<const uint32_t*>(a.stance + 4 * i) : 0u;
    const double duty = a.gait_duty ? a.gait_duty[i] : P.stance_phase;
    const uint32_t stance = contact_mask(a.stance != nullptr, sw, true, ph, duty, true);
    const bool first = prev[0] < 0;
    uint32_t plan = 0u;
#pragma unroll
    for (int l = 0; l < 4; l++)
      if (leg_replans(!((stance >> l) & 1u), first, prev[l])) plan |= 1u << l;
    const bool any = plan != 0u;
    const double half = 0.5 * P.t_stance, kpl = P.planner_k;
    const double root = sqrt(x[2] / 9.81), lip = 0.5 * root, dlip = 0.25 / (9.81 * root);
    const bool undefined = !(x[2] > 0.0 && x[2] < __builtin_inf());
    int fl = 0;
#pragma unroll
    for (int l = 0; l < 4; l++) {
      const bool swing = !((stance >> l) & 1u), planned = (plan >> l) & 1u;
      const int has = any ? (int)planned : had[l];
      double A[3] = {sA[3 * l], sA[3 * l + 1], sA[3 * l + 2]}, C[3] = {sC[3 * l], sC[3 * l + 1], sC[3 * l + 2]};
      if (swing && has) {  // the transpose of track_swing's linear map
        double h[3], dh[3];
        swing_basis(P, ph[l], h, dh);
#pragma unroll
        for (int r = 0; r < 3; r++) {
          const double pr = pbar[3 * l + r], vr = vbar[3 * l + r];
          const double m = r < 2 ? 0.5 : 0.0;  // the centre point: the mean of the ends in x and y, a constant in z
          A[r] += (h[0] + m * h[2]) * pr + (dh[0] + m * dh[2]) * vr;
          C[r] += (h[1] + m * h[2]) * pr + (dh[1] + m * dh[2]) * vr;
        }
      }
      if (planned) {
        if (undefined) fl |= 1 << l;
        C[2] = 0.0;  // fh[2] = 0
        const double ql[3] = {q[3 * l], q[3 * l + 1], q[3 * l + 2]};
        const LegTrig t = leg_trig(ql);
        double p[3], r[3], rxc[3], cxw[3], rbar[3], rt[3], jq[3];
        leg_fk(P, l, t, p);
        mat_vec(R, p, r);
        cross3(r, C, rxc);
        cross3(C, w, cxw);
        const double cv = C[0] * xdot[0] + C[1] * xdot[1] + C[2] * xdot[2];
        const double gain = half + kpl + lip;
#pragma unroll
        for (int k = 0; k < 3; k++) {
          xb[k] += A[k] + C[k];
          xdb[k] += gain * C[k];
          xddb[k] += -kpl * C[k];
          wb[k] += half * rxc[k];
          rbar[k] = A[k] + half * cxw[k];
        }
        xb[2] += dlip * cv;
#pragma unroll
        for (int rr = 0; rr < 3; rr++)
#pragma unroll
          for (int k = 0; k < 3; k++) Rb[3 * rr + k] += rbar[rr] * p[k] + C[rr] * P.planner_hip[3 * l + k];
        mat_t_vec(R, rbar, rt);
        leg_jt_force(P, l, t, rt, jq);  // J(q_l)^T Rwb^T r_bar
#pragma unroll
        for (int k = 0; k < 3; k++) {
          qb[3 * l + k] += jq[k];
          sA[3 * l + k] = 0.0;  // the record was overwritten
          sC[3 * l + k] = 0.0;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 3; k++) {
          sA[3 * l + k] = A[k];
          sC[3 * l + k] = C[k];
        }
      }
    }
    if (live) {
      const bool nan = fl != 0;  // no gradient: every row of the robot
      if (a.Rwb_bar) store_n(a.Rwb_bar, i, Rb, nan);
      if (a.x_bar) store_n(a.x_bar, i, xb, nan);
      if (a.xdot_bar) store_n(a.xdot_bar, i, xdb, nan);
      if (a.w_bar) store_n(a.w_bar, i, wb, nan);
      if (a.xdot_d_bar) store_n(a.xdot_d_bar, i, xddb, nan);
      if (a.joint_q_bar) store_n(a.joint_q_bar, i, qb, nan);
      if (a.p_start_bar) store_n(a.p_start_bar, i, sA, nan);
      if (a.p_final_bar) store_n(a.p_final_bar, i, sC, nan);
      if (a.flags) a.flags[i] = fl;
    }
  }
}

}  // namespace qc
#endif  // __HIPCC__
