// qc_swing_reference_tangent.hpp - forward mode of the swing references: qc_swing_reference_tangent_batch (include/qc_tangent.h), the
// forward derivative of qc_swing_reference_batch - the foothold planner and the sextic swing trajectory - and so the map
// swing_reference_adjoint_kernel (qc_swing_reference.hpp) transposes.  In a forward-mode gait rollout it stands between
// qc_swing_reference_batch and the tick's tangents: it writes the swing_pos_tan / swing_vel_tan that qc_swing_torque_tangent_batch
// reads, and carries the tangents of the record (p_start, p_final) from step to step in place.
//
// The contract of the inputs is the adjoint's: nothing is saved by the forward launch; gait_phase is read as the forward call left it
// (no clock is advanced) and the records from BEFORE it (`before`), from whose leg_state / has_traj and the contact mask the plan
// decision is recomputed by the forward kernel's own contact_mask and leg_replans.  The clock, the mask and the decisions are HELD.
// Per direction, robot and leg l, in the adjoint's symbols (p = FK(q_l), r = Rwb p, half = t_stance / 2, k = planner_k,
// lip = sqrt(x_z / 9.81) / 2, hip = planner_hip[l]), delta the world-frame left tangent of Rwb:
//   replanned:      dr  = delta x r + Rwb J(q_l) dq_l
//                   dps = dr + dx
//                   dpf = delta x (Rwb hip) + dx + (half + k + lip) dxdot - k dxdot_d + (0.25 / (9.81 sqrt(x_z / 9.81))) dx_z xdot
//                         + half (dw x r + w x dr),   dpf_z := 0 (fh[2] = 0 is a constant)
//   not replanned:  dps = p_start_tan_l, dpf = p_final_tan_l            the record passed through
//   track           swing leg with a trajectory after the call, (h, h') = swing_basis(phase_l) - track_swing's own loop:
//                   dpos_r = (h0 + m h2) dps_r + (h1 + m h2) dpf_r, dvel_r likewise with h'; m = 1/2 for x and y, 0 for z
//                   every other leg: exact zeros
//   record          p_start_next_tan_l = dps, p_final_next_tan_l = dpf
// `flags` bit l - leg l is replanned and x_z is not finite and > 0 (the adjoint's rule); a robot with any bit set gets NaN in every
// output row of every direction.  Other non-finite inputs propagate; nothing is clamped.
//
// Kernel: one lane per (direction, robot), the robot index fastest - pair j = k n + i is row j of a [K][n][m] array -, as
// qc_plant_tangent.hpp: a wave's loads of one direction's rows are contiguous and K multiplies the parallelism.  The data of a robot
// that does not depend on the direction (R, x, xdot, w, q, the phases, the decisions; per leg p, r, Rwb hip, the trigonometry of J, the
// basis values) is read and formed once per lane.  The four legs are unrolled so that every per-leg array is indexed by constants.
// FP64, workgroups of one wave, a grid stride once the grid is capped (SWING_REFERENCE_TANGENT_MAX_BLOCKS), no LDS, no atomics, no
// scratch (profiles/swing_reference_tangent_kernel_resources.txt).  A NULL tangent is zero; a NULL output is not stored.  A pair reads
// ALL of its inputs before it writes anything and touches only its own rows: p_start_next_tan may be p_start_tan, p_final_next_tan may
// be p_final_tan, swing_pos_tan / swing_vel_tan any [K][n][12] input tangent.  The robot's flag word is written by its direction-0 pair.
#pragma once
#include "qc_swing_reference.hpp"    // SwingState, load12, load_or_zero, store_n
#include "qc_leg_plant_tangent.hpp"  // leg_jacobian_apply, load3_or_zero

namespace qc {

struct SwingReferenceTangentArgs {
  const double *Rwb, *x, *xdot, *w, *joint_q, *gait_phase;  // [n][9], [n][3] x 3, [n][12], [n][4]
  const uint8_t* stance;                                    // [n][4] or NULL: the phase rule
  const double* gait_duty;                                  // [n] or NULL: the handle's
  const SwingState* before;                                 // [n] the records before the forward call
  long n_dir;                                               // K (1 for a call that asks for the flags alone)
  const double *Rwb_rot_tan, *x_tan, *xdot_tan, *w_tan, *xdot_d_tan;  // [K][n][3], nullptr: zero
  const double *joint_q_tan, *p_start_tan, *p_final_tan;              // [K][n][12], nullptr: zero
  double *swing_pos_tan, *swing_vel_tan, *p_start_next_tan, *p_final_next_tan;  // [K][n][12] optional OUT
  int32_t* flags;                                                     // [n] optional OUT
};

constexpr int SWING_REFERENCE_TANGENT_BLOCK = 64;  // one wave
constexpr int SWING_REFERENCE_TANGENT_MAX_BLOCKS = 4096;

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

__global__ __launch_bounds__(SWING_REFERENCE_TANGENT_BLOCK) void swing_reference_tangent_kernel(const DevParams* __restrict__ Pg, const long n,
                                                                                                const SwingReferenceTangentArgs a) {
  const long total = n * a.n_dir;
  for (long j = (long)blockIdx.x * SWING_REFERENCE_TANGENT_BLOCK + threadIdx.x; j < total; j += (long)gridDim.x * SWING_REFERENCE_TANGENT_BLOCK) {
    const long i = j % n;  // pair j = k n + i: the row of direction k and robot i in a [K][n][m] array is j itself
    CParams& P = *QC_PARAMS_HERE(Pg);
    // ---- the robot: what does not depend on the direction
    double R[9], x[3], xdot[3], w[3], q[12], ph[4];
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
    // ---- the direction: every tangent of the pair, before anything is written
    double dl[3], dx[3], dv[3], dw[3], dvd[3], dq[12], dps[12], dpf[12];
    load3_or_zero(a.Rwb_rot_tan, j, dl);
    load3_or_zero(a.x_tan, j, dx);
    load3_or_zero(a.xdot_tan, j, dv);
    load3_or_zero(a.w_tan, j, dw);
    load3_or_zero(a.xdot_d_tan, j, dvd);
    load_or_zero(a.joint_q_tan, j, dq);
    load_or_zero(a.p_start_tan, j, dps);
    load_or_zero(a.p_final_tan, j, dpf);
    // ---- the held decisions, by the forward kernel's functions
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
    const double gain = half + kpl + lip, dz = dlip * dx[2];
    const int fl = undefined ? (int)plan : 0;  // bit l: leg l is replanned where the LIP square root has no derivative
    double dpos[12], dvel[12];
#pragma unroll
    for (int l = 0; l < 4; l++) {
      const bool swing = !((stance >> l) & 1u), planned = (plan >> l) & 1u;
      const int has = any ? (int)planned : had[l];
      if (planned) {
        const double ql[3] = {q[3 * l], q[3 * l + 1], q[3 * l + 2]}, dql[3] = {dq[3 * l], dq[3 * l + 1], dq[3 * l + 2]};
        const double hip[3] = {P.planner_hip[3 * l], P.planner_hip[3 * l + 1], P.planner_hip[3 * l + 2]};
        const LegGeom lg = {P.links[3 * l], P.links[3 * l + 1], P.links[3 * l + 2], P.hip[3 * l], P.hip[3 * l + 1], P.hip[3 * l + 2]};
        const LegTrig t = leg_trig(ql);
        double p[3], r[3], rh[3], jdq[3], rj[3], cr[3], dr[3], ch[3], dwr[3], wdr[3];
        leg_fk(P, l, t, p);
        mat_vec(R, p, r);
        mat_vec(R, hip, rh);
        leg_jacobian_apply(lg, t, dql, jdq);
        mat_vec(R, jdq, rj);
        cross3(dl, r, cr);
#pragma unroll
        for (int k = 0; k < 3; k++) dr[k] = cr[k] + rj[k];
        cross3(dl, rh, ch);
        cross3(dw, r, dwr);
        cross3(w, dr, wdr);
#pragma unroll
        for (int k = 0; k < 3; k++) {
          dps[3 * l + k] = dr[k] + dx[k];
          dpf[3 * l + k] = ch[k] + dx[k] + gain * dv[k] - kpl * dvd[k] + dz * xdot[k] + half * (dwr[k] + wdr[k]);
        }
        dpf[3 * l + 2] = 0.0;  // fh[2] = 0
      }
      double h[3] = {0.0, 0.0, 0.0}, dh[3] = {0.0, 0.0, 0.0};
      const bool tracks = swing && has;
      if (tracks) swing_basis(P, ph[l], h, dh);
#pragma unroll
      for (int r = 0; r < 3; r++) {
        const double m = r < 2 ? 0.5 : 0.0;  // the centre point: the mean of the ends in x and y, a constant in z
        const double s = dps[3 * l + r], f = dpf[3 * l + r];
        // (a leg that does not track: exact zeros, whatever the record's tangents hold)
        dpos[3 * l + r] = tracks ? (h[0] + m * h[2]) * s + (h[1] + m * h[2]) * f : 0.0;
        dvel[3 * l + r] = tracks ? (dh[0] + m * dh[2]) * s + (dh[1] + m * dh[2]) * f : 0.0;
      }
    }
    // every input of this pair has been read: an output may overwrite an input tangent
    const bool nan = fl != 0;  // no derivative: every row of the robot, in every direction
    if (a.swing_pos_tan) store_n(a.swing_pos_tan, j, dpos, nan);
    if (a.swing_vel_tan) store_n(a.swing_vel_tan, j, dvel, nan);
    if (a.p_start_next_tan) store_n(a.p_start_next_tan, j, dps, nan);
    if (a.p_final_next_tan) store_n(a.p_final_next_tan, j, dpf, nan);
    if (a.flags && j < n) a.flags[i] = fl;
  }
}

}  // namespace qc
#endif  // __HIPCC__
