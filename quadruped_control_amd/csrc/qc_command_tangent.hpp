// qc_command_tangent.hpp - forward mode of the two stages through which a rollout is steered: qc_commander_step_tangent_batch and
// qc_com_reference_tangent_batch (include/qc_tangent.h), the forward derivatives of qc_commander_step_batch (qc_commander.hpp) and
// qc_com_reference_batch (qc_com_reference.hpp) and so the maps commander_step_adjoint_kernel and com_reference_adjoint_kernel
// transpose.  In a forward-mode commander rollout the first stands in front of the gait step: it writes the Rwb_d_rot_tan, x_d_tan,
// xdot_d_tan, w_d_tan that qc_tangent_batch and qc_swing_reference_tangent_batch read, and carries the tangents of the record's
// desired state and of the held command from step to step in place.  The second turns the tangents of the feet, the pose, the phases
// and the schedule of the lean into the tangent of the x_d a tick tracks.
//
// COMMANDER STEP.  The contract of the inputs is the adjoint's: nothing is saved by the forward launch; the caller passes Rwb, x,
// twist, fresh, the three scalars and the records from BEFORE the forward call (`before`); fresh / standing / running / pending /
// applied are recomputed as commander_step (qc_device.hpp) decides them and HELD.  Per direction, in the adjoint's symbols
// (v = vb[0:3], om = vb[3:6], d = cmd_dt om, Rb = Exp(d), t = cmd_dt Rb v, Y = Rz(yaw), (cy, sy) = (R00, R10) / h, u = v - x x om),
// delta the world-frame left tangent of Rwb, dvb = fresh ? twist_tan : Vb_tan = (dv, dom):
//   always        Vb_next_tan = dvb
//   not applied   the four outputs are the four _prev_ tangents, bit for bit
//   applied       beta = Jl(d) cmd_dt dom                      the left tangent of Rb
//                 dt   = beta x t + cmd_dt Rb dv
//                 dpsi = (cy (delta_2 R00 - delta_0 R20) - sy (delta_1 R20 - delta_2 R10)) / h
//                 Rwb_d_rot_tan = dpsi e_z + Y beta
//                 x_d_tan = (dx_0 + g_0, dx_1 + g_1, 0),  g = dpsi e_z x (Y t) + Y dt        (the height is a constant)
//                 xdot_d_tan = Rwb^T (du - delta x u),  du = dv - dx x om - x x dom
//                 w_d_tan = Rwb^T (dom - delta x om)
// Rb and Jl are applied as cross products (exp_apply) with the coefficients of the plant tangent: A = sin th / th, B = (1 - cos th) /
// th^2 from sincos_joint(th / 2), Jl's pair from left_jacobian_coefficients - the series below th^2 = 1, the quotients from it on, the
// limits at th = 0.  SMALL ANGLE (th < 1e-12, where the forward pass takes Rb = I): the SMOOTH function is differentiated, as the
// adjoint does, so a yaw-rate tangent at zero rate is not silently zero.
// `flags` bit 0 - a command is applied at the gimbal-lock branch (h == 0 or not finite below 1e300: the adjoint's rule); every output
// row of that robot, in every direction, is NaN.  Other non-finite inputs propagate; nothing is clamped.
//
// COM REFERENCE.  It takes what com_reference_kernel takes; the contact mask is HELD (support_load's own contact_mask).  Per direction,
// robot and leg l, with r_l = Rwb p_l, (a_i, d_i, e_i, sgn) the adjoint's (support_reverse):
//   dp_l = feet_tan_l + J(q_l) joint_q_tan_l,   dP_l = (delta x r_l + Rwb dp_l + dx) in x and y
//   dw_l = sgn (e1 / d1 - e2 / d2) dphi_l - sum_i e_i a_i root2 / d_i dsigma_i          over the two widths the leg's branch reads
//   dzm = w dP + (1 - w) dP_m + (P - P_m) dw,  dzp likewise
//   dN  = ((dw P + w dP) + (dw_m zm + w_m dzm)) + (dw_p zp + w_p dzp),  dD = (dw + dw_m) + dw_p,  dv = (dN - v dD) / D
//   com_xy_tan = (((dv_FL + dv_FR) + dv_RL) + dv_RR) / 4
//   QC_COM_REPLACE   x_d_out_tan = (com_xy_tan, x_d_in_tan.z)
//   QC_COM_OFFSET    x_d_out_tan = x_d_in_tan + gain (com_xy_tan - (((dP_FL + dP_FR) + dP_RL) + dP_RR) / 4, 0)
// `flags` bit l: the forward rule (the reference's 0/0 at leg l's point); a flagged robot gets NaN in every output row of every
// direction.
//
// Kernels: one lane per (direction, robot), the robot index fastest - pair j = k n + i is row j of a [K][n][m] array -, as
// qc_plant_tangent.hpp.  FP64, workgroups of one wave, a grid stride once the grid is capped, no LDS, no atomics, no scratch
// (profiles/command_tangent_kernel_resources.txt).  A NULL tangent is zero; a NULL output is not stored.  A pair reads ALL of its inputs
// before it writes anything and touches only its own rows: the four desired-state outputs may BE the four _prev_ inputs, Vb_next_tan may
// be Vb_tan, x_d_out_tan may be x_d_in_tan.  The robot's flag word is written by its direction-0 pair.
#pragma once
#include "qc_commander.hpp"          // CmdState (through qc_device.hpp), load_or_zero, store_n
#include "qc_com_reference.hpp"      // SupportIn, support_load, support_point, COM_OFFSET
#include "qc_leg_plant_tangent.hpp"  // leg_jacobian_apply, left_jacobian_coefficients, exp_apply, load3_or_zero

namespace qc {

struct CommanderStepTangentArgs {
  const double *Rwb, *x, *twist;  // [n][9], [n][3], [n][6] or NULL
  const uint8_t* fresh;           // [n] or NULL
  const CmdState* before;         // [n] the records before the forward call
  double stand_height, stand_tol, cmd_dt;
  long n_dir;                     // K (1 for a call that asks for the flags alone)
  const double *twist_tan, *Vb_tan;                                                    // [K][n][6], nullptr: zero
  const double *Rwb_rot_tan, *x_tan;                                                   // [K][n][3]
  const double *Rwb_d_rot_prev_tan, *x_d_prev_tan, *xdot_d_prev_tan, *w_d_prev_tan;    // [K][n][3] on the record before the call
  double *Rwb_d_rot_tan, *x_d_tan, *xdot_d_tan, *w_d_tan;                              // [K][n][3] optional OUT
  double* Vb_next_tan;                                                                 // [K][n][6] optional OUT
  int32_t* flags;                                                                      // [n] optional OUT
};

struct ComReferenceTangentArgs : SupportIn {  // (always world mode)
  int mode;
  double gain;
  long n_dir;  // K (1 for a call that asks for the flags alone)
  const double *x_d_in_tan, *feet_tan, *joint_q_tan, *Rwb_rot_tan, *x_tan, *phase_tan;  // [K][n][3|12|12|3|3|4], nullptr: zero
  const double* schedule_tan;                                                           // [K][n][16], or [K][16] if shared
  double *x_d_out_tan, *com_xy_tan;                                                     // [K][n][3], [K][n][2] optional OUT
  int32_t* flags;                                                                       // [n] optional OUT
};

constexpr int COMMAND_TANGENT_BLOCK = 64;  // one wave
constexpr int COMMAND_TANGENT_MAX_BLOCKS = 4096;

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

__global__ __launch_bounds__(COMMAND_TANGENT_BLOCK) void commander_step_tangent_kernel(const long n, const CommanderStepTangentArgs a) {
  const long total = n * a.n_dir;
  for (long j = (long)blockIdx.x * COMMAND_TANGENT_BLOCK + threadIdx.x; j < total; j += (long)gridDim.x * COMMAND_TANGENT_BLOCK) {
    const long i = j % n;  // pair j = k n + i: the row of direction k and robot i in a [K][n][m] array is j itself
    // ---- the robot: what does not depend on the direction
    double R[9], x[3], vb[6];
    load9(a.Rwb, i, R);
    load3(a.x, i, x);
    const CmdState* C = a.before + i;
    const bool fresh = a.fresh && a.fresh[i] != 0;
    const int standing0 = C->standing, running = C->gait_running, pending0 = C->cmd_pending;
#pragma unroll
    for (int k = 0; k < 6; k++) vb[k] = fresh ? a.twist[6 * i + k] : C->Vb[k];
    // ---- the direction: every tangent of the pair, before anything is written
    double dvb[6], dl[3], dx[3], rot[3], xd[3], xdotd[3], wd[3];
    load_or_zero(fresh ? a.twist_tan : a.Vb_tan, j, dvb);
    load3_or_zero(a.Rwb_rot_tan, j, dl);
    load3_or_zero(a.x_tan, j, dx);
    load3_or_zero(a.Rwb_d_rot_prev_tan, j, rot);
    load3_or_zero(a.x_d_prev_tan, j, xd);
    load3_or_zero(a.xdot_d_prev_tan, j, xdotd);
    load3_or_zero(a.w_d_prev_tan, j, wd);
    // ---- the held decisions, as commander_step takes them
    const bool standing = standing0 || fabs(x[2] - a.stand_height) < a.stand_tol;
    const bool applied = standing && running && (pending0 || fresh);
    int fl = 0;
    if (applied) {
      const double dt = a.cmd_dt;
      const double v[3] = {vb[0], vb[1], vb[2]}, om[3] = {vb[3], vb[4], vb[5]};
      const double dv[3] = {dvb[0], dvb[1], dvb[2]}, dom[3] = {dvb[3], dvb[4], dvb[5]};
      const double d[3] = {om[0] * dt, om[1] * dt, om[2] * dt}, dd[3] = {dom[0] * dt, dom[1] * dt, dom[2] * dt};
      // Exp(d) and Jl(d) of the ANALYTIC function, also below the forward pass's 1e-12 threshold: the plant tangent's coefficients
      const double xx = d[0] * d[0], yy = d[1] * d[1], zz = d[2] * d[2];
      const double th2 = xx + yy + zz;
      const double hh = 0.5 * sqrt(th2);
      double sh, ch;
      sincos_joint(hh, &sh, &ch);
      const double sc = hh > 0.0 ? sh / hh : 1.0;
      const double A = sc * ch, B = 0.5 * (sc * sc);
      double Bj, Cj, beta[3], rv[3], rdv[3], t[3], bt[3], dtt[3];
      left_jacobian_coefficients(th2, A, B, &Bj, &Cj);
      exp_apply(d, Bj, Cj, dd, beta);
      exp_apply(d, A, B, v, rv);
      exp_apply(d, A, B, dv, rdv);
#pragma unroll
      for (int k = 0; k < 3; k++) t[k] = dt * rv[k];
      cross3(beta, t, bt);
#pragma unroll
      for (int k = 0; k < 3; k++) dtt[k] = bt[k] + dt * rdv[k];
      // the yaw of Rwb and its tangent
      const double h = __builtin_sqrt(R[0] * R[0] + R[3] * R[3]);
      const bool ok = h > 0.0 && h < 1.0e300;
      if (!ok) fl = 1;
      const double cy = R[0] / h, sy = R[3] / h;
      const double dpsi = (cy * (dl[2] * R[0] - dl[0] * R[6]) - sy * (dl[1] * R[6] - dl[2] * R[3])) / h;
      const double yt[2] = {cy * t[0] - sy * t[1], sy * t[0] + cy * t[1]};
      rot[0] = cy * beta[0] - sy * beta[1];
      rot[1] = sy * beta[0] + cy * beta[1];
      rot[2] = dpsi + beta[2];
      xd[0] = dx[0] + ((cy * dtt[0] - sy * dtt[1]) - dpsi * yt[1]);
      xd[1] = dx[1] + ((sy * dtt[0] + cy * dtt[1]) + dpsi * yt[0]);
      xd[2] = 0.0;  // stand_height
      // Ad_T: xdot_d = R^T u, w_d = R^T om
      double xo[3], u[3], dxo[3], xdo[3], du[3], cu[3], co[3], e1[3], e2[3];
      cross3(x, om, xo);
      cross3(dx, om, dxo);
      cross3(x, dom, xdo);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        u[k] = v[k] - xo[k];
        du[k] = dv[k] - dxo[k] - xdo[k];
      }
      cross3(dl, u, cu);
      cross3(dl, om, co);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        e1[k] = du[k] - cu[k];
        e2[k] = dom[k] - co[k];
      }
      mat_t_vec(R, e1, xdotd);
      mat_t_vec(R, e2, wd);
    }
    // every input of this pair has been read: an output may overwrite an input tangent
    const bool nan = fl != 0;  // no derivative: every row of the robot, in every direction
    if (a.Rwb_d_rot_tan) store_n(a.Rwb_d_rot_tan, j, rot, nan);
    if (a.x_d_tan) store_n(a.x_d_tan, j, xd, nan);
    if (a.xdot_d_tan) store_n(a.xdot_d_tan, j, xdotd, nan);
    if (a.w_d_tan) store_n(a.w_d_tan, j, wd, nan);
    if (a.Vb_next_tan) store_n(a.Vb_next_tan, j, dvb, nan);
    if (a.flags && j < n) a.flags[i] = fl;
  }
}

__global__ __launch_bounds__(COMMAND_TANGENT_BLOCK) void com_reference_tangent_kernel(const DevParams* __restrict__ Pg, const long n,
                                                                                      const ComReferenceTangentArgs a) {
  const long total = n * a.n_dir;
  for (long j = (long)blockIdx.x * COMMAND_TANGENT_BLOCK + threadIdx.x; j < total; j += (long)gridDim.x * COMMAND_TANGENT_BLOCK) {
    const long i = j % n;  // pair j = k n + i: the row of direction k and robot i in a [K][n][m] array is j itself
    CParams& P = *QC_PARAMS_HERE(Pg);
    // ---- the robot: the points, the ramps, the held mask - the forward kernel's own loads
    SupportRobot S;
    support_load(P, a, i, S);
    // ---- the direction: every tangent of the pair, before anything is written
    double xdt[3], ft[12], dq[12], dl[3], dx[3], dph[4], dsg[16];
    load3_or_zero(a.x_d_in_tan, j, xdt);
    load_or_zero(a.feet_tan, j, ft);
    load_or_zero(a.joint_q_tan, j, dq);
    load3_or_zero(a.Rwb_rot_tan, j, dl);
    load3_or_zero(a.x_tan, j, dx);
    load_or_zero(a.phase_tan, j, dph);
    load_or_zero(a.schedule_tan, a.shared ? j / n : j, dsg);
    // ---- the points' and the weights' tangents
    double dP[4][2], dw[4];
#pragma unroll
    for (int l = 0; l < 4; l++) {
      double dp[3] = {ft[3 * l], ft[3 * l + 1], ft[3 * l + 2]};
      if (a.joint_q_tan) {  // (only with joint_q: the host check)
        const double ql[3] = {a.joint_q[12 * i + 3 * l], a.joint_q[12 * i + 3 * l + 1], a.joint_q[12 * i + 3 * l + 2]};
        const double dql[3] = {dq[3 * l], dq[3 * l + 1], dq[3 * l + 2]};
        const LegGeom lg = {P.links[3 * l], P.links[3 * l + 1], P.links[3 * l + 2], P.hip[3 * l], P.hip[3 * l + 1], P.hip[3 * l + 2]};
        double jdq[3];
        leg_jacobian_apply(lg, leg_trig(ql), dql, jdq);
#pragma unroll
        for (int k = 0; k < 3; k++) dp[k] += jdq[k];
      }
      double r[3], rdp[3], cr[3];
      mat_vec(S.R, S.pb[l], r);
      mat_vec(S.R, dp, rdp);
      cross3(dl, r, cr);
      dP[l][0] = (cr[0] + rdp[0]) + dx[0];
      dP[l][1] = (cr[1] + rdp[1]) + dx[1];
      const bool st = (S.stance >> l) & 1u;
      const SupportRamp& rm = S.ramp[l];
      const double e1 = exp_neg_sq(rm.a1) * SUPPORT_INV_SQRT_PI, e2 = exp_neg_sq(rm.a2) * SUPPORT_INV_SQRT_PI;
      const double ph = (e1 / rm.d1 - e2 / rm.d2) * dph[l];
      const double s1 = st ? dsg[4 * l] : dsg[4 * l + 2], s2 = st ? dsg[4 * l + 1] : dsg[4 * l + 3];
      const double b1 = e1 * rm.a1 * SUPPORT_ROOT2 / rm.d1, b2 = e2 * rm.a2 * SUPPORT_ROOT2 / rm.d2;
      dw[l] = (st ? ph : -ph) - (b1 * s1 + b2 * s2);
    }
    // ---- steps 2 and 3 of the polygon, in the forward pass's summation order
    double dv[4][2];
    int fl = 0;
#pragma unroll
    for (int l = 0; l < 4; l++) {
      const int m = SUPPORT_MINUS[l], p = SUPPORT_PLUS[l];
      double D, zm[2], zp[2], v[2];
      if (support_point(S, l, D, zm, zp, v)) fl |= 1 << l;
      const double w = S.ramp[l].w, wm = S.ramp[m].w, wp = S.ramp[p].w;
      const double dD = (dw[l] + dw[m]) + dw[p];
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const double dzm = (w * dP[l][k] + (1.0 - w) * dP[m][k]) + (S.P[l][k] - S.P[m][k]) * dw[l];
        const double dzp = (w * dP[l][k] + (1.0 - w) * dP[p][k]) + (S.P[l][k] - S.P[p][k]) * dw[l];
        const double dN = ((dw[l] * S.P[l][k] + w * dP[l][k]) + (dw[m] * zm[k] + wm * dzm)) + (dw[p] * zp[k] + wp * dzp);
        dv[l][k] = (dN - v[k] * dD) / D;
      }
    }
    double com[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
      com[k] = (((dv[SUPPORT_SUM_ORDER[0]][k] + dv[SUPPORT_SUM_ORDER[1]][k]) + dv[SUPPORT_SUM_ORDER[2]][k]) + dv[SUPPORT_SUM_ORDER[3]][k]) / 4.0;
      double o = com[k];
      if (a.mode == COM_OFFSET) {
        const double cen = (((dP[SUPPORT_SUM_ORDER[0]][k] + dP[SUPPORT_SUM_ORDER[1]][k]) + dP[SUPPORT_SUM_ORDER[2]][k]) + dP[SUPPORT_SUM_ORDER[3]][k]) / 4.0;
        o = xdt[k] + a.gain * (com[k] - cen);
      }
      xdt[k] = o;
    }
    // every input of this pair has been read: x_d_out_tan may be x_d_in_tan
    const bool nan = fl != 0;  // no derivative: every row of the robot, in every direction
    if (a.x_d_out_tan) store_n(a.x_d_out_tan, j, xdt, nan);
    if (a.com_xy_tan) store_n(a.com_xy_tan, j, com, nan);
    if (a.flags && j < n) a.flags[i] = fl;
  }
}

}  // namespace qc
#endif  // __HIPCC__
