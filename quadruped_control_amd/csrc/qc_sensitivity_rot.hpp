// qc_sensitivity_rot.hpp - the two cotangents qc_sensitivity_batch leaves out: those of Rwb and Rwb_d (qc_sensitivity_rot_batch,
// include/qc_balance.h).  A second, small kernel behind the adjoint: it reads the BatchIn the solve read, the forces, the cotangent
// on them and the b_bar and feet_bar the adjoint kernel wrote - never the adjoint itself, and it repeats no 12x12 solve.
//
// With R = Rwb, Rd = Rwb_d, f_i = -R grf_body_i, ba = b_bar[3:6], and every matrix cotangent ENTRYWISE (R_bar[3 a + b] = dL / dR_ab
// of the expressions exactly as wrench_from_state evaluates them - the nine entries are independent variables, R need not stay a
// rotation), R enters the forces four ways:
//   the output transform   grf_body_i = -R^T f_i at fixed f:        R_bar += -sum_i f_i grf_bar_i^T
//   the lever arms         r_i = R p_i, r_bar_i = R feet_bar_i:      R_bar += sum_i r_bar_i p_i^T        (p_i from `feet` or leg_fk)
//   the inertia            Iw = R Ib R^T in b_ang = Iw al + w_d x (Iw w_d):  Iw_bar = ba al^T + (ba x w_d) w_d^T,
//                          R_bar += Iw_bar R Ib^T + Iw_bar^T R Ib  =  ba u1^T + (ba x w_d) u2^T + al v1^T + w_d v2^T
//                          with u1 = Ib R^T al, u2 = Ib R^T w_d (wrench_from_state's own), v1 = Ib^T R^T ba, v2 = Ib^T R^T (ba x w_d);
//                          al recomputed as the library does, kff[5] on index 1 included
//   the rotation error     e = angle_axis_total(Re), Re = Rd R^T:    e_bar = kp_w o (Iw^T ba) = kp_w o (R v1),
//                          Re_bar = angle_axis_total_bwd(Re, e_bar) (qc_device.hpp: the branch taken, the n2 = 0 limit),
//                          R_bar += Re_bar^T Rd,   Rd_bar = Re_bar R
// Rwb_rot_bar / Rwb_d_rot_bar are the world-frame left-tangent projections: for R <- exp([delta]x) R the cotangent of delta at 0 is
// axial(R_bar R^T), axial(M) = (M21 - M12, M02 - M20, M10 - M01) (rows and columns from 0); the same form for Rd.
//
// Swing feet need no mask: their f_i and feet_bar_i are zero.  A robot the adjoint kernel poisoned (NaN b_bar, feet_bar) is NaN in
// every output here - ba reaches every entry of both cotangents.  Non-finite inputs propagate; nothing is clamped.  Commander mode
// is out of scope as for the certificate: the desired rotation must be in `in` (cmd_state is NULL in the BatchIn this kernel gets).
//
// Kernel: one lane per robot, FP64, workgroups of one wave, the adjoint kernel's grid (sensitivity_blocks) and tail-lane
// convention.  No LDS, no scratch.  `in` and the four input arrays are never written.
#pragma once
#include "qc_sensitivity.hpp"

namespace qc {

struct SensitivityRotArgs {
  const double *grf_body, *grf_bar;                          // [n][4][3]
  const double *b_bar, *feet_bar;                            // [n][6], [n][4][3]: as qc_sensitivity_batch wrote them
  double *Rwb_bar, *Rwb_d_bar, *Rwb_rot_bar, *Rwb_d_rot_bar;  // optional OUT [n][9], [n][9], [n][3], [n][3]
};

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

// axial(Mb R^T): the left-tangent projection of an entrywise cotangent Mb of R
QC_DEV void rot_tangent(const double (&Mb)[9], const double (&R)[9], double (&t)[3]) {
  double M[9];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) M[3 * a + b] = Mb[3 * a] * R[3 * b] + Mb[3 * a + 1] * R[3 * b + 1] + Mb[3 * a + 2] * R[3 * b + 2];
  t[0] = M[7] - M[5];
  t[1] = M[2] - M[6];
  t[2] = M[3] - M[1];
}

template <bool KIN>
__global__ __launch_bounds__(SENSITIVITY_BLOCK) void sensitivity_rot_kernel(const DevParams* __restrict__ Pg, const long n, const BatchIn in,
                                                                            const SensitivityRotArgs a) {
  for (long base = (long)blockIdx.x * SENSITIVITY_BLOCK; base < n; base += (long)gridDim.x * SENSITIVITY_BLOCK) {
    const long me = base + threadIdx.x;
    const bool live = me < n;
    const long i = live ? me : n - 1;  // tail lanes: the last robot again, nothing stored
    CParams& P = *QC_PARAMS_HERE(Pg);
    RawState S;
    double fp[12], gb[4][3], gbar[4][3], fb[4][3], ba[3];
    fetch_state<4, KIN>(in, i, 0, S, fp);
#pragma unroll
    for (int l = 0; l < 4; l++) {
      load3(a.grf_body, 4 * i + l, gb[l]);
      load3(a.grf_bar, 4 * i + l, gbar[l]);
      load3(a.feet_bar, 4 * i + l, fb[l]);
    }
    load3(a.b_bar, 2 * i + 1, ba);  // (b_lin does not see the rotations: the linear half is not read)
    const double (&R)[9] = S.R;
    const double (&Rd)[9] = S.Rd;
    const double (&wd)[3] = S.wd;

    // the output transform and the lever arms
    double Rb[9];
#pragma unroll
    for (int k = 0; k < 9; k++) Rb[k] = 0.0;
#pragma unroll
    for (int l = 0; l < 4; l++) {
      double p[3] = {fp[3 * l], fp[3 * l + 1], fp[3 * l + 2]};
      if (KIN) {
        const double qa[3] = {p[0], p[1], p[2]};
        leg_fk(P, l, leg_trig(qa), p);
      }
      double rg[3], rbar[3];
      mat_vec(R, gb[l], rg);  // -f_l
      mat_vec(R, fb[l], rbar);
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Rb[3 * r + c] += rg[r] * gbar[l][c] + rbar[r] * p[c];
    }

    // al, as wrench_from_state forms it
    double Re[9], e[3], al[3];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) Re[3 * r + c] = Rd[3 * r] * R[3 * c] + Rd[3 * r + 1] * R[3 * c + 1] + Rd[3 * r + 2] * R[3 * c + 2];
    angle_axis_total(Re, e);
    CParams& Pb = *QC_PARAMS_HERE(Pg);
#pragma unroll
    for (int k = 0; k < 3; k++) al[k] = Pb.kp_w[k] * e[k] + Pb.kd_w[k] * (wd[k] - S.w[k]);
    al[0] += Pb.kff[3] * wd[0];
    al[1] += Pb.kff[4] * wd[1];
    al[1] += Pb.kff[5] * wd[2];  // sic (index 1), as wrench_from_state

    // the inertia: R_bar += ba u1^T + bxw u2^T + al v1^T + wd v2^T
    double bxw[3], t1[3], t2[3], t3[3], t4[3], u1[3], u2[3], v1[3], v2[3];
    cross3(ba, wd, bxw);
    mat_t_vec(R, al, t1);
    mat_t_vec(R, wd, t2);
    mat_t_vec(R, ba, t3);
    mat_t_vec(R, bxw, t4);
    mat_vec(Pb.Ib, t1, u1);
    mat_vec(Pb.Ib, t2, u2);
    mat_t_vec(Pb.Ib, t3, v1);
    mat_t_vec(Pb.Ib, t4, v2);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) Rb[3 * r + c] += (ba[r] * u1[c] + bxw[r] * u2[c]) + (al[r] * v1[c] + wd[r] * v2[c]);

    // the rotation error: e_bar = kp_w o (R v1), Re_bar on the branch the log took
    double alb[3], eb[3], Reb[9], Rdb[9];
    mat_vec(R, v1, alb);
#pragma unroll
    for (int k = 0; k < 3; k++) eb[k] = Pb.kp_w[k] * alb[k];
    angle_axis_total_bwd(Re, eb, Reb);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        Rb[3 * r + c] += Reb[r] * Rd[c] + Reb[3 + r] * Rd[3 + c] + Reb[6 + r] * Rd[6 + c];      // Re_bar^T Rd
        Rdb[3 * r + c] = Reb[3 * r] * R[c] + Reb[3 * r + 1] * R[3 + c] + Reb[3 * r + 2] * R[6 + c];  // Re_bar R
      }

    if (live) {
      if (a.Rwb_bar) {
#pragma unroll
        for (int k = 0; k < 9; k++) a.Rwb_bar[9 * i + k] = Rb[k];
      }
      if (a.Rwb_d_bar) {
#pragma unroll
        for (int k = 0; k < 9; k++) a.Rwb_d_bar[9 * i + k] = Rdb[k];
      }
      if (a.Rwb_rot_bar) {
        double t[3];
        rot_tangent(Rb, R, t);
        store3(a.Rwb_rot_bar, i, t);
      }
      if (a.Rwb_d_rot_bar) {
        double t[3];
        rot_tangent(Rdb, Rd, t);
        store3(a.Rwb_d_rot_bar, i, t);
      }
    }
  }
}

}  // namespace qc
#endif  // __HIPCC__
