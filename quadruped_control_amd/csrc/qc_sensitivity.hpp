// qc_sensitivity.hpp - the adjoint of the balance QP on the active face of a solved point, on the device: given the forces
// qc_control_batch returned and a cotangent on them, the cotangents of the inputs the forces depend on through the wrench target b
// and the lever arms r_i (qc_sensitivity_batch, include/qc_balance.h).  One kernel next to the certificate, whose row
// classification (classify_foot, qc_certify.hpp) defines the face, from grf_body alone and whatever form the solver ran.
//
// Per robot the solve minimises phi(f) = (A f - b)^T S (A f - b) + f^T W f over the world-frame forces f (12 values) under the
// pyramid rows qc_certify.hpp documents; A = [I I I I; [r_1]x ... [r_4]x], r_i = Rwb p_i, b from the PD law, the handle's full S
// (6x6) and W (12x12).  H = 2 (A^T S A + W) is the Hessian, g = 2 (A^T S (A f - b) + W f) the gradient.
//
// The face.  Each stance foot's axes are classified at act_tol (codes 0 none, 1 lower, 2 upper, 3 both), and on the face f = Z y + f0:
//   z code != 0          fz is pinned;          z code 0: fz is a coordinate of y
//   x (y) code 0         fx (fy) is a coordinate of y
//   x (y) code 1 or 2    fx = -mu fz (1) or +mu fz (2): tied to fz where fz is free - the column of fz in Z carries -+mu in that row -,
//                        pinned where fz is
//   a code 3 on any axis the whole foot is pinned and bit 0 of `flags` is set: the derivative is one-sided there
//   swing feet           pinned
// A failed robot has all-zero forces: every stance foot classifies as pinned and flagged, its adjoint is 0 - no special case.
//
// The adjoint.  On the face Z^T g = 0; differentiating at fixed Z and f0, df = -Z (Z^T H Z)^-1 Z^T (dg/dtheta) dtheta, so with
//   f_bar = -Rwb grf_bar                      (grf_body_i = -Rwb^T f_i, Rwb held fixed)
//   z     = Z (Z^T H Z)^-1 Z^T f_bar          the adjoint force: world frame, 12 values, 0 in pinned coordinates
// every cotangent is -<z, dg/dtheta>:
//   b_bar      = 2 S A z                      (dg/db = -2 A^T S)
//   r_bar_i    = -2 (z_i x v_ang + f_i x q_ang),  v = S (A f - b),  q = S A z   (dA enters g twice: dA^T v and A^T S dA f)
//   feet_bar_i = Rwb^T r_bar_i                the cotangent of the body-frame foot position p_i, whether p_i came from `feet` or
//                                             from the forward kinematics of joint_q
//   x_bar ... w_d_bar                         b_bar pulled back through wrench_from_state (qc_device.hpp) at fixed Rwb and Rwb_d,
//                                             line by line, its kff lines included: b_lin = m (kp_p (x_d - x) + kd_p (xdot_d - xdot)
//                                             + kff[0..1] xdot_d[0..1] + const), b_ang = Iw al + w_d x (Iw w_d) with al = kp_w e +
//                                             kd_w (w_d - w) + (kff[3] w_d[0], kff[4] w_d[1] + kff[5] w_d[2], 0), Iw = Rwb Ib Rwb^T:
//                                             with al_bar = Iw^T b_bar_ang,  w_bar = -kd_w al_bar,  w_d_bar = kd_w al_bar +
//                                             (kff[3] al_bar[0], kff[4] al_bar[1], kff[5] al_bar[1]) + (Iw w_d) x b_bar_ang +
//                                             Iw^T (b_bar_ang x w_d)
// NOT produced: the cotangents of Rwb and Rwb_d (qc_sensitivity_rot.hpp makes them from b_bar and feet_bar, in a kernel of its own); the
// weak activity - a row whose multiplier is about 0 is on the face like any other active row (the caller has the certificate's lambda
// for that).  The cotangents of the handle's parameters (mu, fzmin, fzmax, the weights, the gains, mass, Ib) come from
// qc_sensitivity_params.hpp, from the adjoint written here, in a kernel of its own.  Commander mode is out of scope, as for the certificate.
//
// The reduced solve is branch-free: with e_j = 1 for a coordinate of y and 0 for a pinned or tied one, the fixed 12x12 system
// M = Z^T H Z (rows and columns with e = 1) + diag(1 - e), rhs e o Z^T f_bar - the pinned coordinates are identity rows selected
// in, never multiplied in, so a NaN behind a pinned coordinate stays out - factorised by ldlt_solve<12> (fully unrolled, statically
// indexed: the 78-entry triangle lives in VGPRs, no LDS, no scratch).  A pivot that is not positive and finite sets bit 1 of
// `flags` and every output of the robot is NaN.  Non-finite inputs propagate as NaN; nothing is clamped.
//
// Kernel: one lane per robot, FP64, workgroups of one wave, a grid stride once the grid is capped (SENSITIVITY_MAX_BLOCKS
// workgroups, above 262 144 robots).  Tail lanes recompute the last robot and store nothing.  `in` is never written.
#pragma once
#include "qc_certify.hpp"

namespace qc {

// The kernel's argument struct (by value in the kernarg segment, next to the BatchIn the solve takes).
struct SensitivityArgs {
  const double *grf_body, *grf_bar;  // [n][4][3]
  double act_tol;
  double *adjoint, *b_bar, *feet_bar;                              // optional OUT [n][12], [n][6], [n][4][3]
  double *x_bar, *xdot_bar, *w_bar, *x_d_bar, *xdot_d_bar, *w_d_bar;  // optional OUT [n][3]
  int32_t* flags;                                                  // optional OUT [n]
};

constexpr int SENSITIVITY_BLOCK = 64;  // one wave
constexpr int SENSITIVITY_MAX_BLOCKS = 4096;

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

template <bool KIN>
__global__ __launch_bounds__(SENSITIVITY_BLOCK) void sensitivity_kernel(const DevParams* __restrict__ Pg, const long n, const BatchIn in,
                                                                        const SensitivityArgs a) {
  for (long base = (long)blockIdx.x * SENSITIVITY_BLOCK; base < n; base += (long)gridDim.x * SENSITIVITY_BLOCK) {
    const long me = base + threadIdx.x;
    const bool live = me < n;
    const long i = live ? me : n - 1;  // tail lanes: the last robot again, nothing stored
    CParams& P = *QC_PARAMS_HERE(Pg);
    RawState S;
    double fp[12], gb[4][3], gbar[4][3];
    fetch_state<4, KIN>(in, i, 0, S, fp);
#pragma unroll
    for (int l = 0; l < 4; l++) {
      load3(a.grf_body, 4 * i + l, gb[l]);
      load3(a.grf_bar, 4 * i + l, gbar[l]);
    }
    const uint32_t mask = load_contact_mask(&P, in.stance, in.gait_phase, in.gait_duty, i, true);
    Wrench<4> W;
    (void)wrench_from_state<4, KIN>(P, S, fp, 0, W);

    // f_i = -Rwb grf_body_i, f_bar_i = -Rwb grf_bar_i;  v = S (A f - b)
    double f[4][3], fbar[4][3], u[6];
    forces_and_residual(S.R, gb, W, f, u);
#pragma unroll
    for (int l = 0; l < 4; l++) {
      double rb[3];
      mat_vec(S.R, gbar[l], rb);
#pragma unroll
      for (int k = 0; k < 3; k++) fbar[l][k] = -rb[k];
    }
    double v[6];
    {
      CParams& Ps = *QC_PARAMS_HERE(Pg);
#pragma unroll
      for (int r = 0; r < 6; r++) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; c++) s += Ps.S[6 * r + c] * u[c];
        v[r] = s;
      }
    }

    // the face: e[j] = coordinate j of the force is a coordinate of y; (tx, ty) = the slopes of a tied fx, fy in the column of fz
    bool e[12], flagged = false;
    double tx[4], ty[4];
    {
      CParams& Pc = *QC_PARAMS_HERE(Pg);
      const double mu = Pc.mu, fzmin = Pc.fzmin, fzmax = Pc.fzmax;
#pragma unroll
      for (int l = 0; l < 4; l++) {
        double viol;
        int cx, cy, cz;
        classify_foot(mu, fzmin, fzmax, a.act_tol, f[l][0], f[l][1], f[l][2], viol, cx, cy, cz);
        const bool stance = (mask & (1u << l)) != 0;
        const bool both = stance && (cx == 3 || cy == 3 || cz == 3);
        const bool moves = stance && !both;
        const bool zfree = moves && cz == 0;
        flagged = flagged || both;
        e[3 * l] = moves && cx == 0;
        e[3 * l + 1] = moves && cy == 0;
        e[3 * l + 2] = zfree;
        tx[l] = (zfree && cx != 0) ? (cx == 1 ? -mu : mu) : 0.0;
        ty[l] = (zfree && cy != 0) ? (cy == 1 ? -mu : mu) : 0.0;
      }
    }

    // M = Z^T H Z + diag(1 - e), column by column: column c of Z is d = (1,0,0), (0,1,0) or (tx, ty, 1) in the rows of its foot;
    // H d = 2 (A^T (S (A d)) + W d) for the feet from that one on, and row r of the triangle is the r-th column of Z against it
    double M[78], y[12];
#pragma unroll
    for (int c = 0; c < 12; c++) {
      const int lc = c / 3, kc = c % 3;
      const double d[3] = {kc == 0 ? 1.0 : (kc == 2 ? tx[lc] : 0.0), kc == 1 ? 1.0 : (kc == 2 ? ty[lc] : 0.0), kc == 2 ? 1.0 : 0.0};
      double ad[3], sa[6];
      cross3(W.r[lc], d, ad);
      CParams& Pw = *QC_PARAMS_HERE(Pg);  // one column at a time: the scalar loads of S and W stay next to their use
#pragma unroll
      for (int r = 0; r < 6; r++)
        sa[r] = Pw.S[6 * r] * d[0] + Pw.S[6 * r + 1] * d[1] + Pw.S[6 * r + 2] * d[2] + Pw.S[6 * r + 3] * ad[0] + Pw.S[6 * r + 4] * ad[1] +
                Pw.S[6 * r + 5] * ad[2];
      const double sl[3] = {sa[0], sa[1], sa[2]}, sg[3] = {sa[3], sa[4], sa[5]};
#pragma unroll
      for (int l = lc; l < 4; l++) {
        double cr[3], hz[3];
        cross3(sg, W.r[l], cr);
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const int row = 12 * (3 * l + k) + 3 * lc;
          const double wd = Pw.W[row] * d[0] + Pw.W[row + 1] * d[1] + Pw.W[row + 2] * d[2];
          hz[k] = 2.0 * ((sl[k] + cr[k]) + wd);
        }
        const double rows[3] = {hz[0], hz[1], hz[2] + tx[l] * hz[0] + ty[l] * hz[1]};
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const int r = 3 * l + k;
          if (r >= c) M[r * (r + 1) / 2 + c] = (e[r] && e[c]) ? rows[k] : (r == c ? 1.0 : 0.0);
        }
      }
    }
#pragma unroll
    for (int l = 0; l < 4; l++) {
      y[3 * l] = e[3 * l] ? fbar[l][0] : 0.0;
      y[3 * l + 1] = e[3 * l + 1] ? fbar[l][1] : 0.0;
      y[3 * l + 2] = e[3 * l + 2] ? fbar[l][2] + tx[l] * fbar[l][0] + ty[l] * fbar[l][1] : 0.0;
    }
    bool ok = ldlt_solve<12>(M, y);
#pragma unroll
    for (int k = 0; k < 12; k++) {  // the diagonal holds 1 / d_k: positive and finite iff the pivot was
      const double rd = M[k * (k + 1) / 2 + k];
      ok = ok && rd > 0.0 && rd < __builtin_huge_val();
    }
    const double poison = ok ? 0.0 : __builtin_nan("");

    // z = Z y
    double z[4][3];
#pragma unroll
    for (int l = 0; l < 4; l++) {
      const double yz = e[3 * l + 2] ? y[3 * l + 2] : 0.0;
      z[l][0] = ((e[3 * l] ? y[3 * l] : 0.0) + tx[l] * yz) + poison;
      z[l][1] = ((e[3 * l + 1] ? y[3 * l + 1] : 0.0) + ty[l] * yz) + poison;
      z[l][2] = yz + poison;
    }
    // q = S A z, b_bar = 2 q
    double az[6], q[6], bb[6];
#pragma unroll
    for (int k = 0; k < 6; k++) az[k] = 0.0;
#pragma unroll
    for (int l = 0; l < 4; l++) {
      double m[3];
      cross3(W.r[l], z[l], m);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        az[k] += z[l][k];
        az[3 + k] += m[k];
      }
    }
    {
      CParams& Ps = *QC_PARAMS_HERE(Pg);
#pragma unroll
      for (int r = 0; r < 6; r++) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; c++) s += Ps.S[6 * r + c] * az[c];
        q[r] = s;
        bb[r] = 2.0 * s;
      }
    }
    const int flags = (flagged ? 1 : 0) | (ok ? 0 : 2);

    if (live) {
      if (a.adjoint) {
#pragma unroll
        for (int l = 0; l < 4; l++) store3(a.adjoint, 4 * i + l, z[l]);
      }
      if (a.b_bar) {
        const double lo[3] = {bb[0], bb[1], bb[2]}, hi[3] = {bb[3], bb[4], bb[5]};
        store3(a.b_bar, 2 * i, lo);
        store3(a.b_bar, 2 * i + 1, hi);
      }
      if (a.feet_bar) {
        const double va[3] = {v[3], v[4], v[5]}, qa[3] = {q[3], q[4], q[5]};
#pragma unroll
        for (int l = 0; l < 4; l++) {
          double c1[3], c2[3], rbar[3], pbar[3];
          cross3(z[l], va, c1);
          cross3(f[l], qa, c2);
#pragma unroll
          for (int k = 0; k < 3; k++) rbar[k] = -2.0 * (c1[k] + c2[k]);
          mat_t_vec(S.R, rbar, pbar);
          store3(a.feet_bar, 4 * i + l, pbar);
        }
      }
      // b_bar pulled back through wrench_from_state, line by line (Rwb, Rwb_d fixed)
      CParams& Pb = *QC_PARAMS_HERE(Pg);
      if (a.x_bar || a.x_d_bar || a.xdot_bar || a.xdot_d_bar) {
        double xb[3], xdb[3], vb[3], vdb[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const double ab = Pb.mass * bb[k];  // b_lin = mass a (+ const)
          xdb[k] = Pb.kp_p[k] * ab;
          xb[k] = -xdb[k];
          vb[k] = -(Pb.kd_p[k] * ab);
          vdb[k] = k < 2 ? (Pb.kd_p[k] + Pb.kff[k]) * ab : Pb.kd_p[k] * ab;  // a[0], a[1] += kff xdot_d
        }
        if (a.x_bar) store3(a.x_bar, i, xb);
        if (a.x_d_bar) store3(a.x_d_bar, i, xdb);
        if (a.xdot_bar) store3(a.xdot_bar, i, vb);
        if (a.xdot_d_bar) store3(a.xdot_d_bar, i, vdb);
      }
      if (a.w_bar || a.w_d_bar) {
        // b_ang = Iw al + wd x (Iw wd), Iw = R Ib R^T: al_bar = Iw^T ba, wd_bar = (Iw wd) x ba + Iw^T (ba x wd) + what al carries
        const double ba[3] = {bb[3], bb[4], bb[5]};
        double bxw[3], t1[3], t2[3], t3[3], u1[3], u2[3], u3[3], alb[3], itb[3], iw[3], cxb[3];
        cross3(ba, S.wd, bxw);
        mat_t_vec(S.R, ba, t1);
        mat_t_vec(S.R, bxw, t2);
        mat_t_vec(S.R, S.wd, t3);
        mat_t_vec(Pb.Ib, t1, u1);
        mat_t_vec(Pb.Ib, t2, u2);
        mat_vec(Pb.Ib, t3, u3);
        mat_vec(S.R, u1, alb);
        mat_vec(S.R, u2, itb);
        mat_vec(S.R, u3, iw);
        cross3(iw, ba, cxb);
        double wb[3], wdb[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
          wb[k] = -(Pb.kd_w[k] * alb[k]);
          wdb[k] = Pb.kd_w[k] * alb[k] + (cxb[k] + itb[k]);
        }
        wdb[0] += Pb.kff[3] * alb[0];
        wdb[1] += Pb.kff[4] * alb[1];
        wdb[2] += Pb.kff[5] * alb[1];  // al[1] += kff[5] wd[2]
        if (a.w_bar) store3(a.w_bar, i, wb);
        if (a.w_d_bar) store3(a.w_d_bar, i, wdb);
      }
      if (a.flags) a.flags[i] = flags;
    }
  }
}

}  // namespace qc
#endif  // __HIPCC__
