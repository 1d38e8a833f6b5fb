// qc_tangent.hpp - forward mode of the balance QP on the active face of a solved point, on the device: given the forces
// qc_control_batch returned and K tangents on the inputs, the K tangents of the forces (qc_tangent_batch, include/qc_tangent.h).
// The face, the reduced matrix M = Z^T H Z + diag(1 - e) and its LDL^T are qc_sensitivity.hpp's, line for line (duplicated, not
// shared, so that sensitivity_kernel stays the kernel it was: DESIGN.md 9e); what is new is the right-hand side and the loop around it.
//
// Per direction, with f_i = -Rwb grf_body_i, v = S (A f - b), delta / delta_d the world-frame left tangents of Rwb / Rwb_d:
//   dp_i = feet_tan_i + J_i joint_q_tan_i (KIN),   dr_i = delta x r_i + Rwb dp_i
//   db_lin = m (kp_p (dx_d - dx) + kd_p (dxdot_d - dxdot) + (kff0 dxdot_d0, kff1 dxdot_d1, 0))
//   de     = Ed delta_d + E delta: the log of Re = Rwb_d Rwb^T along dRe = [delta_d]x Re - Re [delta]x on the branch taken.  Row k of
//            the log's Jacobian is angle_axis_total_bwd(Re, unit_k) (the n2 = 0 limit included), so Ed[k] = axial(J_k Re^T),
//            E[k] = axial(J_k^T Re): two 3x3 matrices, once per robot
//   dal    = kp_w de + kd_w (dw_d - dw) + (kff3 dw_d0, kff4 dw_d1 + kff5 dw_d2, 0)
//   db_ang = Iw (dal - delta x al) + delta x (Iw al) + dw_d x (Iw w_d) + w_d x (delta x (Iw w_d) + Iw (dw_d - delta x w_d))
//            (b_ang = Iw al + w_d x (Iw w_d), dIw = [delta]x Iw - Iw [delta]x)
//   dg_i   = 2 (v_ang x dr_i + q_lin + q_ang x r_i),   q = S (dA f - db),  dA f = (0; sum_i dr_i x f_i)
//   y      = M^-1 (e o Z^T dg) by ldlt_apply against the stored factor,  df = -Z y
//   grf_tan_i = Rwb^T (Z y)_i + Rwb^T (delta x f_i),   b_tan = db
// A pivot that is not positive and finite sets bit 1 of `flags`; every grf_tan and b_tan of the robot is then NaN in all K
// directions.  Non-finite inputs propagate as NaN; nothing is clamped.
//
// Kernel: one lane per robot, FP64, workgroups of one wave, a grid stride once the grid is capped (TANGENT_MAX_BLOCKS workgroups).
// Tail lanes recompute the last robot and store nothing.  Per robot the state, the wrench, the face and the factor are made ONCE
// and stay in registers across a runtime loop over the K directions, which is not unrolled: a pass loads its direction's tangents
// (a NULL array reads as zeros through the same arithmetic), forms the right-hand side, substitutes and stores.  No scratch; the
// cold part of the per-robot state is in LDS (below), the factor and what a pass reads most in registers: profiles/tangent.md.
#pragma once
#include "qc_plant_adjoint.hpp"  // load3_or_zero
#include "qc_sensitivity_rot.hpp"

namespace qc {

// The kernel's argument struct (by value in the kernarg segment, next to the BatchIn the solve takes).
struct TangentArgs {
  const double* grf_body;  // [n][4][3]
  double act_tol;
  long n_dir;  // K
  const double *x_tan, *xdot_tan, *w_tan, *x_d_tan, *xdot_d_tan, *w_d_tan, *Rwb_rot_tan, *Rwb_d_rot_tan;  // [K][n][3], NULL = 0
  const double *feet_tan, *joint_q_tan;  // [K][n][4][3], NULL = 0
  double *grf_tan, *b_tan;               // optional OUT [K][n][4][3], [K][n][6]
  int32_t* flags;                        // optional OUT [n]
};

constexpr int TANGENT_BLOCK = 64;  // one wave
constexpr int TANGENT_MAX_BLOCKS = 4096;
// The cold part of a robot's direction-independent state lives in LDS, one column per lane (plane j of lane t: cold[j][t], no bank
// conflict, no barrier - a lane reads only what it wrote): Iw (9), al, w_d, Iw al, Iw w_d (12), the log's two Jacobians (18), the
// lever arms (12) and v_ang (3), and with joint_q six values per leg (24).  The factor, Rwb and the forces stay in registers.
// 27 KB (feet) / 39 KB (joint_q) per one-wave workgroup: four workgroups per CU (156 of 160 KB), which is what the registers allow anyway.
// With these planes both instantiations need no scratch (404 / 458 registers); with everything in registers they spilled 100 / 492 B.
constexpr int TANGENT_COLD = 54, TANGENT_COLD_KIN = 24;

// robot i of direction k in a direction-major [K][n][m] array: its row (of m values)
#ifdef __HIPCC__
__host__ __device__
#endif
inline long tangent_row(long k, long n, long i) { return k * n + i; }

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

template <bool KIN>
__global__ __launch_bounds__(TANGENT_BLOCK) void tangent_kernel(const DevParams* __restrict__ Pg, const long n, const BatchIn in, const TangentArgs a) {
  __shared__ double cold[TANGENT_COLD + (KIN ? TANGENT_COLD_KIN : 0)][TANGENT_BLOCK];
  const int lane = threadIdx.x;
  for (long base = (long)blockIdx.x * TANGENT_BLOCK; base < n; base += (long)gridDim.x * TANGENT_BLOCK) {
    const long me = base + threadIdx.x;
    const bool live = me < n;
    const long i = live ? me : n - 1;  // tail lanes: the last robot again, nothing stored
    CParams& P = *QC_PARAMS_HERE(Pg);
    RawState S;
    double fp[12], gb[4][3];
    fetch_state<4, KIN>(in, i, 0, S, fp);
#pragma unroll
    for (int l = 0; l < 4; l++) load3(a.grf_body, 4 * i + l, gb[l]);
    const uint32_t mask = load_contact_mask(&P, in.stance, in.gait_phase, in.gait_duty, i, true);
    // the leg Jacobians (kinematics.cpp:162-188, as leg_jt_force spells them), six values per leg: s1, c1, a = jac(0,1), b, and
    // jac(0,2) = l3 c23, l3 s23 - the nine entries are products of these and l1
    if (KIN) {
#pragma unroll
      for (int l = 0; l < 4; l++) {
        const double qa[3] = {fp[3 * l], fp[3 * l + 1], fp[3 * l + 2]};
        const LegTrig t = leg_trig(qa);
        double pb[3];
        leg_fk(P, l, t, pb);  // the foot, exactly as wrench_from_state<4, true> makes it: the wrench below takes it as `feet`
        fp[3 * l] = pb[0]; fp[3 * l + 1] = pb[1]; fp[3 * l + 2] = pb[2];
        CParams& Pk = *QC_PARAMS_HERE(Pg);
        const double l2 = Pk.links[3 * l + 1], l3 = Pk.links[3 * l + 2];
        cold[TANGENT_COLD + 6 * l + 0][lane] = t.s1;
        cold[TANGENT_COLD + 6 * l + 1][lane] = t.c1;
        cold[TANGENT_COLD + 6 * l + 2][lane] = l2 * t.c2 + l3 * t.c23;
        cold[TANGENT_COLD + 6 * l + 3][lane] = l2 * t.s2 + l3 * t.s23;
        cold[TANGENT_COLD + 6 * l + 4][lane] = l3 * t.c23;
        cold[TANGENT_COLD + 6 * l + 5][lane] = l3 * t.s23;
      }
    }

    Wrench<4> W;
    (void)wrench_from_state<4, false>(P, S, fp, 0, W);

    // (made before the face and the factor, so that Rwb_d, w and the joint angles are dead by then)
    // what db needs of the state, once: al as wrench_from_state forms it, Iw = R Ib R^T, Iw al, Iw w_d, and the log's two 3x3 Jacobians
    const double (&R)[9] = S.R;
    const double (&wd)[3] = S.wd;
    {
      double Re[9], al[3], Iw[9], Ia[3], Iwd[3], E[9], Ed[9];
      double er[3];
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Re[3 * r + c] = S.Rd[3 * r] * R[3 * c] + S.Rd[3 * r + 1] * R[3 * c + 1] + S.Rd[3 * r + 2] * R[3 * c + 2];
      angle_axis_total(Re, er);
      CParams& Pb = *QC_PARAMS_HERE(Pg);
#pragma unroll
      for (int k = 0; k < 3; k++) al[k] = Pb.kp_w[k] * er[k] + Pb.kd_w[k] * (wd[k] - S.w[k]);
      al[0] += Pb.kff[3] * wd[0];
      al[1] += Pb.kff[4] * wd[1];
      al[1] += Pb.kff[5] * wd[2];  // sic (index 1), as wrench_from_state
      double T[9];
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) T[3 * r + c] = Pb.Ib[3 * r] * R[3 * c] + Pb.Ib[3 * r + 1] * R[3 * c + 1] + Pb.Ib[3 * r + 2] * R[3 * c + 2];  // Ib R^T
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Iw[3 * r + c] = R[3 * r] * T[c] + R[3 * r + 1] * T[3 + c] + R[3 * r + 2] * T[6 + c];
      mat_vec(Iw, al, Ia);
      mat_vec(Iw, wd, Iwd);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const double ob[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
        double Jk[9], td[3], N[9];
        angle_axis_total_bwd(Re, ob, Jk);
        rot_tangent(Jk, Re, td);  // axial(J_k Re^T)
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
          for (int c = 0; c < 3; c++) N[3 * r + c] = Jk[r] * Re[c] + Jk[3 + r] * Re[3 + c] + Jk[6 + r] * Re[6 + c];  // J_k^T Re
        Ed[3 * k] = td[0]; Ed[3 * k + 1] = td[1]; Ed[3 * k + 2] = td[2];
        E[3 * k] = N[7] - N[5]; E[3 * k + 1] = N[2] - N[6]; E[3 * k + 2] = N[3] - N[1];
      }
#pragma unroll
      for (int j = 0; j < 9; j++) {
        cold[j][lane] = Iw[j];
        cold[21 + j][lane] = E[j];
        cold[30 + j][lane] = Ed[j];
      }
#pragma unroll
      for (int j = 0; j < 3; j++) {
        cold[9 + j][lane] = al[j];
        cold[12 + j][lane] = wd[j];
        cold[15 + j][lane] = Ia[j];
        cold[18 + j][lane] = Iwd[j];
      }
    }
    // f_i = -Rwb grf_body_i;  v = S (A f - b)
    double f[4][3], u[6];
    forces_and_residual(S.R, gb, W, f, u);
    double va[3];
    {
      CParams& Ps = *QC_PARAMS_HERE(Pg);
#pragma unroll
      for (int r = 0; r < 3; r++) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; c++) s += Ps.S[6 * (3 + r) + c] * u[c];
        va[r] = s;
      }
    }

#pragma unroll
    for (int l = 0; l < 4; l++)
#pragma unroll
      for (int c = 0; c < 3; c++) cold[39 + 3 * l + c][lane] = W.r[l][c];
#pragma unroll
    for (int c = 0; c < 3; c++) cold[51 + c][lane] = va[c];

    // the face (qc_sensitivity.hpp): e[j] = coordinate j is a coordinate of y; (tx, ty) = the slopes of a tied fx, fy in the column of fz
    // (across the direction loop the face is ONE word: bit j = e[j], bits 12 + 2 l and 20 + 2 l the codes of tx[l], ty[l] - 1: -mu, 2: +mu)
    bool e[12], flagged = false;
    double tx[4], ty[4];
    uint32_t face = 0;
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
        face |= (e[3 * l] ? 1u : 0u) << (3 * l) | (e[3 * l + 1] ? 1u : 0u) << (3 * l + 1) | (zfree ? 1u : 0u) << (3 * l + 2);
        face |= (zfree ? (uint32_t)cx : 0u) << (12 + 2 * l) | (zfree ? (uint32_t)cy : 0u) << (20 + 2 * l);
      }
    }

    // M = Z^T H Z + diag(1 - e), column by column (qc_sensitivity.hpp), and its factor: unit L, 1 / d on the diagonal
    double M[78];
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
    bool ok;
    {
      double none[12];  // the factorisation alone: a zero right-hand side, whose substitution is dead
#pragma unroll
      for (int k = 0; k < 12; k++) none[k] = 0.0;
      ok = ldlt_solve<12>(M, none);
    }
#pragma unroll
    for (int k = 0; k < 12; k++) {  // the diagonal holds 1 / d_k: positive and finite iff the pivot was
      const double rd = M[k * (k + 1) / 2 + k];
      ok = ok && rd > 0.0 && rd < __builtin_huge_val();
    }
    const double poison = ok ? 0.0 : __builtin_nan("");
    const int flags = (flagged ? 1 : 0) | (ok ? 0 : 2);

#pragma clang loop unroll(disable)
    for (long k = 0; k < a.n_dir; k++) {
      const long row = tangent_row(k, n, i);
      double dx[3], dv[3], dw[3], dxd[3], dvd[3], dwd[3], dl[3], dld[3];
      load3_or_zero(a.x_tan, row, dx);
      load3_or_zero(a.xdot_tan, row, dv);
      load3_or_zero(a.w_tan, row, dw);
      load3_or_zero(a.x_d_tan, row, dxd);
      load3_or_zero(a.xdot_d_tan, row, dvd);
      load3_or_zero(a.w_d_tan, row, dwd);
      load3_or_zero(a.Rwb_rot_tan, row, dl);
      load3_or_zero(a.Rwb_d_rot_tan, row, dld);
      // db, line by line
      CParams& Pb = *QC_PARAMS_HERE(Pg);
      double db[6];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        double da = Pb.kp_p[c] * (dxd[c] - dx[c]) + Pb.kd_p[c] * (dvd[c] - dv[c]);
        if (c < 2) da += Pb.kff[c] * dvd[c];
        db[c] = Pb.mass * da;
      }
      double de[3], dal[3], t1[3], t2[3], c1[3], c2[3], it[3], is[3], c3[3], c4[3], c5[3], c6[3];
      {
        double E[9], Ed[9];
#pragma unroll
        for (int j = 0; j < 9; j++) {
          E[j] = cold[21 + j][lane];
          Ed[j] = cold[30 + j][lane];
        }
        mat_vec(Ed, dld, t1);
        mat_vec(E, dl, t2);
      }
#pragma unroll
      for (int c = 0; c < 3; c++) {
        de[c] = t1[c] + t2[c];
        dal[c] = Pb.kp_w[c] * de[c] + Pb.kd_w[c] * (dwd[c] - dw[c]);
      }
      dal[0] += Pb.kff[3] * dwd[0];
      dal[1] += Pb.kff[4] * dwd[1];
      dal[1] += Pb.kff[5] * dwd[2];
      double Iw[9], al[3], wd[3], Ia[3], Iwd[3];
#pragma unroll
      for (int j = 0; j < 9; j++) Iw[j] = cold[j][lane];
#pragma unroll
      for (int j = 0; j < 3; j++) {
        al[j] = cold[9 + j][lane];
        wd[j] = cold[12 + j][lane];
        Ia[j] = cold[15 + j][lane];
        Iwd[j] = cold[18 + j][lane];
      }
      cross3(dl, al, c1);
      cross3(dl, wd, c2);
#pragma unroll
      for (int c = 0; c < 3; c++) {
        t1[c] = dal[c] - c1[c];
        t2[c] = dwd[c] - c2[c];
      }
      mat_vec(Iw, t1, it);
      mat_vec(Iw, t2, is);
      cross3(dl, Ia, c3);
      cross3(dwd, Iwd, c4);
      cross3(dl, Iwd, c5);
#pragma unroll
      for (int c = 0; c < 3; c++) c5[c] += is[c];
      cross3(wd, c5, c6);
#pragma unroll
      for (int c = 0; c < 3; c++) db[3 + c] = (it[c] + c3[c]) + (c4[c] + c6[c]);

      // dr_i, dA f, q = S (dA f - db)
      double dr[4][3], ua[3] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int l = 0; l < 4; l++) {  // (leg by leg, loads included: the eight state tangents are dead by now, all but delta)
        double dp[3];
        load3_or_zero(a.feet_tan, 4 * row + l, dp);
        if (KIN) {
          double dq[3];
          load3_or_zero(a.joint_q_tan, 4 * row + l, dq);
          CParams& Pk = *QC_PARAMS_HERE(Pg);
          const double (&J)[6] = {cold[TANGENT_COLD + 6 * l][lane],     cold[TANGENT_COLD + 6 * l + 1][lane], cold[TANGENT_COLD + 6 * l + 2][lane],
                                  cold[TANGENT_COLD + 6 * l + 3][lane], cold[TANGENT_COLD + 6 * l + 4][lane], cold[TANGENT_COLD + 6 * l + 5][lane]};
          const double l1 = Pk.links[3 * l], s1 = J[0], c1 = J[1], ja = J[2];
          const double t = J[3] * dq[1] + J[5] * dq[2];  // rows 1 and 2 share it: (j11, j12) = s1 (b, l3 s23), (j21, j22) = -c1 (b, l3 s23)
          dp[0] += ja * dq[1] + J[4] * dq[2];
          dp[1] += (-l1 * s1 - ja * c1) * dq[0] + s1 * t;
          dp[2] += (l1 * c1 - ja * s1) * dq[0] - c1 * t;
        }
        double rp[3], cr[3], m[3];
        const double rl[3] = {cold[39 + 3 * l][lane], cold[40 + 3 * l][lane], cold[41 + 3 * l][lane]};
        cross3(dl, rl, cr);
        mat_vec(R, dp, rp);
#pragma unroll
        for (int c = 0; c < 3; c++) dr[l][c] = cr[c] + rp[c];
        cross3(dr[l], f[l], m);
#pragma unroll
        for (int c = 0; c < 3; c++) ua[c] += m[c];
      }
      const double du[6] = {-db[0], -db[1], -db[2], ua[0] - db[3], ua[1] - db[4], ua[2] - db[5]};
      double qs[6];
      {
        CParams& Ps = *QC_PARAMS_HERE(Pg);
#pragma unroll
        for (int r = 0; r < 6; r++) {
          double s = 0.0;
#pragma unroll
          for (int c = 0; c < 6; c++) s += Ps.S[6 * r + c] * du[c];
          qs[r] = s;
        }
      }
      const double qa[3] = {qs[3], qs[4], qs[5]};
      // y = e o Z^T dg, substituted against the factor
      double y[12];
      const double mu = Pb.mu;
      const uint32_t fc = face;
      const auto on = [fc](int j) { return (fc & (1u << j)) != 0; };
      const auto slope = [fc, mu](int at) { return (fc & (1u << at)) ? -mu : ((fc & (2u << at)) ? mu : 0.0); };
#pragma unroll
      for (int l = 0; l < 4; l++) {
        double g1[3], g2[3], dg[3];
        const double rl[3] = {cold[39 + 3 * l][lane], cold[40 + 3 * l][lane], cold[41 + 3 * l][lane]};
        const double vl[3] = {cold[51][lane], cold[52][lane], cold[53][lane]};
        cross3(vl, dr[l], g1);
        cross3(qa, rl, g2);
#pragma unroll
        for (int c = 0; c < 3; c++) dg[c] = 2.0 * (g1[c] + (qs[c] + g2[c]));
        y[3 * l] = on(3 * l) ? dg[0] : 0.0;
        y[3 * l + 1] = on(3 * l + 1) ? dg[1] : 0.0;
        y[3 * l + 2] = on(3 * l + 2) ? dg[2] + slope(12 + 2 * l) * dg[0] + slope(20 + 2 * l) * dg[1] : 0.0;
      }
      ldlt_apply<12>(M, y);

      if (live) {
        double* const grf_tan = a.grf_tan;
        double* const b_tan = a.b_tan;
        if (grf_tan) {
#pragma unroll
          for (int l = 0; l < 4; l++) {
            // -df_l = (Z y)_l, and the output transform's own term delta x f_l
            const double yz = on(3 * l + 2) ? y[3 * l + 2] : 0.0;
            double cf[3], wv[3], gt[3];
            cross3(dl, f[l], cf);
            wv[0] = (((on(3 * l) ? y[3 * l] : 0.0) + slope(12 + 2 * l) * yz) + cf[0]) + poison;
            wv[1] = (((on(3 * l + 1) ? y[3 * l + 1] : 0.0) + slope(20 + 2 * l) * yz) + cf[1]) + poison;
            wv[2] = (yz + cf[2]) + poison;
            mat_t_vec(R, wv, gt);
            store3(grf_tan, 4 * row + l, gt);
          }
        }
        if (b_tan) {
          const double lo[3] = {db[0] + poison, db[1] + poison, db[2] + poison}, hi[3] = {db[3] + poison, db[4] + poison, db[5] + poison};
          store3(b_tan, 2 * row, lo);
          store3(b_tan, 2 * row + 1, hi);
        }
      }
    }
    if (live && a.flags) a.flags[i] = flags;
  }
}

}  // namespace qc
#endif  // __HIPCC__
