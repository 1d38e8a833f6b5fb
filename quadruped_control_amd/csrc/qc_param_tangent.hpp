// qc_param_tangent.hpp - forward mode of the balance QP in the handle's own parameters, on the device: given the forces
// qc_control_batch returned and K directions in the 211 doubles of qc_params (PARAM_COUNT, qc_sensitivity_params.hpp: mu, mass, fzmin,
// fzmax, Ib, S, W, kff, kp_p, kd_p, kp_w, kd_w - matrices entrywise and row-major, NOT symmetrised), the K tangents of the forces
// (qc_param_tangent_batch, include/qc_tangent.h).  The transpose of sensitivity_param_kernel: <grf_bar, grf_tan_k> per robot equals
// <that kernel's row for grf_bar, param_tan_k>.  The face, the reduced matrix and its LDL^T are tangent_kernel's, line for line
// (param_tangent_face_factor, below) - this launch repeats that call's factorisation, once per robot -, the substitution is
// ldlt_apply, the gradient g is hessian_like (qc_sensitivity_params.hpp); what is new is the right-hand side.
//
// In the notation of qc_sensitivity_params.hpp - f the world forces, u = A f - b, v = S u, g = 2 (A^T v + W f), H = 2 (A^T S A + W),
// sx, sy in {-1, 0, +1} from the x / y codes of a foot that moves (stance, no code 3) - per direction (dmu, dmass, dfzmin, ...):
//   da     = dkp_p o (x_d - x) + dkd_p o (xdot_d - xdot) + (dkff0 xdot_d0, dkff1 xdot_d1, dkff2 mass 9.81 + kff2 dmass 9.81)
//   db_lin = dmass (a - (0, 0, 9.81)) + mass da                 (mass three times: the factor, the gravity term, inside a_z)
//   dal    = dkp_w o e + dkd_w o (w_d - w) + (dkff3 w_d0, dkff4 w_d1 + dkff5 w_d2, 0)      (kff[5] on the second component)
//   db_ang = Iw dal + dIw al + w_d x (dIw w_d),   Iw x = R (Ib (R^T x)),  dIw x = R (dIb (R^T x))
//   df0_l  = (sx (dmu f_lz + mu dlim), sy (dmu f_lz + mu dlim), dlim)   dlim = 0 / dfzmin / dfzmax for z code 0 / 1 / 2: the motion
//            of the foot at fixed free coordinates (f_lz is the limit itself at a z code 1 or 2, to act_tol; the adjoint reads f_lz
//            there and so does this)
//   s      = S (A df0 - db) + dS u
//   dg_l   = 2 (s_lin + s_ang x r_l + (W df0 + dW f)_l)         = H df0 + 2 (A^T dS u + dW f - A^T S db)
//   rhs    = e o Z^T dg, and on the z column of a foot with fz free + dmu (sx g_lx + sy g_ly)      (the column itself moves)
//   y      = M^-1 rhs,   df = df0 - Z y,   grf_tan_l = -Rwb^T df_l (+ grf_tan_in),   b_tan = db (+ b_tan_in).
// A pivot that is not positive and finite sets bit 1 of `flags`; every grf_tan and b_tan of the robot is then NaN in all K
// directions, whatever grf_tan_in holds.  A robot whose face is empty at zero forces (a failed robot, an all-swing robot) gets
// grf_tan = R^T 0 (+ grf_tan_in): exact zeros, or grf_tan_in's numbers (gi + 0: only a -0.0 may come back as +0.0).  Non-finite
// inputs propagate; nothing is clamped.
//
// Kernel: tangent_kernel's shape - one lane per robot, FP64, workgroups of one wave, a grid stride beyond PARAM_TANGENT_MAX_BLOCKS
// workgroups, tail lanes recompute the last robot and store nothing, a runtime loop over the K directions that is not unrolled.
// param_tan is SHARED by the batch: a direction's 211 values are wave-uniform and are read through the constant address space
// (scalar loads into SGPRs, next to their use, as the handle's parameters are) - no lane holds a copy.  The factor, Rwb and the
// forces stay in registers; the rest of the per-robot state is in LDS, one column per lane (no bank conflict, no barrier - a lane
// reads only what it wrote).  A (direction, robot) pair reads grf_tan_in / b_tan_in before it writes: each may BE the output.
// 0 B of scratch: profiles/param_tangent.md.
#pragma once
#include "qc_sensitivity_params.hpp"  // PARAM_COUNT, hessian_like
#include "qc_tangent.hpp"             // tangent_row

namespace qc {

// The kernel's argument struct (by value in the kernarg segment, next to the BatchIn the solve takes).
struct ParamTangentArgs {
  const double* grf_body;  // [n][4][3]
  double act_tol;
  long n_dir;                            // K
  const double* param_tan;               // [K][PARAM_COUNT], shared by the batch; never written by the launch
  const double *grf_tan_in, *b_tan_in;   // optional [K][n][4][3], [K][n][6]: added
  double *grf_tan, *b_tan;               // optional OUT [K][n][4][3], [K][n][6]
  int32_t* flags;                        // optional OUT [n]
};

constexpr int PARAM_TANGENT_BLOCK = 64;  // one wave
constexpr int PARAM_TANGENT_MAX_BLOCKS = 4096;
// the per-robot state in LDS (plane j of lane t: cold[j][t]): the lever arms (12), u (6), a - (0, 0, 9.81) (3), x_d - x, xdot_d - xdot
// (6), the rotation error e (3), w_d - w (3), w_d (3), R^T al, R^T w_d (6), sx g_lx + sy g_ly of the feet with fz free (4), xdot_d0,
// xdot_d1 (2): 24 KB per one-wave workgroup
constexpr int PARAM_TANGENT_COLD = 48;
// where the groups start in a row of param_tan (PARAM_LAYOUT's order)
constexpr int PT_MU = 0, PT_MASS = 1, PT_FZMIN = 2, PT_FZMAX = 3, PT_IB = 4, PT_S = 13, PT_W = 49, PT_KFF = 193, PT_KP_P = 199, PT_KD_P = 202, PT_KP_W = 205,
              PT_KD_W = 208;
static_assert(PT_KD_W + 3 == PARAM_COUNT, "the groups fill the row");

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

// a wave-uniform row of doubles read through the constant address space (scalar loads), the pointer re-derived next to its use
typedef const __attribute__((address_space(4))) double CDouble;
#define QC_ROW_HERE(ptr)                  \
  ({                                      \
    const double* r_ = (ptr);             \
    asm volatile("" : "+s"(r_));         \
    (CDouble*)(unsigned long long)r_;     \
  })

// The face of a solved point and the factor of its reduced system: `face` (bit j = e[j], bits 12 + 2 l and 20 + 2 l the codes of
// tx[l], ty[l] - 1: -mu, 2: +mu), `flagged` (a code 3 foot: bit 0 of the flags), M = the LDL^T of Z^T H Z + diag(1 - e) and `ok`
// (every pivot positive and finite).  tangent_kernel's lines (qc_tangent.hpp), DUPLICATED: taken out of that kernel into a function
// both call, its instruction stream moved (12 / 38 instructions of its two instantiations), so it keeps its lines and this file has
// a copy, as qc_tangent.hpp has of qc_sensitivity.hpp's.  classify_foot, ldlt_solve and ldlt_apply are shared.
QC_DEV void param_tangent_face_factor(const DevParams* Pg, const double act_tol, const uint32_t mask, const double (&f)[4][3], const Wrench<4>& W,
                                      double (&M)[78], uint32_t& face, bool& flagged, bool& ok) {
  bool e[12];
  double tx[4], ty[4];
  flagged = false;
  face = 0;
  {
    CParams& Pc = *QC_PARAMS_HERE(Pg);
    const double mu = Pc.mu, fzmin = Pc.fzmin, fzmax = Pc.fzmax;
#pragma unroll
    for (int l = 0; l < 4; l++) {
      double viol;
      int cx, cy, cz;
      classify_foot(mu, fzmin, fzmax, act_tol, f[l][0], f[l][1], f[l][2], viol, cx, cy, cz);
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
  // M = Z^T H Z + diag(1 - e), column by column, and its factor: unit L, 1 / d on the diagonal
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
}

template <bool KIN>
__global__ __launch_bounds__(PARAM_TANGENT_BLOCK) void param_tangent_kernel(const DevParams* __restrict__ Pg, const long n, const BatchIn in,
                                                                            const ParamTangentArgs a) {
  __shared__ double cold[PARAM_TANGENT_COLD][PARAM_TANGENT_BLOCK];
  const int lane = threadIdx.x;
  for (long base = (long)blockIdx.x * PARAM_TANGENT_BLOCK; base < n; base += (long)gridDim.x * PARAM_TANGENT_BLOCK) {
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
    Wrench<4> W;
    (void)wrench_from_state<4, KIN>(P, S, fp, 0, W);
    const double (&R)[9] = S.R;

    // what db needs of the state, once: the PD law's factors as wrench_from_state forms them
    {
      CParams& Pb = *QC_PARAMS_HERE(Pg);
      double ex[3], ev[3], ag[3], Re[9], er[3], dwv[3], al[3], t1[3], t2[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        ex[k] = S.xd[k] - S.x[k];
        ev[k] = S.xdotd[k] - S.xdot[k];
        ag[k] = Pb.kp_p[k] * ex[k] + Pb.kd_p[k] * ev[k];
      }
      ag[0] += Pb.kff[0] * S.xdotd[0];
      ag[1] += Pb.kff[1] * S.xdotd[1];
      ag[2] += Pb.kff[2] * Pb.mass * 9.81;
      ag[2] -= 9.81;
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Re[3 * r + c] = S.Rd[3 * r] * R[3 * c] + S.Rd[3 * r + 1] * R[3 * c + 1] + S.Rd[3 * r + 2] * R[3 * c + 2];
      angle_axis_total(Re, er);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        dwv[k] = S.wd[k] - S.w[k];
        al[k] = Pb.kp_w[k] * er[k] + Pb.kd_w[k] * dwv[k];
      }
      al[0] += Pb.kff[3] * S.wd[0];
      al[1] += Pb.kff[4] * S.wd[1];
      al[1] += Pb.kff[5] * S.wd[2];  // sic (index 1), as wrench_from_state
      mat_t_vec(R, al, t1);
      mat_t_vec(R, S.wd, t2);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        cold[18 + k][lane] = ag[k];
        cold[21 + k][lane] = ex[k];
        cold[24 + k][lane] = ev[k];
        cold[27 + k][lane] = er[k];
        cold[30 + k][lane] = dwv[k];
        cold[33 + k][lane] = S.wd[k];
        cold[36 + k][lane] = t1[k];
        cold[39 + k][lane] = t2[k];
      }
      cold[46][lane] = S.xdotd[0];
      cold[47][lane] = S.xdotd[1];
    }

    // f_l = -Rwb grf_body_l, u = A f - b;  v = S u;  g = 2 (A^T v + W f)
    double f[4][3], u[6];
    uint32_t codes = 0;
    forces_and_residual(R, gb, W, f, u);
#pragma unroll
    for (int l = 0; l < 4; l++)
#pragma unroll
      for (int c = 0; c < 3; c++) cold[3 * l + c][lane] = W.r[l][c];
#pragma unroll
    for (int c = 0; c < 6; c++) cold[12 + c][lane] = u[c];
    {
      double v[6], g[4][3];
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
      hessian_like(Pg, v, W, f, g);
      // one pass over the feet for what the face word (below) does not say: sx g_lx + sy g_ly where the column of fz moves with mu (a
      // foot that moves with fz free), and of a foot that moves its x and y codes whatever fz does (bits 2 l, 8 + 2 l) and its z code
      // (bits 16 + 2 l).  A foot that does not move has all three at 0: its df0 is 0.
      CParams& Pc = *QC_PARAMS_HERE(Pg);
      const double mu = Pc.mu, fzmin = Pc.fzmin, fzmax = Pc.fzmax;
#pragma unroll
      for (int l = 0; l < 4; l++) {
        double viol;
        int cx, cy, cz;
        classify_foot(mu, fzmin, fzmax, a.act_tol, f[l][0], f[l][1], f[l][2], viol, cx, cy, cz);
        const bool moves = (mask & (1u << l)) != 0 && !(cx == 3 || cy == 3 || cz == 3);
        const double sx = cx == 1 ? -1.0 : (cx == 2 ? 1.0 : 0.0), sy = cy == 1 ? -1.0 : (cy == 2 ? 1.0 : 0.0);
        cold[42 + l][lane] = (moves && cz == 0) ? sx * g[l][0] + sy * g[l][1] : 0.0;
        codes |= (moves ? (uint32_t)cx : 0u) << (2 * l) | (moves ? (uint32_t)cy : 0u) << (8 + 2 * l) | (moves ? (uint32_t)cz : 0u) << (16 + 2 * l);
      }
    }

    // the face and the factor of the reduced system
    double M[78];
    uint32_t face;
    bool flagged, ok;
    param_tangent_face_factor(Pg, a.act_tol, mask, f, W, M, face, flagged, ok);
    const double poison = ok ? 0.0 : __builtin_nan("");
    const int flags = (flagged ? 1 : 0) | (ok ? 0 : 2);

#pragma clang loop unroll(disable)
    for (long k = 0; k < a.n_dir; k++) {
      const long row = tangent_row(k, n, i);
      const double* const th = a.param_tan + k * PARAM_COUNT;
      const uint32_t cd = codes;
      const auto sign = [cd](int at) { return (cd & (1u << at)) ? -1.0 : ((cd & (2u << at)) ? 1.0 : 0.0); };
      // db, line by line
      double db[6];
      {
        CParams& Pb = *QC_PARAMS_HERE(Pg);
        CDouble* const t = QC_ROW_HERE(th);
        const double mass = Pb.mass, dmass = t[PT_MASS];
        double da[3], dal[3];
#pragma unroll
        for (int c = 0; c < 3; c++) da[c] = t[PT_KP_P + c] * cold[21 + c][lane] + t[PT_KD_P + c] * cold[24 + c][lane];
        da[0] += t[PT_KFF] * cold[46][lane];
        da[1] += t[PT_KFF + 1] * cold[47][lane];
        da[2] += t[PT_KFF + 2] * (mass * 9.81) + Pb.kff[2] * (dmass * 9.81);
#pragma unroll
        for (int c = 0; c < 3; c++) db[c] = dmass * cold[18 + c][lane] + mass * da[c];
#pragma unroll
        for (int c = 0; c < 3; c++) dal[c] = t[PT_KP_W + c] * cold[27 + c][lane] + t[PT_KD_W + c] * cold[30 + c][lane];
        dal[0] += t[PT_KFF + 3] * cold[33][lane];
        dal[1] += t[PT_KFF + 4] * cold[34][lane];
        dal[1] += t[PT_KFF + 5] * cold[35][lane];
        // Iw dal = R (Ib (R^T dal));  dIw al = R (dIb (R^T al)),  dIw w_d = R (dIb (R^T w_d))
        double q1[3], q2[3], m1[3], h1[3], h2[3], cw[3];
        mat_t_vec(R, dal, q1);
        const double t1[3] = {cold[36][lane], cold[37][lane], cold[38][lane]}, t2[3] = {cold[39][lane], cold[40][lane], cold[41][lane]};
        const double wd[3] = {cold[33][lane], cold[34][lane], cold[35][lane]};
#pragma unroll
        for (int r = 0; r < 3; r++) {
          q2[r] = (Pb.Ib[3 * r] * q1[0] + Pb.Ib[3 * r + 1] * q1[1] + Pb.Ib[3 * r + 2] * q1[2]) +
                  (t[PT_IB + 3 * r] * t1[0] + t[PT_IB + 3 * r + 1] * t1[1] + t[PT_IB + 3 * r + 2] * t1[2]);
          m1[r] = t[PT_IB + 3 * r] * t2[0] + t[PT_IB + 3 * r + 1] * t2[1] + t[PT_IB + 3 * r + 2] * t2[2];
        }
        mat_vec(R, q2, h1);  // Iw dal + dIw al
        mat_vec(R, m1, h2);  // dIw w_d
        cross3(wd, h2, cw);
#pragma unroll
        for (int c = 0; c < 3; c++) db[3 + c] = h1[c] + cw[c];
      }

      // df0, A df0, s = S (A df0 - db) + dS u
      double df0[4][3], du[6], s[6];
      {
        CParams& Pc = *QC_PARAMS_HERE(Pg);
        CDouble* const t = QC_ROW_HERE(th);
        const double mu = Pc.mu, dmu = t[PT_MU], dfzmin = t[PT_FZMIN], dfzmax = t[PT_FZMAX];
#pragma unroll
        for (int c = 0; c < 6; c++) du[c] = -db[c];
#pragma unroll
        for (int l = 0; l < 4; l++) {
          const double dlim = (cd & (1u << (16 + 2 * l))) ? dfzmin : ((cd & (2u << (16 + 2 * l))) ? dfzmax : 0.0);
          const double tie = dmu * f[l][2] + mu * dlim;
          double m[3];
          df0[l][0] = sign(2 * l) * tie;
          df0[l][1] = sign(8 + 2 * l) * tie;
          df0[l][2] = dlim;
          const double rl[3] = {cold[3 * l][lane], cold[3 * l + 1][lane], cold[3 * l + 2][lane]};
          cross3(rl, df0[l], m);
#pragma unroll
          for (int c = 0; c < 3; c++) {
            du[c] += df0[l][c];
            du[3 + c] += m[c];
          }
        }
      }
      {
        CParams& Ps = *QC_PARAMS_HERE(Pg);
        CDouble* const t = QC_ROW_HERE(th);
#pragma unroll
        for (int r = 0; r < 6; r++) {
          double sa = 0.0, sb = 0.0;
#pragma unroll
          for (int c = 0; c < 6; c++) {
            sa += Ps.S[6 * r + c] * du[c];
            sb += t[PT_S + 6 * r + c] * cold[12 + c][lane];
          }
          s[r] = sa + sb;
        }
      }
      // rhs = e o Z^T dg + dZ^T g, substituted against the factor
      double y[12];
      const uint32_t fc = face;
      const auto on = [fc](int j) { return (fc & (1u << j)) != 0; };
      const double sl[3] = {s[0], s[1], s[2]}, sg[3] = {s[3], s[4], s[5]};
      double mu, dmu;
      {
        CParams& Pc = *QC_PARAMS_HERE(Pg);
        CDouble* const t = QC_ROW_HERE(th);
        mu = Pc.mu;
        dmu = t[PT_MU];
      }
      const auto slope = [fc, mu](int at) { return (fc & (1u << at)) ? -mu : ((fc & (2u << at)) ? mu : 0.0); };
#pragma unroll
      for (int l = 0; l < 4; l++) {
        double cr[3], dg[3];
        const double rl[3] = {cold[3 * l][lane], cold[3 * l + 1][lane], cold[3 * l + 2][lane]};
        cross3(sg, rl, cr);
#pragma unroll
        for (int c = 0; c < 3; c++) {
          CParams& Pw = *QC_PARAMS_HERE(Pg);  // one row of W and of dW at a time: the scalar loads stay next to their use
          CDouble* const t = QC_ROW_HERE(th);
          double wx = 0.0, dwf = 0.0;
#pragma unroll
          for (int m = 0; m < 12; m++) {
            wx += Pw.W[12 * (3 * l + c) + m] * df0[m / 3][m % 3];
            dwf += t[PT_W + 12 * (3 * l + c) + m] * f[m / 3][m % 3];
          }
          dg[c] = 2.0 * ((sl[c] + cr[c]) + (wx + dwf));
        }
        y[3 * l] = on(3 * l) ? dg[0] : 0.0;
        y[3 * l + 1] = on(3 * l + 1) ? dg[1] : 0.0;
        y[3 * l + 2] = on(3 * l + 2) ? (dg[2] + slope(12 + 2 * l) * dg[0] + slope(20 + 2 * l) * dg[1]) + dmu * cold[42 + l][lane] : 0.0;
      }
      ldlt_apply<12>(M, y);

      if (live) {
        double* const grf_tan = a.grf_tan;
        double* const b_tan = a.b_tan;
        if (grf_tan) {
#pragma unroll
          for (int l = 0; l < 4; l++) {
            // -df_l = (Z y)_l - df0_l
            const double yz = on(3 * l + 2) ? y[3 * l + 2] : 0.0;
            double wv[3], gt[3];
            wv[0] = (((on(3 * l) ? y[3 * l] : 0.0) + slope(12 + 2 * l) * yz) - df0[l][0]) + poison;
            wv[1] = (((on(3 * l + 1) ? y[3 * l + 1] : 0.0) + slope(20 + 2 * l) * yz) - df0[l][1]) + poison;
            wv[2] = (yz - df0[l][2]) + poison;
            mat_t_vec(R, wv, gt);
            if (a.grf_tan_in) {  // read before the row is written: grf_tan_in may BE grf_tan
              double gi[3];
              load3(a.grf_tan_in, 4 * row + l, gi);
#pragma unroll
              for (int c = 0; c < 3; c++) gt[c] = gi[c] + gt[c];
            }
            store3(grf_tan, 4 * row + l, gt);
          }
        }
        if (b_tan) {
          double lo[3] = {db[0] + poison, db[1] + poison, db[2] + poison}, hi[3] = {db[3] + poison, db[4] + poison, db[5] + poison};
          if (a.b_tan_in) {
            double bl[3], bh[3];
            load3(a.b_tan_in, 2 * row, bl);
            load3(a.b_tan_in, 2 * row + 1, bh);
#pragma unroll
            for (int c = 0; c < 3; c++) {
              lo[c] = bl[c] + lo[c];
              hi[c] = bh[c] + hi[c];
            }
          }
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
