// qc_plant_tangent.hpp - forward mode of the plant step (qc_plant.hpp): qc_plant_step_tangent_batch (include/qc_tangent.h), the
// kernel that follows qc_tangent_batch in a forward-mode closed loop.  Given the state BEFORE a step, the forces and the feet the
// step read, and K tangents on them, it writes the K tangents of what the step wrote (Rwb', x', xdot', w', feet').  Rotations move
// along world-frame left tangents (Rwb <- exp([delta]x) Rwb), qc_tangent_batch's convention, so the two kernels chain in place.
// Nothing is saved by the forward launch: the step is recomputed (restated here as in qc_plant_adjoint.hpp; rigid_body_step keeps
// its intermediates to itself and stays as it is).
//
// Per direction, in the notation of qc_plant.hpp (h = Iw w, c = tau - w x h, Iw u = R Ib R^T u):
//   df_l  = delta x f_l - R dg_l,   dr_l = dp_l - dx,   da = (sum df_l) / m,   dtau = sum (dr_l x f_l + r_l x df_l)
//   dh    = delta x h + Iw (dw - delta x w)                  (dIw = [delta]x Iw - Iw [delta]x)
//   dc    = dtau - dw x h - w x dh
//   dwdot = Iw^-1 (dc - delta x c) + delta x wdot
//   dxdot' = dxdot + dt da,   dx' = dx + dt dxdot',   dw' = dw + dt dwdot
//   delta' = Jl(phi) dt dw' + Exp(phi) delta,   phi = dt w',   Jl = I + B K + C K^2,   B = (1 - cos theta) / theta^2,
//            C = (theta - sin theta) / theta^3                 (Rn = Exp(phi) R: the left Jacobian of the exponential)
//   dfeet'_l = Rn^T (dp_l - dx' - delta' x d_l),   d_l = foot_world_l - x'
// Exp(phi) u and Rn^T u = R^T Exp(-phi) u are applied as cross products with the forward step's A and B (exp_apply), Jl with B and C.
//
// B and C: below theta^2 = 1 (qc_plant_adjoint.hpp's threshold) the series  B = sum_k (-1)^k theta^(2k) / (2k+2)!,
// C = sum_k (-1)^k theta^(2k) / (2k+3)!  (k = 0 ... 9; the first term left out is 1 / 22! = 9e-22 and 1 / 23! = 4e-23 of sums of at
// least 0.45 and 0.15), whose values at theta = 0 are the limits 1/2 and 1/6: at an angle of exactly 0 the smooth limit is
// differentiated, Jl = I.  From theta^2 = 1 on the quotients from the forward step's own sincos_joint(theta / 2): B is the step's
// 2 sin^2(theta / 2) / theta^2 (no cancellation), C = (1 - A) / theta^2, a difference of at least 0.158 of a minuend of 1.
// Non-finite inputs propagate as NaN (a NaN theta^2 takes the quotients); nothing is clamped.
//
// Kernel: one lane per (direction, robot), the robot index fastest - pair j = k n + i - so a wave's loads of one direction's rows
// are contiguous as the plant's are, and K multiplies the parallelism a small batch lacks.  The base state is re-read per direction
// (from L2) and the direction-independent part (two 3x3 applications, one sincos) recomputed: there is no factorisation to share.
// FP64, workgroups of one wave, a grid stride once the grid is capped (PLANT_TANGENT_MAX_BLOCKS), no LDS, no atomics, no scratch.
// A NULL tangent is zero; a NULL output is not stored.  A pair reads ALL of its inputs before it writes anything and touches only
// its own rows, so an output may be the input tangent of its layout (x_next_tan over x_tan, Rwb_rot_next_tan over Rwb_rot_tan,
// feet_next_tan over grf_tan or foot_world_tan): a rollout carries one set of tangent buffers.  336 B of base state and up to
// 288 B of tangents in, up to 144 B out per pair.
#pragma once
#include "qc_plant_adjoint.hpp"  // load3_or_zero, exp_apply

namespace qc {

struct PlantTangentArgs : BodyConst {
  const double *Rwb, *x, *xdot, *w;       // [n][9], [n][3] x 3: the state BEFORE the step
  const double *grf_body, *foot_world;    // [n][4][3]
  long n_dir;                             // K
  const double *Rwb_rot_tan, *x_tan, *xdot_tan, *w_tan;  // [K][n][3], nullptr: zero
  const double *grf_tan, *foot_world_tan;                // [K][n][4][3], nullptr: zero
  double *Rwb_rot_next_tan, *x_next_tan, *xdot_next_tan, *w_next_tan, *feet_next_tan;  // optional OUT
};

constexpr int PLANT_TANGENT_BLOCK = 64;  // one wave
constexpr int PLANT_TANGENT_MAX_BLOCKS = 4096;

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

// Bj = (1 - cos theta) / theta^2 and Cj = (theta - sin theta) / theta^3 from th2 = theta^2 and the forward step's A and B
QC_DEV void left_jacobian_coefficients(double th2, double A, double B, double* __restrict__ Bj, double* __restrict__ Cj) {
  if (th2 < SERIES_BELOW) {  // qc_plant_adjoint.hpp's threshold
    const double z = th2;
    // 1 / (2k+2)! and 1 / (2k+3)!, k = 9 ... 0, alternating
    double p = -4.110317623312165e-19, q = -1.9572941063391263e-20;  // -1 / 20!, -1 / 21!
    p = __builtin_fma(p, z, 1.5619206968586225e-16);   q = __builtin_fma(q, z, 8.22063524662433e-18);     //  1 / 18!,  1 / 19!
    p = __builtin_fma(p, z, -4.779477332387385e-14);   q = __builtin_fma(q, z, -2.8114572543455206e-15);  // -1 / 16!, -1 / 17!
    p = __builtin_fma(p, z, 1.1470745597729725e-11);   q = __builtin_fma(q, z, 7.647163731819816e-13);    //  1 / 14!,  1 / 15!
    p = __builtin_fma(p, z, -2.08767569878681e-09);    q = __builtin_fma(q, z, -1.6059043836821613e-10);  // -1 / 12!, -1 / 13!
    p = __builtin_fma(p, z, 2.755731922398589e-07);    q = __builtin_fma(q, z, 2.505210838544172e-08);    //  1 / 10!,  1 / 11!
    p = __builtin_fma(p, z, -2.48015873015873e-05);    q = __builtin_fma(q, z, -2.7557319223985893e-06);  // -1 / 8!,  -1 / 9!
    p = __builtin_fma(p, z, 0.001388888888888889);     q = __builtin_fma(q, z, 0.0001984126984126984);    //  1 / 6!,   1 / 7!
    p = __builtin_fma(p, z, -0.041666666666666664);    q = __builtin_fma(q, z, -0.008333333333333333);    // -1 / 4!,  -1 / 5!
    *Bj = __builtin_fma(p, z, 0.5);                   //  1 / 2!
    *Cj = __builtin_fma(q, z, 0.16666666666666666);   //  1 / 3!
  } else {  // (NaN comes here and stays NaN)
    *Bj = B;
    *Cj = (1.0 - A) / th2;
  }
}

// o = R Mb R^T u: the world-frame inertia (Mb = Ib) or its inverse (Mb = Ib^-1) applied, as rigid_body_step does
QC_DEV void world_apply(const double (&R)[9], const double (&Mb)[9], const double (&u)[3], double (&o)[3]) {
  double ub[3], mb[3];
  mat_t_vec(R, u, ub);
  mat_vec(Mb, ub, mb);
  mat_vec(R, mb, o);
}

__global__ __launch_bounds__(PLANT_TANGENT_BLOCK) void plant_step_tangent_kernel(const long n, const PlantTangentArgs a) {
  const long total = n * a.n_dir;
  for (long j = (long)blockIdx.x * PLANT_TANGENT_BLOCK + threadIdx.x; j < total; j += (long)gridDim.x * PLANT_TANGENT_BLOCK) {
    const long i = j % n;  // pair j = k n + i: the row of direction k and robot i in a [K][n][m] array is j itself
    double R[9], x[3], v[3], w[3], gb[4][3], pw[4][3];
    load9(a.Rwb, i, R);
    load3(a.x, i, x);
    load3(a.xdot, i, v);
    load3(a.w, i, w);
#pragma unroll
    for (int l = 0; l < 4; l++) {
      load3(a.grf_body, 4 * i + l, gb[l]);
      load3(a.foot_world, 4 * i + l, pw[l]);
    }
    double dl[3], dx[3], dv[3], dw[3], dg[4][3], dp[4][3];
    load3_or_zero(a.Rwb_rot_tan, j, dl);
    load3_or_zero(a.x_tan, j, dx);
    load3_or_zero(a.xdot_tan, j, dv);
    load3_or_zero(a.w_tan, j, dw);
#pragma unroll
    for (int l = 0; l < 4; l++) {
      load3_or_zero(a.grf_tan, 4 * j + l, dg[l]);
      load3_or_zero(a.foot_world_tan, 4 * j + l, dp[l]);
    }

    // ---- forces and moments, the step's and the tangent's
    double fs[3] = {0.0, 0.0, 0.0}, tau[3] = {0.0, 0.0, 0.0}, dfs[3] = {0.0, 0.0, 0.0}, dtau[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int l = 0; l < 4; l++) {
      double rg[3], rdg[3], f[3], r[3], df[3], dr[3], m[3], cf[3], m1[3], m2[3];
      mat_vec(R, gb[l], rg);
      mat_vec(R, dg[l], rdg);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        f[k] = -rg[k];
        r[k] = pw[l][k] - x[k];
        dr[k] = dp[l][k] - dx[k];
      }
      cross3(dl, f, cf);
#pragma unroll
      for (int k = 0; k < 3; k++) df[k] = cf[k] - rdg[k];
      cross3(r, f, m);
      cross3(dr, f, m1);
      cross3(r, df, m2);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        fs[k] += f[k];
        tau[k] += m[k];
        dfs[k] += df[k];
        dtau[k] += m1[k] + m2[k];
      }
    }
    // ---- wdot = Iw^-1 c, c = tau - w x h, h = Iw w
    double h[3], gyro[3], c[3], wdot[3];
    world_apply(R, a.Ib, w, h);
    cross3(w, h, gyro);
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = tau[k] - gyro[k];
    world_apply(R, a.Ib_inv, c, wdot);
    double dh[3], dc[3], dwdot[3];
    {
      double t0[3], t1[3], t2[3], t3[3], t4[3], t5[3], t6[3], t7[3];
      cross3(dl, w, t0);
#pragma unroll
      for (int k = 0; k < 3; k++) t0[k] = dw[k] - t0[k];
      world_apply(R, a.Ib, t0, t1);
      cross3(dl, h, t2);
#pragma unroll
      for (int k = 0; k < 3; k++) dh[k] = t2[k] + t1[k];
      cross3(dw, h, t3);
      cross3(w, dh, t4);
      cross3(dl, c, t5);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        dc[k] = dtau[k] - t3[k] - t4[k];
        t5[k] = dc[k] - t5[k];
      }
      world_apply(R, a.Ib_inv, t5, t6);
      cross3(dl, wdot, t7);
#pragma unroll
      for (int k = 0; k < 3; k++) dwdot[k] = t6[k] + t7[k];
    }
    // ---- semi-implicit Euler
    double x1[3], phi[3], dv1[3], dx1[3], dw1[3], dphi[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double acc = fs[k] / a.mass - (k == 2 ? a.g : 0.0);
      const double v1 = v[k] + a.dt * acc;
      x1[k] = x[k] + a.dt * v1;
      phi[k] = a.dt * (w[k] + a.dt * wdot[k]);
      dv1[k] = dv[k] + a.dt * (dfs[k] / a.mass);
      dx1[k] = dx[k] + a.dt * dv1[k];
      dw1[k] = dw[k] + a.dt * dwdot[k];
      dphi[k] = a.dt * dw1[k];
    }
    // ---- Rn = Exp(phi) R: delta' = Jl(phi) dphi + Exp(phi) delta
    const double xx = phi[0] * phi[0], yy = phi[1] * phi[1], zz = phi[2] * phi[2];
    const double th2 = xx + yy + zz;  // (separately rounded squares, as the step and its adjoint form it: the same side of the threshold)
    const double hh = 0.5 * sqrt(th2);
    double sh, ch;
    sincos_joint(hh, &sh, &ch);
    const double sc = hh > 0.0 ? sh / hh : 1.0;
    const double A = sc * ch, B = 0.5 * (sc * sc);
    double Bj, Cj, jd[3], ed[3], dl1[3];
    left_jacobian_coefficients(th2, A, B, &Bj, &Cj);
    exp_apply(phi, Bj, Cj, dphi, jd);
    exp_apply(phi, A, B, dl, ed);
#pragma unroll
    for (int k = 0; k < 3; k++) dl1[k] = jd[k] + ed[k];
    // ---- feet'_l = Rn^T d_l
    double dft[4][3];
    if (a.feet_next_tan) {
#pragma unroll
      for (int l = 0; l < 4; l++) {
        const double d[3] = {pw[l][0] - x1[0], pw[l][1] - x1[1], pw[l][2] - x1[2]};
        double cd[3], u[3], eu[3];
        cross3(dl1, d, cd);
#pragma unroll
        for (int k = 0; k < 3; k++) u[k] = dp[l][k] - dx1[k] - cd[k];
        exp_apply(phi, -A, B, u, eu);  // Exp(phi)^T u
        mat_t_vec(R, eu, dft[l]);
      }
    }
    // every input of this pair has been read: an output may overwrite an input tangent
    if (a.Rwb_rot_next_tan) store3(a.Rwb_rot_next_tan, j, dl1);
    if (a.x_next_tan) store3(a.x_next_tan, j, dx1);
    if (a.xdot_next_tan) store3(a.xdot_next_tan, j, dv1);
    if (a.w_next_tan) store3(a.w_next_tan, j, dw1);
    if (a.feet_next_tan) {
#pragma unroll
      for (int l = 0; l < 4; l++) store3(a.feet_next_tan, 4 * j + l, dft[l]);
    }
  }
}

}  // namespace qc
#endif  // __HIPCC__
