// qc_plant_adjoint.hpp - the reverse pass of the plant step (qc_plant.hpp): qc_plant_step_adjoint_batch (include/qc_balance.h), the
// kernel between control_batch_autograd() and backpropagation through a closed-loop rollout.
//
// Given the state BEFORE a step, the forces and the feet the step read, and cotangents on what the step wrote (Rwb', x', xdot', w',
// feet'), it writes the cotangents of Rwb, x, xdot, w, grf_body and foot_world: the transpose-Jacobian of the step exactly as
// plant_step_kernel evaluates it.  Matrix cotangents are ENTRYWISE (Rb[3 a + b] = dL / dR_ab, the nine entries independent - Rwb need
// not stay a rotation), qc_sensitivity_rot_io.Rwb_bar's convention.  Nothing is saved by the forward launch: the kernel recomputes
// the forward step (restated here; rigid_body_step keeps its intermediates to itself and stays as it is).
//
// The reverse pass, in the notation of qc_plant.hpp (a cotangent of v is vb):
//   feet     feet'_l = Rn^T d_l, d_l = foot_world_l - x':   Rnb += d_l feetb_l^T,  db_l = Rn feetb_l,  foot_worldb_l += db_l,  x'b -= db_l
//   product  Rn = E R:                                       Eb = Rnb R^T,  Rb += E^T Rnb
//   Exp      E = I + A K + B K^2, K = hat(phi), K^2 = phi phi^T - theta^2 I; with M = Eb, ax = axial(M), Ms = M + M^T:
//              phib = A ax + B (Ms phi - 2 tr(M) phi) + (Ab A1 + Bb B1) phi,   Ab = <M, K> = phi . ax,   Bb = <M, K^2> = phi^T M phi - theta^2 tr M
//              (the same vector as vee(Kb - Kb^T), Kb = A M + B (M K^T + K^T M), without the 3x3 products)
//              A1 = A'(theta) / theta = (cos theta - A) / theta^2,   B1 = B'(theta) / theta = (A - 2 B) / theta^2      (below)
//   Euler    phi = dt w', w' = w + dt wdot, x' = x + dt xdot', xdot' = xdot + dt (fs / m - g e3)
//   wdot     wdot = R Ib^-1 R^T (tau - w x (R Ib R^T w)): into Rb (four outer products), wb and taub
//   forces   tau = sum r_l x f_l, r_l = foot_world_l - x, f_l = -R grf_body_l:
//              fb_l = fsb + taub x r_l,  rb_l = f_l x taub,  grfb_l = -R^T fb_l,  Rb -= fb_l grf_body_l^T
//
// A1 and B1 are differences that cancel for a small angle: (cos theta - A) and (A - 2 B) are both O(theta^2).  Below theta^2 = 1
// they are the series  A1 = sum_k (-1)^k theta^(2k-2) 2k / (2k+1)!,  B1 = sum_k (-1)^k theta^(2k-2) 2k / (2k+2)!  (k = 1 ... 9;
// the first term left out is 20 / 21! = 4e-19 and 20 / 22! = 2e-20 of a sum of 1/3 and 1/12), whose values at theta = 0 are the limits -1/3
// and -1/12: at an angle of exactly 0 the smooth limit is differentiated, not the forward step's select.  From theta^2 = 1 on they are the
// quotients themselves from the forward step's own sincos_joint(theta / 2), cos theta = 1 - 2 sin^2(theta / 2): the differences are
// then at least 0.30 of a minuend of at most 1 (A1) and 0.078 of 0.92 (B1), so at most 4 and 12 times their roundings.  (An angle
// of 1 rad PER STEP is far outside what a controller runs at; the tests sweep it.)
//
// Non-finite inputs propagate as NaN (a NaN theta^2 takes the quotients); nothing is clamped.
//
// Kernel: qc_plant.hpp's shape - one lane per robot, FP64, blocks of PLANT_BLOCK, tail lanes return, no LDS, no scratch, the
// per-argument arrays read directly.  A NULL input cotangent is zero; a NULL output is not stored.  A lane reads ALL of its inputs
// before it writes anything and touches only its own rows, so an output may be the same array as an input cotangent of the same
// layout (x_bar over x_next_bar, Rwb_bar over Rwb_next_bar, foot_world_bar or grf_bar over feet_next_bar, ...): backpropagation
// through time runs in place.  576 B in and 336 B out per robot with every array given.
#pragma once
#include "qc_plant.hpp"

namespace qc {

struct PlantAdjointArgs : BodyConst {
  const double *Rwb, *x, *xdot, *w;                                                       // [n][9], [n][3] x 3: the state BEFORE the step
  const double *grf_body, *foot_world;                                                    // [n][4][3]
  const double *Rwb_next_bar, *x_next_bar, *xdot_next_bar, *w_next_bar, *feet_next_bar;   // optional IN (nullptr: zero)
  double *Rwb_bar, *x_bar, *xdot_bar, *w_bar, *grf_bar, *foot_world_bar;                  // optional OUT
};

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

// theta^2 below which the coefficients that cancel for a small angle are series (A1, B1 here; B, C of qc_plant_tangent.hpp)
constexpr double SERIES_BELOW = 1.0;

QC_DEV void load3_or_zero(const double* p, long idx, double (&v)[3]) {
  if (p) load3(p, idx, v);
  else v[0] = v[1] = v[2] = 0.0;
}

// A1 = (cos theta - A) / theta^2 and B1 = (A - 2 B) / theta^2 from th2 = theta^2, sh = sin(theta / 2) and the forward step's A and B
QC_DEV void exp_coefficient_slopes(double th2, double sh, double A, double B, double* __restrict__ A1, double* __restrict__ B1) {
  if (th2 < SERIES_BELOW) {
    const double z = th2;
    // 2k / (2k+1)! and 2k / (2k+2)!, k = 9 ... 1, alternating
    double p = -1.4797143443923793e-16, q = -7.398571721961897e-18;  // -18 / 19!, -18 / 20!
    p = __builtin_fma(p, z, 4.498331606952833e-14);    q = __builtin_fma(q, z, 2.499073114973796e-15);    //  16 / 17!,  16 / 18!
    p = __builtin_fma(p, z, -1.0706029224547743e-11);  q = __builtin_fma(q, z, -6.691268265342339e-13);   // -14 / 15!, -14 / 16!
    p = __builtin_fma(p, z, 1.9270852604185937e-09);   q = __builtin_fma(q, z, 1.376489471727567e-10);    //  12 / 13!,  12 / 14!
    p = __builtin_fma(p, z, -2.505210838544172e-07);   q = __builtin_fma(q, z, -2.08767569878681e-08);    // -10 / 11!, -10 / 12!
    p = __builtin_fma(p, z, 2.2045855379188714e-05);   q = __builtin_fma(q, z, 2.204585537918871e-06);    //   8 / 9!,    8 / 10!
    p = __builtin_fma(p, z, -0.0011904761904761906);   q = __builtin_fma(q, z, -0.00014880952380952382);  //  -6 / 7!,   -6 / 8!
    p = __builtin_fma(p, z, 0.03333333333333333);      q = __builtin_fma(q, z, 0.005555555555555556);     //   4 / 5!,    4 / 6!
    *A1 = __builtin_fma(p, z, -0.3333333333333333);   // -2 / 3!
    *B1 = __builtin_fma(q, z, -0.08333333333333333);  // -2 / 4!
  } else {  // (NaN comes here and stays NaN)
    const double cth = 1.0 - 2.0 * (sh * sh);
    *A1 = (cth - A) / th2;
    *B1 = (A - 2.0 * B) / th2;
  }
}

// o = (I + A K + B K^2) u, K = hat(phi): Exp(phi) u with the step's A and B, its transpose with -A
QC_DEV void exp_apply(const double (&phi)[3], double A, double B, const double (&u)[3], double (&o)[3]) {
  double k1[3], k2[3];
  cross3(phi, u, k1);
  cross3(phi, k1, k2);
#pragma unroll
  for (int k = 0; k < 3; k++) o[k] = u[k] + (A * k1[k] + B * k2[k]);
}

// Rb[3 r + c] += u[r] v[c]
QC_DEV void add_outer(double (&Rb)[9], const double (&u)[3], const double (&v)[3]) {
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) Rb[3 * r + c] += u[r] * v[c];
}

__global__ __launch_bounds__(PLANT_BLOCK) void plant_step_adjoint_kernel(const long n, const PlantAdjointArgs a) {
  const long i = (long)blockIdx.x * PLANT_BLOCK + threadIdx.x;
  if (i >= n) return;  // tail lanes
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
  double Rnb[9], x1b[3], v1b[3], w1b[3], ftb[4][3];
  if (a.Rwb_next_bar) load9(a.Rwb_next_bar, i, Rnb);
  else {
#pragma unroll
    for (int k = 0; k < 9; k++) Rnb[k] = 0.0;
  }
  load3_or_zero(a.x_next_bar, i, x1b);
  load3_or_zero(a.xdot_next_bar, i, v1b);
  load3_or_zero(a.w_next_bar, i, w1b);
#pragma unroll
  for (int l = 0; l < 4; l++) load3_or_zero(a.feet_next_bar, 4 * i + l, ftb[l]);

  // ---- the forward step, as plant_step_kernel and rigid_body_step evaluate it
  double fs[3] = {0.0, 0.0, 0.0}, tau[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int l = 0; l < 4; l++) {
    double rg[3], f[3], r[3], m[3];
    mat_vec(R, gb[l], rg);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      f[k] = -rg[k];
      r[k] = pw[l][k] - x[k];
    }
    cross3(r, f, m);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      fs[k] += f[k];
      tau[k] += m[k];
    }
  }
  double wb[3], Iwb[3], Iw_w[3], gyro[3], nb[3], Inb[3], wdot[3];
  mat_t_vec(R, w, wb);
  mat_vec(a.Ib, wb, Iwb);
  mat_vec(R, Iwb, Iw_w);
  cross3(w, Iw_w, gyro);
#pragma unroll
  for (int k = 0; k < 3; k++) tau[k] -= gyro[k];
  mat_t_vec(R, tau, nb);
  mat_vec(a.Ib_inv, nb, Inb);
  mat_vec(R, Inb, wdot);
  double x1[3], phi[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double acc = fs[k] / a.mass - (k == 2 ? a.g : 0.0);
    const double v1 = v[k] + a.dt * acc;
    x1[k] = x[k] + a.dt * v1;
    phi[k] = a.dt * (w[k] + a.dt * wdot[k]);
  }
  const double xx = phi[0] * phi[0], yy = phi[1] * phi[1], zz = phi[2] * phi[2];
  const double th2 = xx + yy + zz;
  const double h = 0.5 * sqrt(th2);
  double sh, ch;
  sincos_joint(h, &sh, &ch);
  const double sc = h > 0.0 ? sh / h : 1.0;
  const double A = sc * ch, B = 0.5 * (sc * sc);
  // (neither E nor Rn = E R is formed: the reverse pass applies E = I + A K + B K^2 and its transpose as cross products, exp_apply)

  // ---- the reverse pass
  double pwb[4][3];
  // feet'_l = Rn^T (foot_world_l - x')
#pragma unroll
  for (int l = 0; l < 4; l++) {
    const double d[3] = {pw[l][0] - x1[0], pw[l][1] - x1[1], pw[l][2] - x1[2]};
    double Rf[3];
    add_outer(Rnb, d, ftb[l]);
    mat_vec(R, ftb[l], Rf);
    exp_apply(phi, A, B, Rf, pwb[l]);  // Rn feetb_l
#pragma unroll
    for (int k = 0; k < 3; k++) x1b[k] -= pwb[l][k];
  }
  // Rn = E R
  double M[9], Rb[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      M[3 * r + c] = Rnb[3 * r] * R[3 * c] + Rnb[3 * r + 1] * R[3 * c + 1] + Rnb[3 * r + 2] * R[3 * c + 2];  // Rnb R^T
    }
#pragma unroll
  for (int c = 0; c < 3; c++) {  // E^T Rnb, column by column (E^T = Exp(-phi))
    const double col[3] = {Rnb[c], Rnb[3 + c], Rnb[6 + c]};
    double o[3];
    exp_apply(phi, -A, B, col, o);
    Rb[c] = o[0]; Rb[3 + c] = o[1]; Rb[6 + c] = o[2];
  }
  // E = Exp(phi)
  double A1, B1, phib[3];
  exp_coefficient_slopes(th2, sh, A, B, &A1, &B1);
  {
    const double ax[3] = {M[7] - M[5], M[2] - M[6], M[3] - M[1]};
    const double tr = M[0] + M[4] + M[8];
    double ms[3];
#pragma unroll
    for (int r = 0; r < 3; r++) ms[r] = (M[3 * r] + M[r]) * phi[0] + (M[3 * r + 1] + M[3 + r]) * phi[1] + (M[3 * r + 2] + M[6 + r]) * phi[2];
    const double Ab = phi[0] * ax[0] + phi[1] * ax[1] + phi[2] * ax[2];
    const double Bb = 0.5 * (phi[0] * ms[0] + phi[1] * ms[1] + phi[2] * ms[2]) - th2 * tr;
    const double radial = Ab * A1 + Bb * B1;
#pragma unroll
    for (int k = 0; k < 3; k++) phib[k] = A * ax[k] + B * (ms[k] - 2.0 * tr * phi[k]) + radial * phi[k];
  }
  // semi-implicit Euler
  double wbar[3], wdotb[3], fsb[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    w1b[k] += a.dt * phib[k];
    wbar[k] = w1b[k];
    wdotb[k] = a.dt * w1b[k];
    v1b[k] += a.dt * x1b[k];
    fsb[k] = a.dt * v1b[k] / a.mass;
  }
  // wdot = R Ib^-1 R^T tau,  tau = (sum r x f) - w x (R Ib R^T w)
  double Inbb[3], nbb[3], taub[3], Iwwb[3], Iwbb[3], wbb[3], t[3];
  add_outer(Rb, wdotb, Inb);
  mat_t_vec(R, wdotb, Inbb);
  mat_t_vec(a.Ib_inv, Inbb, nbb);
  add_outer(Rb, tau, nbb);
  mat_vec(R, nbb, taub);
  cross3(taub, Iw_w, t);  // Iw_w x gyrob, gyrob = -taub
  cross3(w, taub, Iwwb);  // gyrob x w
  add_outer(Rb, Iwwb, Iwb);
  mat_t_vec(R, Iwwb, Iwbb);
  mat_t_vec(a.Ib, Iwbb, wbb);
  add_outer(Rb, w, wbb);
  {
    double Rwbb[3];
    mat_vec(R, wbb, Rwbb);
#pragma unroll
    for (int k = 0; k < 3; k++) wbar[k] += t[k] + Rwbb[k];
  }
  // moments and forces
  double xbar[3] = {x1b[0], x1b[1], x1b[2]}, gbb[4][3];
#pragma unroll
  for (int l = 0; l < 4; l++) {
    double rg[3], f[3], r[3], rb[3], fb[3], g[3];
    mat_vec(R, gb[l], rg);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      f[k] = -rg[k];
      r[k] = pw[l][k] - x[k];
    }
    cross3(f, taub, rb);
    cross3(taub, r, fb);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      fb[k] += fsb[k];
      pwb[l][k] += rb[k];
      xbar[k] -= rb[k];
    }
    mat_t_vec(R, fb, g);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      gbb[l][k] = -g[k];
      fb[k] = -fb[k];
    }
    add_outer(Rb, fb, gb[l]);
  }
  // every input of this robot has been read: an output may overwrite an input cotangent
  if (a.Rwb_bar) {
    double* q = a.Rwb_bar + 9 * i;
#pragma unroll
    for (int k = 0; k < 9; k++) q[k] = Rb[k];
  }
  if (a.x_bar) store3(a.x_bar, i, xbar);
  if (a.xdot_bar) store3(a.xdot_bar, i, v1b);
  if (a.w_bar) store3(a.w_bar, i, wbar);
  if (a.grf_bar) {
#pragma unroll
    for (int l = 0; l < 4; l++) store3(a.grf_bar, 4 * i + l, gbb[l]);
  }
  if (a.foot_world_bar) {
#pragma unroll
    for (int l = 0; l < 4; l++) store3(a.foot_world_bar, 4 * i + l, pwb[l]);
  }
}

}  // namespace qc
#endif  // __HIPCC__
