// qc_plant.hpp - the plant the controller itself assumes, stepped on the device: ONE rigid body with world-frame forces at the
// feet, the model of BalanceController::dynamics() (balance_controller.cpp:237-272).  qc_plant_step_batch (include/qc_balance.h)
// alternates with qc_control_batch on one stream, so a batch of robots advances without a host round trip.
//
// Per robot, with the conventions of control() and dynamics() (Rwb world<-base row-major; x, xdot, w in the WORLD frame, w as in
// Iw wdot_d + w_d x Iw w_d; grf_body as qc_control_batch wrote it: negated, body frame, 0 for swing legs and failed robots):
//   f_i   = -Rwb grf_body_i                 force ON the body from leg i, world frame
//   r_i   = foot_world_i - x
//   a     = (sum f_i) / m - (0, 0, g)
//   Iw    = Rwb Ib Rwb^T,   Iw^-1 = Rwb Ib^-1 Rwb^T
//   wdot  = Iw^-1 (sum r_i x f_i - w x (Iw w))
// and one semi-implicit Euler step
//   xdot' = xdot + dt a,   x' = x + dt xdot',   w' = w + dt wdot,   Rwb' = Exp(dt w') Rwb,
// Exp being Rodrigues' formula I + A K + B K^2 (K = hat(phi), theta = |phi|) with A = sin(theta) / theta and
// B = (sin(theta/2) / (theta/2))^2 / 2: no 1 - cos(theta), so nothing cancels for a small angle, and both take their limits
// (1 and 1/2) at theta = 0.  With h = theta / 2 one sincos_joint(h) gives both: A = (sin h / h) cos h.
// Optional output: feet'_i = Rwb'^T (foot_world_i - x'), the `feet` array the next qc_control_batch reads.
//
// What it is NOT: there is no contact model.  Forces are applied as given, a stance foot is wherever foot_world says it is, and
// a failed QP (zero forces) is free fall for that step.  The body has no legs: joints and the leg-level tick (joint_q,
// qc_tick_batch) are outside this model.
//
// Kernel: one lane per robot, FP64, no LDS, no scratch.  A lane reads ALL of its inputs before it writes anything and touches
// only its own rows, so the state arrays are updated in place and an output may be the same array as an input of the same
// layout.  Like the solver kernels it reads the per-argument arrays directly (load3 / load9): a wave's loads of one array cover
// one contiguous span (64 x 24, 72 or 96 B) and consume every fetched line; 336 B in and 240 B out per robot.
//
// The body's step from the net force and moment on is ONE function, rigid_body_step, which this kernel and leg_plant_step_kernel
// (qc_leg_plant.hpp) both call.  The rule for touching it: a change must leave both kernels' RESULTS (bit for bit, against the parent
// build, on the tests' pools) and RESOURCES (registers, scratch, occupancy, instruction counts: profiles/*_kernel_resources.txt) as
// they are - not their assembly text.  Register numbers, instruction order and the operand order of a commutative IEEE multiply or
// add may move: commuting the operands changes no finite result, no infinity and no NaN-ness.
#pragma once
#include "qc_device.hpp"

namespace qc {

// The constants of the body: the base of both plant kernels' argument structs (by value in the kernarg segment; not part of
// DevParams), so they lead both layouts and read a.mass ... a.dt in either.
struct BodyConst {
  double mass, Ib[9], Ib_inv[9], g, dt;
};

struct PlantArgs : BodyConst {
  double *Rwb, *x, *xdot, *w;  // [n][9], [n][3] x 3, IN/OUT
  const double *grf_body, *foot_world;  // [n][4][3]
  double* feet;  // [n][4][3] OUT or nullptr
};

constexpr double PLANT_G = 9.81;  // the constant of the kernels (plan_foothold) and of the checker
constexpr int PLANT_BLOCK = 256;

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

// The body's step from the net force fs and the net moment tau about the centre of mass (world frame): gyroscopic term, Ib^-1,
// semi-implicit Euler, Rodrigues without 1 - cos.  x, v, w are updated, tau is consumed, Rn = Rwb'.
QC_DEV void rigid_body_step(const BodyConst& b, const double (&R)[9], double (&x)[3], double (&v)[3], double (&w)[3], const double (&fs)[3],
                            double (&tau)[3], double (&Rn)[9]) {
  // wdot = R Ib^-1 R^T (tau - w x (R Ib R^T w))
  double wb[3], Iwb[3], Iw_w[3], gyro[3], nb[3], Inb[3], wdot[3];
  mat_t_vec(R, w, wb);
  mat_vec(b.Ib, wb, Iwb);
  mat_vec(R, Iwb, Iw_w);
  cross3(w, Iw_w, gyro);
#pragma unroll
  for (int k = 0; k < 3; k++) tau[k] -= gyro[k];
  mat_t_vec(R, tau, nb);
  mat_vec(b.Ib_inv, nb, Inb);
  mat_vec(R, Inb, wdot);
  // semi-implicit Euler
  double phi[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double acc = fs[k] / b.mass - (k == 2 ? b.g : 0.0);
    v[k] += b.dt * acc;
    x[k] += b.dt * v[k];
    w[k] += b.dt * wdot[k];
    phi[k] = b.dt * w[k];
  }
  // Rwb' = Exp(phi) Rwb
  const double xx = phi[0] * phi[0], yy = phi[1] * phi[1], zz = phi[2] * phi[2];
  const double h = 0.5 * sqrt(xx + yy + zz);
  double sh, ch;
  sincos_joint(h, &sh, &ch);
  const double sc = h > 0.0 ? sh / h : 1.0;  // sin(h) / h, 1 at h = 0 (NaN stays NaN through ch)
  const double A = sc * ch, B = 0.5 * (sc * sc);
  const double E[9] = {1.0 - B * (yy + zz),                 B * (phi[0] * phi[1]) - A * phi[2], B * (phi[0] * phi[2]) + A * phi[1],
                       B * (phi[0] * phi[1]) + A * phi[2], 1.0 - B * (xx + zz),                 B * (phi[1] * phi[2]) - A * phi[0],
                       B * (phi[0] * phi[2]) - A * phi[1], B * (phi[1] * phi[2]) + A * phi[0], 1.0 - B * (xx + yy)};
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) Rn[3 * r + c] = E[3 * r] * R[c] + E[3 * r + 1] * R[3 + c] + E[3 * r + 2] * R[6 + c];
}

__global__ __launch_bounds__(PLANT_BLOCK) void plant_step_kernel(const long n, const PlantArgs a) {
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
  // net force and moment about the centre of mass, world frame
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
  double Rn[9];
  rigid_body_step(a, R, x, v, w, fs, tau, Rn);
  // every input of this robot has been read: the outputs may overwrite them
  {
    double* q = a.Rwb + 9 * i;
#pragma unroll
    for (int k = 0; k < 9; k++) q[k] = Rn[k];
  }
  store3(a.x, i, x);
  store3(a.xdot, i, v);
  store3(a.w, i, w);
  if (a.feet) {
#pragma unroll
    for (int l = 0; l < 4; l++) {
      const double d[3] = {pw[l][0] - x[0], pw[l][1] - x[1], pw[l][2] - x[2]};
      double fb[3];
      mat_t_vec(Rn, d, fb);
      store3(a.feet, 4 * i + l, fb);
    }
  }
}

}  // namespace qc
#endif  // __HIPCC__
