// qc_plant_model.hpp - a plant of its own (include/qc_plant_model.h): the rigid-body step, the legged step and the rigid-body step's
// reverse pass with a PER-ROBOT body - mass [n], Ib [n][9] - and an external wrench [n][6] at the centre of mass.
//
// Each kernel is its base kernel's text (plant_step_kernel, leg_plant_step_kernel, plant_step_adjoint_kernel - duplicated, not
// shared: the base kernels and their ISA stay as they are) with three differences:
//   - the lane builds its own BodyConst - the robot's mass, its Ib and the general 3x3 inverse of it (adjugate over determinant, all
//     nine entries as given), g and dt from the call - and hands it to the EXISTING rigid_body_step;
//   - fs and tau start from the wrench instead of from +0.0, the per-leg terms added in the base kernel's order behind it: a wrench
//     of +0.0 gives the base kernel's bits;
//   - a robot whose mass or Ib is refused (model_body's bits) gets NaN in every state output, and its bits in `flags`.
// The three optional inputs are TEMPLATE parameters <MASS, IB, WRENCH>: an absent one costs neither loads nor registers (the handle's
// constants stay in the kernarg segment's scalars).  The reverse pass adds three outputs, run-time optional like the base's:
//   wrench_bar = (fsb, taub),  mass_bar = -<fs, fsb> / m  (fsb = a_bar / m),  Ib_bar = Iwbb wb^T - nbb Inb^T  (nbb = Ib^-T Inbb).
//
// Kernels: one lane per robot, FP64, blocks of PLANT_BLOCK, tail lanes return, no LDS, no scratch; a lane reads ALL of its inputs
// before it writes anything and touches only its own rows.  Per robot the model adds 8 (mass), 72 (Ib) and 48 (wrench) B of loads and
// 4 B of flags to the base kernels' traffic; the reverse pass up to 48 + 8 + 72 + 4 B of stores.
#pragma once
#include "qc_leg_plant.hpp"
#include "qc_plant_adjoint.hpp"

namespace qc {

struct PlantModelArgs {
  const double *mass, *Ib, *wrench;  // [n], [n][9], [n][6]: each read only by the instantiations that carry it
  int32_t* flags;                    // [n] OUT or nullptr
};

struct PlantModelBarArgs {
  double *wrench_bar, *mass_bar, *Ib_bar;  // [n][6], [n], [n][9] OUT or nullptr
  int32_t* flags;                          // [n] OUT or nullptr
};

constexpr int PLANT_MODEL_BAD_MASS = 1, PLANT_MODEL_BAD_IB = 2;  // qc_plant_model.flags
constexpr double PLANT_MODEL_SYM_TOL = 1e-12;                    // |Ib[ab] - Ib[ba]| <= this x max|Ib|

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

// Ib^-1 = adj(Ib) / det(Ib) from all nine entries as given, and whether Ib is refused: an entry not finite, Sylvester's leading
// minors not all positive, or an asymmetry beyond PLANT_MODEL_SYM_TOL x max|Ib|.
QC_DEV bool inertia_inverse_general(const double (&I)[9], double (&inv)[9]) {
  const double c00 = I[4] * I[8] - I[5] * I[7], c01 = I[5] * I[6] - I[3] * I[8], c02 = I[3] * I[7] - I[4] * I[6];
  const double m2 = I[0] * I[4] - I[1] * I[3];
  const double det = I[0] * c00 + I[1] * c01 + I[2] * c02;
  const double id = 1.0 / det;
  inv[0] = c00 * id; inv[1] = (I[2] * I[7] - I[1] * I[8]) * id; inv[2] = (I[1] * I[5] - I[2] * I[4]) * id;
  inv[3] = c01 * id; inv[4] = (I[0] * I[8] - I[2] * I[6]) * id; inv[5] = (I[2] * I[3] - I[0] * I[5]) * id;
  inv[6] = c02 * id; inv[7] = (I[1] * I[6] - I[0] * I[7]) * id; inv[8] = m2 * id;
  double mx = 0.0;
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 9; k++) {
    finite = finite && __builtin_isfinite(I[k]);
    mx = fmax(mx, fabs(I[k]));
  }
  const double tol = PLANT_MODEL_SYM_TOL * mx;
  const bool sym = !(fabs(I[1] - I[3]) > tol) && !(fabs(I[2] - I[6]) > tol) && !(fabs(I[5] - I[7]) > tol);
  const bool pd = I[0] > 0.0 && m2 > 0.0 && det > 0.0;
  return !(finite && sym && pd);
}

// The lane's own body: mass and Ib from the model's arrays where the instantiation carries them, from the call's constants otherwise
// (b.Ib_inv: the general inverse, or the one the handle holds); g and dt are the call's.  Returns the model's flag bits.
template <bool MASS, bool IB>
QC_DEV int model_body(const BodyConst& a, const PlantModelArgs& m, long i, BodyConst& b) {
  int bad = 0;
  if constexpr (MASS) {
    b.mass = m.mass[i];
    if (!(__builtin_isfinite(b.mass) && b.mass > 0.0)) bad |= PLANT_MODEL_BAD_MASS;
  } else {
    b.mass = a.mass;
  }
  if constexpr (IB) {
    load9(m.Ib, i, b.Ib);
    if (inertia_inverse_general(b.Ib, b.Ib_inv)) bad |= PLANT_MODEL_BAD_IB;
  } else {
#pragma unroll
    for (int k = 0; k < 9; k++) {
      b.Ib[k] = a.Ib[k];
      b.Ib_inv[k] = a.Ib_inv[k];
    }
  }
  b.g = a.g;
  b.dt = a.dt;
  return bad;
}

// (F, M) of robot i, or +0.0
template <bool WRENCH>
QC_DEV void load_wrench(const PlantModelArgs& m, long i, double (&fs)[3], double (&tau)[3]) {
  if constexpr (WRENCH) {
    load3(m.wrench, 2 * i, fs);
    load3(m.wrench, 2 * i + 1, tau);
  } else {
    fs[0] = fs[1] = fs[2] = 0.0;
    tau[0] = tau[1] = tau[2] = 0.0;
  }
}

template <int N>
QC_DEV void fill_nan(double (&v)[N]) {
#pragma unroll
  for (int k = 0; k < N; k++) v[k] = __builtin_nan("");
}

// plant_step_kernel (qc_plant.hpp) on the model's body
template <bool MASS, bool IB, bool WRENCH>
__global__ __launch_bounds__(PLANT_BLOCK) void plant_step_model_kernel(const long n, const PlantArgs a, const PlantModelArgs md) {
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
  BodyConst b;
  const int bad = model_body<MASS, IB>(a, md, i, b);
  // net force and moment about the centre of mass, world frame: the wrench, then the legs
  double fs[3], tau[3];
  load_wrench<WRENCH>(md, i, fs, tau);
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
  rigid_body_step(b, R, x, v, w, fs, tau, Rn);
  if (bad) {  // a refused body: every state output of this robot's step is NaN
    fill_nan(Rn);
    fill_nan(x);
    fill_nan(v);
    fill_nan(w);
  }
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
  if (md.flags) md.flags[i] = bad;
}

// leg_plant_step_kernel (qc_leg_plant.hpp) on the model's body
template <bool MASS, bool IB, bool WRENCH>
__global__ __launch_bounds__(LEG_PLANT_BLOCK) void leg_plant_step_model_kernel(const DevParams* __restrict__ Pg, const long n, const LegPlantArgs a,
                                                                               const PlantModelArgs md) {
  const long i = (long)blockIdx.x * LEG_PLANT_BLOCK + threadIdx.x;
  if (i >= n) return;  // tail lanes
  CParams& P = *QC_PARAMS_HERE(Pg);
  double R[9], x[3], v[3], w[3], q[4][3], qd[4][3], tq[4][3];
  load9(a.Rwb, i, R);
  load3(a.x, i, x);
  load3(a.xdot, i, v);
  load3(a.w, i, w);
#pragma unroll
  for (int l = 0; l < 4; l++) {
    load3(a.joint_q, 4 * i + l, q[l]);
    load3(a.joint_qdot, 4 * i + l, qd[l]);
    load3(a.joint_tau, 4 * i + l, tq[l]);
  }
  double ph[4] = {0.0, 0.0, 0.0, 0.0};
  if (a.gait_phase && !a.stance) {
#pragma unroll
    for (int l = 0; l < 4; l++) ph[l] = a.gait_phase[4 * i + l];
  }
  const uint32_t sw = a.stance ? *reinterpret_cast<const uint32_t*>(a.stance + 4 * i) : 0u;
  const double duty = a.gait_duty ? a.gait_duty[i] : P.stance_phase;
  const bool running = a.cmd_state ? a.cmd_state[i].gait_running != 0 : true;
  const uint32_t mask = contact_mask(a.stance != nullptr, sw, a.gait_phase != nullptr, ph, duty, running);
  BodyConst b;
  const int bad = model_body<MASS, IB>(a, md, i, b);

  // force pass: the wrench, then the stance legs; swing joints integrate
  double fs[3], tau[3];
  load_wrench<WRENCH>(md, i, fs, tau);
  double c[4][3];  // x + Rwb FK(q): the pinned contact point of a stance leg
  int flags = 0;
#pragma unroll
  for (int l = 0; l < 4; l++) {
    const LegGeom lg = {P.links[3 * l], P.links[3 * l + 1], P.links[3 * l + 2], P.hip[3 * l], P.hip[3 * l + 1], P.hip[3 * l + 2]};
    const LegTrig t = leg_trig(q[l]);
    double p[3], r[3];
    leg_fk(P, l, t, p);
    mat_vec(R, p, r);
#pragma unroll
    for (int k = 0; k < 3; k++) c[l][k] = x[k] + r[k];
    if (mask & (1u << l)) {
      double g[3], rg[3], f[3], m[3];
      if (leg_force_from_torque(lg, t, tq[l], g)) flags |= 1 << l;
      mat_vec(R, g, rg);
#pragma unroll
      for (int k = 0; k < 3; k++) f[k] = -rg[k];
      cross3(r, f, m);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        fs[k] += f[k];
        tau[k] += m[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 3; k++) {
        qd[l][k] += a.dt * (tq[l][k] / a.leg_inertia[k]);
        q[l][k] += a.dt * qd[l][k];
      }
    }
  }
  double Rn[9];
  rigid_body_step(b, R, x, v, w, fs, tau, Rn);
  // IK pass: the stance feet stay where they were
#pragma unroll
  for (int l = 0; l < 4; l++) {
    if (mask & (1u << l)) {
      const LegGeom lg = {P.links[3 * l], P.links[3 * l + 1], P.links[3 * l + 2], P.hip[3 * l], P.hip[3 * l + 1], P.hip[3 * l + 2]};
      const double d[3] = {c[l][0] - x[0], c[l][1] - x[1], c[l][2] - x[2]};
      double pb[3], qn[3];
      mat_t_vec(Rn, d, pb);
      if (leg_ik(lg, pb, qn)) flags |= 16 << l;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        qd[l][k] = wrap_PI(qn[k] - q[l][k]) / a.dt;
        q[l][k] = qn[k];
      }
    }
  }
  if (bad) {  // a refused body: every state output of this robot's step is NaN (foot_world and the step's own flags keep their meaning)
    fill_nan(Rn);
    fill_nan(x);
    fill_nan(v);
    fill_nan(w);
#pragma unroll
    for (int l = 0; l < 4; l++) {
      fill_nan(q[l]);
      fill_nan(qd[l]);
    }
  }
  // every input of this robot has been read: the outputs may overwrite them
  {
    double* o = a.Rwb + 9 * i;
#pragma unroll
    for (int k = 0; k < 9; k++) o[k] = Rn[k];
  }
  store3(a.x, i, x);
  store3(a.xdot, i, v);
  store3(a.w, i, w);
#pragma unroll
  for (int l = 0; l < 4; l++) {
    store3(a.joint_q, 4 * i + l, q[l]);
    store3(a.joint_qdot, 4 * i + l, qd[l]);
    if (a.foot_world) store3(a.foot_world, 4 * i + l, c[l]);
  }
  if (a.flags) a.flags[i] = flags;
  if (md.flags) md.flags[i] = bad;
}

// plant_step_adjoint_kernel (qc_plant_adjoint.hpp) on the model's body, with the model's three cotangents
template <bool MASS, bool IB, bool WRENCH>
__global__ __launch_bounds__(PLANT_BLOCK) void plant_step_model_adjoint_kernel(const long n, const PlantAdjointArgs a, const PlantModelArgs md,
                                                                               const PlantModelBarArgs mb) {
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
  BodyConst b;
  const int bad = model_body<MASS, IB>(a, md, i, b);

  // ---- the forward step, as plant_step_model_kernel and rigid_body_step evaluate it
  double fs[3], tau[3];
  load_wrench<WRENCH>(md, i, fs, tau);
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
  mat_vec(b.Ib, wb, Iwb);
  mat_vec(R, Iwb, Iw_w);
  cross3(w, Iw_w, gyro);
#pragma unroll
  for (int k = 0; k < 3; k++) tau[k] -= gyro[k];
  mat_t_vec(R, tau, nb);
  mat_vec(b.Ib_inv, nb, Inb);
  mat_vec(R, Inb, wdot);
  double x1[3], phi[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double acc = fs[k] / b.mass - (k == 2 ? b.g : 0.0);
    const double v1 = v[k] + b.dt * acc;
    x1[k] = x[k] + b.dt * v1;
    phi[k] = b.dt * (w[k] + b.dt * wdot[k]);
  }
  const double xx = phi[0] * phi[0], yy = phi[1] * phi[1], zz = phi[2] * phi[2];
  const double th2 = xx + yy + zz;
  const double h = 0.5 * sqrt(th2);
  double sh, ch;
  sincos_joint(h, &sh, &ch);
  const double sc = h > 0.0 ? sh / h : 1.0;
  const double A = sc * ch, B = 0.5 * (sc * sc);

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
    w1b[k] += b.dt * phib[k];
    wbar[k] = w1b[k];
    wdotb[k] = b.dt * w1b[k];
    v1b[k] += b.dt * x1b[k];
    fsb[k] = b.dt * v1b[k] / b.mass;
  }
  // a = fs / m - g e_z:  mass_bar = -<fs, a_bar> / m^2, a_bar = m fsb
  double massb = -(fs[0] * fsb[0] + fs[1] * fsb[1] + fs[2] * fsb[2]) / b.mass;
  // wdot = R Ib^-1 R^T tau,  tau = (M + sum r x f) - w x (R Ib R^T w)
  double Inbb[3], nbb[3], taub[3], Iwwb[3], Iwbb[3], wbb[3], t[3];
  add_outer(Rb, wdotb, Inb);
  mat_t_vec(R, wdotb, Inbb);
  mat_t_vec(b.Ib_inv, Inbb, nbb);
  add_outer(Rb, tau, nbb);
  mat_vec(R, nbb, taub);
  cross3(taub, Iw_w, t);  // Iw_w x gyrob, gyrob = -taub
  cross3(w, taub, Iwwb);  // gyrob x w
  add_outer(Rb, Iwwb, Iwb);
  mat_t_vec(R, Iwwb, Iwbb);
  mat_t_vec(b.Ib, Iwbb, wbb);
  add_outer(Rb, w, wbb);
  {
    double Rwbb[3];
    mat_vec(R, wbb, Rwbb);
#pragma unroll
    for (int k = 0; k < 3; k++) wbar[k] += t[k] + Rwbb[k];
  }
  // Iwb = Ib wb, Inb = Ib^-1 nb:  Ib_bar = Iwbb wb^T - (Ib^-T Inbb) Inb^T
  double Ibb[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) Ibb[3 * r + c] = Iwbb[r] * wb[c] - nbb[r] * Inb[c];
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
  if (bad) {  // a refused body: NaN in every output of this robot's row
    fill_nan(Rb);
    fill_nan(xbar);
    fill_nan(v1b);
    fill_nan(wbar);
    fill_nan(fsb);
    fill_nan(taub);
    fill_nan(Ibb);
    massb = __builtin_nan("");
#pragma unroll
    for (int l = 0; l < 4; l++) {
      fill_nan(gbb[l]);
      fill_nan(pwb[l]);
    }
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
  if (mb.wrench_bar) {
    store3(mb.wrench_bar, 2 * i, fsb);
    store3(mb.wrench_bar, 2 * i + 1, taub);
  }
  if (mb.mass_bar) mb.mass_bar[i] = massb;
  if (mb.Ib_bar) {
    double* q = mb.Ib_bar + 9 * i;
#pragma unroll
    for (int k = 0; k < 9; k++) q[k] = Ibb[k];
  }
  if (mb.flags) mb.flags[i] = bad;
}

}  // namespace qc
#endif  // __HIPCC__
