// qc_leg_plant_adjoint.hpp - the reverse pass of the legged plant step (qc_leg_plant.hpp): qc_leg_plant_step_adjoint_batch
// (include/qc_balance.h), the kernel between fused_tick_autograd() and backpropagation through the closed loop around the tick.
//
// Given the state BEFORE a step, the torques and the contact inputs the step read, and cotangents on what the step wrote (Rwb', x',
// xdot', w', joint_q', joint_qdot'), it writes the cotangents of Rwb, x, xdot, w, joint_q, joint_qdot and joint_tau: the
// transpose-Jacobian of the step exactly as leg_plant_step_kernel evaluates it.  Matrix cotangents are ENTRYWISE, as in
// qc_plant_adjoint.hpp.  Nothing is saved by the forward launch: the kernel recomputes the forward step - force pass, body, IK.
//
// The reverse pass, in the notation of qc_leg_plant.hpp (a cotangent of v is vb; q', qd' are the step's joint outputs):
//   stance leg, IK end   qnb = q'b + qd'b / dt,  qb = -qd'b / dt                                      (wrap_PI has slope 1)
//                        pbb = (dIK / dpb)^T qnb = J(qn)^-T qnb: inside reach and on the q3 <= 0 branch leg_ik inverts leg_fk, so
//                        its derivative is the inverse leg Jacobian AT THE ANGLES IT RETURNED (tests/test_leg_plant_adjoint_cpu.py
//                        holds that against the 50-digit derivative of the atan2 / sqrt chain as written): leg_force_from_torque at
//                        leg_trig(qn) with its band rule
//                        pb = Rn^T d, d = c - x':  Rnb += d pbb^T,  db = Rn pbb,  cb = db,  x'b -= db
//   body                 qc_plant_adjoint.hpp's Exp / product / Euler / wdot block, from (Rnb, x'b, xdot'b, w'b) to
//                        (Rb, xb, xdotb, wb, fsb, taub)
//   stance leg, force    fb = fsb + taub x r,  rb = f x taub + cb,  xb += cb,  gb = -R^T fb,  Rb -= fb g^T
//                        r = R p:  Rb += rb p^T,  pb = R^T rb,  qb += J(q)^T pb                                   (leg_jt_force)
//                        g = J^-T tau:  y = J^-1 gb,  joint_taub = y,  qb -= G(g) y   (G = sum_r g_r H_r: the six entries of
//                        qc_sensitivity_kin.hpp)
//                        joint_qdotb = 0: the stance leg's qdot is not read by the step
//   swing leg            s = qd'b + dt q'b;  qb = q'b,  joint_qdotb = s,  joint_taub = dt s / leg_inertia
// The step is linear in a swing leg's joint_qdot and reads no stance leg's: the kernel does not load that array.
//
// UNDEFINED GRADIENTS.  flags bit l: J(q_l) of a stance leg is outside leg_force_from_torque's band - the forward step took the
// pseudo-inverse, which this pass does not differentiate.  Bit 4 + l: the forward IK reported the foot out of reach (the clamp at
// d = 1 has no slope, d < -1 is NaN), or J(qn_l) is outside the band.  A robot with any bit set gets NaN in every output row.
// Other non-finite inputs propagate as NaN; nothing is clamped.  (A foot inside the hip roll's cylinder, y^2 + z^2 < l1^2, where
// leg_ik clamps the root at 0, is in reach by the forward rule and unflagged: the IK no longer inverts the FK there, and the
// gradient is that of the unclamped map.  No posture of a standing or walking robot comes near it.)
//
// OUT OF SCOPE: a cotangent on the optional foot_world output; gradients in mass, Ib, leg_inertia, dt and the kinematic constants as
// the plant uses them; the swing legs' PD torques (the tick's side: qc_sensitivity_kin.hpp); commander mode (cmd_state only resolves
// the contact mask here, as in the forward step); the gait clock (the mask is piecewise constant: no gradient in the phases).
//
// Kernel: qc_leg_plant.hpp's shape - ONE LANE PER ROBOT, FP64, blocks of LEG_PLANT_BLOCK, tail lanes return, no LDS, no scratch,
// the four legs unrolled.  Across the body's block a lane keeps per leg q, g and c's cotangent (9 doubles; qn is used where the IK
// returns it) and the three joint cotangents (9), and recomputes the trigonometry where the reverse pass needs it: at q for J^T,
// J^-1 and G, at qn for J^-T.  A block of 256 lanes has 512 registers per lane (VGPR + AGPR) on gfx950, which qc_sensitivity.hpp
// relies on as well (profiles/leg_plant_adjoint_kernel_resources.txt has the counts).  The body's block is RESTATED from qc_plant_adjoint.hpp, which
// stays as it is: here the forward half forms E and Rn as rigid_body_step does (the IK reads Rn), there neither is formed.
// A NULL input cotangent is zero; a NULL output is not stored.  A lane reads ALL of its inputs before it writes anything and
// touches only its own rows, so an output may be the same array as an input cotangent of the same layout (joint_q_bar over
// joint_q_next_bar, joint_qdot_bar or joint_tau_bar over joint_qdot_next_bar, x_bar over x_next_bar, ...).
#pragma once
#include "qc_leg_plant.hpp"
#include "qc_plant_adjoint.hpp"

namespace qc {

struct LegPlantAdjointArgs : BodyConst {
  double leg_inertia[3];
  const double *Rwb, *x, *xdot, *w;                 // [n][9], [n][3] x 3: the state BEFORE the step
  const double *joint_q, *joint_qdot, *joint_tau;   // [n][4][3]
  const uint8_t* stance;                            // the contact inputs of the forward call, optional
  const double* gait_phase;
  const double* gait_duty;
  const CmdState* cmd_state;
  const double *Rwb_next_bar, *x_next_bar, *xdot_next_bar, *w_next_bar, *joint_q_next_bar, *joint_qdot_next_bar;  // optional IN (nullptr: zero)
  double *Rwb_bar, *x_bar, *xdot_bar, *w_bar, *joint_q_bar, *joint_qdot_bar, *joint_tau_bar;                      // optional OUT
  int32_t* flags;                                   // optional OUT
};

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

// y = J^-1 v for the leg Jacobian at t by the cofactors over det: the transpose of leg_force_from_torque's closed form.  No band
// rule of its own - the caller holds the leg's band bit from the forward pass and discards the robot when it is set.
QC_DEV void leg_jacobian_solve(const LegGeom& lg, const LegTrig& t, const double (&v)[3], double (&y)[3]) {
  const double L1 = lg.L1, L2 = lg.L2, L3 = lg.L3;
  const double a = L2 * t.c2 + L3 * t.c23, b = L2 * t.s2 + L3 * t.s23;
  const double J[9] = {0.0, a, L3 * t.c23, -L1 * t.s1 - a * t.c1, b * t.s1, L3 * t.s1 * t.s23, L1 * t.c1 - a * t.s1, -b * t.c1, -L3 * t.s23 * t.c1};
  const double c00 = J[4] * J[8] - J[5] * J[7], c01 = J[5] * J[6] - J[3] * J[8], c02 = J[3] * J[7] - J[4] * J[6];
  const double c10 = J[2] * J[7] - J[1] * J[8], c11 = J[0] * J[8] - J[2] * J[6], c12 = J[1] * J[6] - J[0] * J[7];
  const double c20 = J[1] * J[5] - J[2] * J[4], c21 = J[2] * J[3] - J[0] * J[5], c22 = J[0] * J[4] - J[1] * J[3];
  const double id = 1.0 / (J[0] * c00 + J[1] * c01 + J[2] * c02);
  // J^-1 = cof(J)^T / det: column c of the cofactor matrix dotted with v
  y[0] = id * (c00 * v[0] + c10 * v[1] + c20 * v[2]);
  y[1] = id * (c01 * v[0] + c11 * v[1] + c21 * v[2]);
  y[2] = id * (c02 * v[0] + c12 * v[1] + c22 * v[2]);
}

// o = G(g) y,  G = sum_r g_r d^2 p_r / d q^2 (symmetric; the six entries of qc_sensitivity_kin.hpp)
QC_DEV void leg_fk_hessian_apply(const LegGeom& lg, const LegTrig& t, const double (&g)[3], const double (&y)[3], double (&o)[3]) {
  const double ja = lg.L2 * t.c2 + lg.L3 * t.c23, jb = lg.L2 * t.s2 + lg.L3 * t.s23;
  const double jd = lg.L3 * t.c23, je = lg.L3 * t.s23;
  const double u = g[1] * t.c1 + g[2] * t.s1, v = g[1] * t.s1 - g[2] * t.c1;
  const double G00 = ja * v - lg.L1 * u, G01 = jb * u, G02 = je * u, G11 = ja * v - g[0] * jb, G12 = jd * v - g[0] * je;
  o[0] = G00 * y[0] + G01 * y[1] + G02 * y[2];
  o[1] = G01 * y[0] + G11 * y[1] + G12 * y[2];
  o[2] = G02 * y[0] + G12 * y[1] + G12 * y[2];
}

__global__ __launch_bounds__(LEG_PLANT_BLOCK) void leg_plant_step_adjoint_kernel(const DevParams* __restrict__ Pg, const long n, const LegPlantAdjointArgs a) {
  const long i = (long)blockIdx.x * LEG_PLANT_BLOCK + threadIdx.x;
  if (i >= n) return;  // tail lanes
  CParams& P = *QC_PARAMS_HERE(Pg);
  double R[9], x[3], v[3], w[3], q[4][3], g[4][3];  // g: the torques first, then the forces they encode
  load9(a.Rwb, i, R);
  load3(a.x, i, x);
  load3(a.xdot, i, v);
  load3(a.w, i, w);
#pragma unroll
  for (int l = 0; l < 4; l++) {
    load3(a.joint_q, 4 * i + l, q[l]);
    load3(a.joint_tau, 4 * i + l, g[l]);
  }
  const uint32_t mask = load_contact_mask(&P, a.stance, a.gait_phase, a.gait_duty, i, a.cmd_state ? a.cmd_state[i].gait_running != 0 : true);
  double Rnb[9], x1b[3], v1b[3], w1b[3], qb[4][3], sb[4][3];  // qb: q'b first, sb: qd'b first
  if (a.Rwb_next_bar) load9(a.Rwb_next_bar, i, Rnb);
  else {
#pragma unroll
    for (int k = 0; k < 9; k++) Rnb[k] = 0.0;
  }
  load3_or_zero(a.x_next_bar, i, x1b);
  load3_or_zero(a.xdot_next_bar, i, v1b);
  load3_or_zero(a.w_next_bar, i, w1b);
#pragma unroll
  for (int l = 0; l < 4; l++) {
    load3_or_zero(a.joint_q_next_bar, 4 * i + l, qb[l]);
    load3_or_zero(a.joint_qdot_next_bar, 4 * i + l, sb[l]);
  }

  // ---- the forward step, as leg_plant_step_kernel and rigid_body_step evaluate it
  double fs[3] = {0.0, 0.0, 0.0}, tau[3] = {0.0, 0.0, 0.0};
  double c[4][3];
  int flags = 0;
#pragma unroll
  for (int l = 0; l < 4; l++) {
    if (mask & (1u << l)) {
      const LegGeom lg = {P.links[3 * l], P.links[3 * l + 1], P.links[3 * l + 2], P.hip[3 * l], P.hip[3 * l + 1], P.hip[3 * l + 2]};
      const LegTrig t = leg_trig(q[l]);
      double p[3], r[3], gl[3], rg[3], f[3], m[3];
      leg_fk(P, l, t, p);
      mat_vec(R, p, r);
      if (leg_force_from_torque(lg, t, g[l], gl)) flags |= 1 << l;
      mat_vec(R, gl, rg);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        c[l][k] = x[k] + r[k];
        g[l][k] = gl[k];
        f[k] = -rg[k];
      }
      cross3(r, f, m);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        fs[k] += f[k];
        tau[k] += m[k];
      }
    }
  }
  double Iwb[3], Iw_w[3], Inb[3], x1[3], phi[3], Rn[9];
  {
    double wb[3], gyro[3], nb[3], wdot[3];
    mat_t_vec(R, w, wb);
    mat_vec(a.Ib, wb, Iwb);
    mat_vec(R, Iwb, Iw_w);
    cross3(w, Iw_w, gyro);
#pragma unroll
    for (int k = 0; k < 3; k++) tau[k] -= gyro[k];
    mat_t_vec(R, tau, nb);
    mat_vec(a.Ib_inv, nb, Inb);
    mat_vec(R, Inb, wdot);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double acc = fs[k] / a.mass - (k == 2 ? a.g : 0.0);
      const double v1 = v[k] + a.dt * acc;
      x1[k] = x[k] + a.dt * v1;
      phi[k] = a.dt * (w[k] + a.dt * wdot[k]);
    }
  }
  const double xx = phi[0] * phi[0], yy = phi[1] * phi[1], zz = phi[2] * phi[2];
  const double th2 = xx + yy + zz;
  const double h = 0.5 * sqrt(th2);
  double sh, ch;
  sincos_joint(h, &sh, &ch);
  const double sc = h > 0.0 ? sh / h : 1.0;
  const double A = sc * ch, B = 0.5 * (sc * sc);
  {
    const double E[9] = {1.0 - B * (yy + zz),                 B * (phi[0] * phi[1]) - A * phi[2], B * (phi[0] * phi[2]) + A * phi[1],
                         B * (phi[0] * phi[1]) + A * phi[2], 1.0 - B * (xx + zz),                 B * (phi[1] * phi[2]) - A * phi[0],
                         B * (phi[0] * phi[2]) - A * phi[1], B * (phi[1] * phi[2]) + A * phi[0], 1.0 - B * (xx + yy)};
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int k = 0; k < 3; k++) Rn[3 * r + k] = E[3 * r] * R[k] + E[3 * r + 1] * R[3 + k] + E[3 * r + 2] * R[6 + k];
  }

  // ---- the reverse pass: the joints' end.  (The legs' constants are fetched again in each of the three passes over the legs: held
  // from the first pass on, the 24 of them overflow the scalar registers.)
  double tqb[4][3];
  CParams& P2 = *QC_PARAMS_HERE(Pg);
#pragma unroll
  for (int l = 0; l < 4; l++) {
    if (mask & (1u << l)) {
      const LegGeom lg = {P2.links[3 * l], P2.links[3 * l + 1], P2.links[3 * l + 2], P2.hip[3 * l], P2.hip[3 * l + 1], P2.hip[3 * l + 2]};
      const double d[3] = {c[l][0] - x1[0], c[l][1] - x1[1], c[l][2] - x1[2]};
      double pb[3], qn[3], qnb[3], pbb[3], db[3];
      mat_t_vec(Rn, d, pb);
      if (leg_ik(lg, pb, qn)) flags |= 16 << l;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const double s = sb[l][k] / a.dt;
        qnb[k] = qb[l][k] + s;
        qb[l][k] = -s;
        sb[l][k] = 0.0;  // joint_qdotb of a stance leg
      }
      if (leg_force_from_torque(lg, leg_trig(qn), qnb, pbb)) flags |= 16 << l;
      add_outer(Rnb, d, pbb);
      mat_vec(Rn, pbb, db);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        c[l][k] = db[k];  // c's place holds cb from here on
        x1b[k] -= db[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 3; k++) {
        sb[l][k] += a.dt * qb[l][k];
        tqb[l][k] = a.dt * sb[l][k] / a.leg_inertia[k];
      }
    }
  }
  // ---- the body (qc_plant_adjoint.hpp): Rn = E R, E = Exp(phi), the semi-implicit Euler step, wdot
  double Rb[9], phib[3];
  {
    double M[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int k = 0; k < 3; k++) M[3 * r + k] = Rnb[3 * r] * R[3 * k] + Rnb[3 * r + 1] * R[3 * k + 1] + Rnb[3 * r + 2] * R[3 * k + 2];  // Rnb R^T
#pragma unroll
    for (int k = 0; k < 3; k++) {  // E^T Rnb, column by column (E^T = Exp(-phi))
      const double col[3] = {Rnb[k], Rnb[3 + k], Rnb[6 + k]};
      double o[3];
      exp_apply(phi, -A, B, col, o);
      Rb[k] = o[0]; Rb[3 + k] = o[1]; Rb[6 + k] = o[2];
    }
    double A1, B1;
    exp_coefficient_slopes(th2, sh, A, B, &A1, &B1);
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
  double wbar[3], wdotb[3], fsb[3], taub[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    w1b[k] += a.dt * phib[k];
    wbar[k] = w1b[k];
    wdotb[k] = a.dt * w1b[k];
    v1b[k] += a.dt * x1b[k];
    fsb[k] = a.dt * v1b[k] / a.mass;
  }
  {
    double Inbb[3], nbb[3], Iwwb[3], Iwbb[3], wbb[3], t[3], Rwbb[3];
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
    mat_vec(R, wbb, Rwbb);
#pragma unroll
    for (int k = 0; k < 3; k++) wbar[k] += t[k] + Rwbb[k];
  }
  // ---- the stance legs' forces, moments and pinned points
  double xbar[3] = {x1b[0], x1b[1], x1b[2]};
  CParams& P3 = *QC_PARAMS_HERE(Pg);
#pragma unroll
  for (int l = 0; l < 4; l++) {
    if (mask & (1u << l)) {
      const LegGeom lg = {P3.links[3 * l], P3.links[3 * l + 1], P3.links[3 * l + 2], P3.hip[3 * l], P3.hip[3 * l + 1], P3.hip[3 * l + 2]};
      const LegTrig t = leg_trig(q[l]);
      double p[3], r[3], rg[3], f[3], fb[3], rb[3], gb[3], pb[3], jt[3], gy[3];
      leg_fk(P3, l, t, p);
      mat_vec(R, p, r);
      mat_vec(R, g[l], rg);
#pragma unroll
      for (int k = 0; k < 3; k++) f[k] = -rg[k];
      cross3(taub, r, fb);
      cross3(f, taub, rb);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        fb[k] += fsb[k];
        rb[k] += c[l][k];
        xbar[k] += c[l][k];
      }
      mat_t_vec(R, fb, gb);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        gb[k] = -gb[k];
        fb[k] = -fb[k];
      }
      add_outer(Rb, fb, g[l]);
      add_outer(Rb, rb, p);
      mat_t_vec(R, rb, pb);
      leg_jt_force(lg, t, pb, jt);
      leg_jacobian_solve(lg, t, gb, tqb[l]);
      leg_fk_hessian_apply(lg, t, g[l], tqb[l], gy);
#pragma unroll
      for (int k = 0; k < 3; k++) qb[l][k] += jt[k] - gy[k];
    }
  }
  // every input of this robot has been read: an output may overwrite an input cotangent.  A flagged robot has no gradient.
  const double nan = __builtin_nan("");
  const bool bad = flags != 0;
  if (a.Rwb_bar) {
    double* o = a.Rwb_bar + 9 * i;
#pragma unroll
    for (int k = 0; k < 9; k++) o[k] = bad ? nan : Rb[k];
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    xbar[k] = bad ? nan : xbar[k];
    v1b[k] = bad ? nan : v1b[k];
    wbar[k] = bad ? nan : wbar[k];
  }
  if (a.x_bar) store3(a.x_bar, i, xbar);
  if (a.xdot_bar) store3(a.xdot_bar, i, v1b);
  if (a.w_bar) store3(a.w_bar, i, wbar);
#pragma unroll
  for (int l = 0; l < 4; l++) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      qb[l][k] = bad ? nan : qb[l][k];
      sb[l][k] = bad ? nan : sb[l][k];
      tqb[l][k] = bad ? nan : tqb[l][k];
    }
    if (a.joint_q_bar) store3(a.joint_q_bar, 4 * i + l, qb[l]);
    if (a.joint_qdot_bar) store3(a.joint_qdot_bar, 4 * i + l, sb[l]);
    if (a.joint_tau_bar) store3(a.joint_tau_bar, 4 * i + l, tqb[l]);
  }
  if (a.flags) a.flags[i] = flags;
}

}  // namespace qc
#endif  // __HIPCC__
