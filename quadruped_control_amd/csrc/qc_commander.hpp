// qc_commander.hpp - the commander step of the tick as a launch of its own (qc_commander_step_batch, include/qc_balance.h) and its
// reverse pass (qc_commander_step_adjoint_batch): from the measured pose and the user's body twist to the desired state the QP and the
// foothold planner are fed - the stage through which a loss on a rollout reaches THE COMMAND.
//
// FORWARD, per robot: the tick's own commander_step (qc_device.hpp - one function, so the values are
// the tick's bit for bit, tests/test_gpu_commander_adjoint.py) behind the loads fetch_extra / fetch_state make in commander mode:
//   vb = fresh ? twist : Vb; a fresh command sets cmd_pending and is stored as Vb
//   standing latches once |x_z - stand_height| < stand_tol
//   standing, not running:  gait_running is set, nothing else
//   standing, running, pending: APPLIED - with v = vb[0:3], om = vb[3:6], d = cmd_dt om, Rb = Exp(d) (I below |d| = 1e-12), t = cmd_dt Rb v,
//                               Y = Rz(yaw), (cy, sy) = (R00, R10) / h, h = hypot(R00, R10) (yaw 0 where h == 0 or not finite below 1e300):
//       Rwb_d = Y Rb,  x_d = (x0 + (Y t)0, x1 + (Y t)1, stand_height),  xdot_d = Rwb^T (v - x x om),  w_d = Rwb^T om
//     stored into the record; cmd_pending cleared
// The record is updated in place exactly as the tick does it.  Outputs: the desired state the tick would feed the QP THIS tick (the
// record's own where no command was applied), `run` (standing and running before the call) and `applied`.
//
// REVERSE.  Nothing is saved: the caller passes Rwb, x, twist, fresh, the three scalars and the records from BEFORE the forward call;
// fresh / standing / running / pending / applied are recomputed and held.  A cotangent of v is vb.  G = Rwb_d_bar (entrywise,
// row-major), a = x_d_bar, b = xdot_d_bar, c = w_d_bar, n = Vb_next_bar; a missing one counts as zero.
//   not applied:  the four _prev_bar = G, a, b, c (the record passed through); Rwb_bar = Rwb_bar_in, x_bar = x_bar_in; vb_bar = n
//   applied:      the four _prev_bar = 0 (the record was overwritten); a_2 is dropped (the height is a constant); with u = v - x x om:
//     ub = Rwb b,  Rwb_bar[i][k] += u_i b_k + om_i c_k,  v_bar = ub,  om_bar = Rwb c + x x ub,  x_bar += ub x om + (a_0, a_1, 0)
//     tb = Y^T (a_0, a_1, 0),  M = Y^T G + cmd_dt tb v^T (the total on Rb),  v_bar += cmd_dt Rb^T tb
//     cy_bar = a_0 t_0 + a_1 t_1 + sum_j G_0j Rb_0j + G_1j Rb_1j,  sy_bar = a_1 t_0 - a_0 t_1 + sum_j G_1j Rb_0j - G_0j Rb_1j
//     q = cy_bar sy - sy_bar cy:  Rwb_bar[0] += sy q / h,  Rwb_bar[3] -= cy q / h           (the yaw normalisation)
//     wv = axial(M Rb^T) = (N_21 - N_12, N_02 - N_20, N_10 - N_01),  d_bar = Jl(d)^T wv = wv - A d x wv + B d x (d x wv),
//       A = (1 - cos th) / th^2 = (sin(th / 2) / (th / 2))^2 / 2,  B = (th - sin th) / th^3,  th = |d|;  om_bar += cmd_dt d_bar
//     SMALL-ANGLE BRANCH (th < 1e-12, where the forward pass takes Rb = I): the SMOOTH function is differentiated, not the branch as
//       written (whose derivative in om is zero) - Rb = Exp(d), A, B by the same formulas down to th = 0, where Rb = I, d_bar = wv:
//       delta Rb = [delta d]x, delta t = cmd_dt [delta d]x v.  A twist without angular rate is where an optimisation starts, and
//       its yaw rate must get a gradient; B takes its series below th = 1e-4
//     vb_bar = n + (v_bar, om_bar)
//   command source: fresh: twist_bar = vb_bar, Vb_bar = 0;  held: Vb_bar = vb_bar, twist_bar = 0
// UNDEFINED GRADIENT: `flags` bit 0 - a command is applied at the gimbal-lock branch (h == 0 or not finite below 1e300); every output
// row of that robot is NaN.  Other non-finite inputs propagate; nothing is clamped.  NO cotangent of stand_height, stand_tol, cmd_dt;
// the flags and latches are held.
//
// Kernels: ONE LANE PER ROBOT, FP64, no LDS, no atomics, 0 B scratch (profiles/commander_adjoint_kernel_resources.txt).  Launch geometry,
// the "n beyond one launch" refusal and the tail lanes are qc_swing_reference.hpp's.  Both read every input of a robot before they
// write any of its outputs, and a lane writes its own robot only: an output may be the same array as its `_in` or as the incoming
// cotangent of its layout.
#pragma once
#include "qc_swing_reference.hpp"

namespace qc {

struct CommanderStepArgs {
  const double *Rwb, *x;             // [n][9], [n][3]
  const double* twist;               // [n][6] or NULL (no fresh command)
  const uint8_t* fresh;              // [n] or NULL
  CmdState* state;                   // [n] IN/OUT
  double stand_height, stand_tol, cmd_dt;
  double *Rwb_d, *x_d, *xdot_d, *w_d;  // optional OUT
  uint8_t *run, *applied;            // [n] optional OUT
};

struct CommanderStepAdjointArgs {
  const double *Rwb, *x, *twist;
  const uint8_t* fresh;
  const CmdState* before;            // [n] the records before the forward call
  double stand_height, stand_tol, cmd_dt;
  const double *Rwb_d_bar, *x_d_bar, *xdot_d_bar, *w_d_bar, *Vb_next_bar;  // optional cotangents
  const double *Rwb_bar_in, *x_bar_in;                                      // optional
  double *twist_bar, *Vb_bar, *Rwb_bar, *x_bar, *Rwb_d_prev_bar, *x_d_prev_bar, *xdot_d_prev_bar, *w_d_prev_bar;  // optional OUT
  int32_t* flags;                    // [n] optional OUT
};

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

__global__ __launch_bounds__(SENSITIVITY_BLOCK) void commander_step_kernel(const long n, const CommanderStepArgs a) {
  for (long base = (long)blockIdx.x * SENSITIVITY_BLOCK; base < n; base += (long)gridDim.x * SENSITIVITY_BLOCK) {
    const long me = base + threadIdx.x;
    const bool live = me < n;
    const long i = live ? me : n - 1;  // tail lanes: the last robot again, nothing stored
    // the batch as the tick sees it in commander mode: fetch_extra and fetch_state's loads, commander_step's stores
    BatchIn in{};
    in.Rwb = a.Rwb;
    in.x = a.x;
    in.cmd_state = a.state;
    in.cmd_twist = a.fresh ? a.twist : nullptr;
    in.cmd_fresh = a.fresh;
    in.stand_height = a.stand_height;
    in.stand_tol = a.stand_tol;
    in.cmd_dt = a.cmd_dt;
    RawState S;
    TickExtra X;
    fetch_extra<true>(in, i, X);
    load9(a.Rwb, i, S.R);
    load3(a.x, i, S.x);
    const CmdState* C = a.state + i;
#pragma unroll
    for (int k = 0; k < 9; k++) S.Rd[k] = C->Rwb_d[k];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      S.xd[k] = C->x_d[k];
      S.xdotd[k] = C->xdot_d[k];
      S.wd[k] = C->w_d[k];
    }
    // (the step's own decision, for the `applied` byte: the record's cmd_pending says the same after the call)
    const bool standing = X.flags[0] || fabs(S.x[2] - a.stand_height) < a.stand_tol;
    const bool applied = standing && X.flags[1] && (X.flags[2] || X.fresh);
    const bool run = commander_step(in, i, live ? 0 : 1, S, X);  // member 0 stores the record
    if (live) {
      if (a.Rwb_d) store_n(a.Rwb_d, i, S.Rd, false);
      if (a.x_d) store_n(a.x_d, i, S.xd, false);
      if (a.xdot_d) store_n(a.xdot_d, i, S.xdotd, false);
      if (a.w_d) store_n(a.w_d, i, S.wd, false);
      if (a.run) a.run[i] = run ? 1 : 0;
      if (a.applied) a.applied[i] = applied ? 1 : 0;
    }
  }
}

__global__ __launch_bounds__(SENSITIVITY_BLOCK) void commander_step_adjoint_kernel(const long n, const CommanderStepAdjointArgs a) {
  for (long base = (long)blockIdx.x * SENSITIVITY_BLOCK; base < n; base += (long)gridDim.x * SENSITIVITY_BLOCK) {
    const long me = base + threadIdx.x;
    const bool live = me < n;
    const long i = live ? me : n - 1;  // tail lanes: the last robot again, nothing stored
    // every input of the robot first: an output may be one of these arrays
    double R[9], x[3], vb[6], G[9], xa[3], b[3], c[3], nb[6], Rbar[9], xb[3];
    load9(a.Rwb, i, R);
    load3(a.x, i, x);
    const CmdState* C = a.before + i;
    const bool fresh = a.fresh && a.fresh[i] != 0;
    const int standing0 = C->standing, running = C->gait_running, pending0 = C->cmd_pending;
#pragma unroll
    for (int k = 0; k < 6; k++) vb[k] = fresh ? a.twist[6 * i + k] : C->Vb[k];
    load_or_zero(a.Rwb_d_bar, i, G);
    load_or_zero(a.x_d_bar, i, xa);
    load_or_zero(a.xdot_d_bar, i, b);
    load_or_zero(a.w_d_bar, i, c);
    load_or_zero(a.Vb_next_bar, i, nb);
    load_or_zero(a.Rwb_bar_in, i, Rbar);
    load_or_zero(a.x_bar_in, i, xb);
    const bool standing = standing0 || fabs(x[2] - a.stand_height) < a.stand_tol;
    const bool applied = standing && running && (pending0 || fresh);
    int fl = 0;
    if (applied) {
      const double dt = a.cmd_dt;
      const double v[3] = {vb[0], vb[1], vb[2]}, om[3] = {vb[3], vb[4], vb[5]};
      const double d[3] = {om[0] * dt, om[1] * dt, om[2] * dt};
      const double th = __builtin_sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
      const bool zero = th == 0.0;  // (a NaN angle takes the formulas and propagates)
      // the forward values the reverse pass needs, of the ANALYTIC function: Rb = Exp(d) also below the forward pass's 1e-12
      // threshold (there it differs from I by less than the threshold), t = dt Rb v, (cy, sy); Jl's coefficients A, B
      double Rb[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3];
      double A = 0.5, B = 1.0 / 6.0;
      if (!zero) {
        double s, co, sh, ch;
        sincos_joint(th, &s, &co);
        sincos_joint(0.5 * th, &sh, &ch);
        const double ax[3] = {d[0] / th, d[1] / th, d[2] / th};
        const double oc = 2.0 * sh * sh;  // 1 - cos th, without the cancellation
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
          for (int j = 0; j < 3; j++) Rb[3 * r + j] = oc * ax[r] * ax[j] + (r == j ? co : 0.0);
        Rb[1] -= s * ax[2]; Rb[3] += s * ax[2];
        Rb[2] += s * ax[1]; Rb[6] -= s * ax[1];
        Rb[5] -= s * ax[0]; Rb[7] += s * ax[0];
        const double q = sh / (0.5 * th);
        A = 0.5 * q * q;
        // (th - sin th) / th^3: the difference is good to EPS th, which B th^2 |wv| turns into EPS |wv|; below 1e-4 the series
        B = th < 1.0e-4 ? (1.0 - th * th / 20.0) / 6.0 : (th - s) / (th * th * th);
      }
#pragma unroll
      for (int r = 0; r < 3; r++) t[r] = (Rb[3 * r] * v[0] + Rb[3 * r + 1] * v[1] + Rb[3 * r + 2] * v[2]) * dt;
      const double h = __builtin_sqrt(R[0] * R[0] + R[3] * R[3]);
      const bool ok = h > 0.0 && h < 1.0e300;
      if (!ok) fl = 1;
      const double cy = R[0] / h, sy = R[3] / h;
      // Ad_T: xdot_d = R^T u, w_d = R^T om
      double xo[3], u[3], ub[3], rc[3], uxo[3], xxu[3];
      cross3(x, om, xo);
#pragma unroll
      for (int k = 0; k < 3; k++) u[k] = v[k] - xo[k];
      mat_vec(R, b, ub);
      mat_vec(R, c, rc);
      cross3(ub, om, uxo);
      cross3(x, ub, xxu);
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) Rbar[3 * r + k] += u[r] * b[k] + om[r] * c[k];
      // the pose: Y t and Y Rb
      const double tb[3] = {cy * xa[0] + sy * xa[1], cy * xa[1] - sy * xa[0], 0.0};
      double M[9];
      double cyb = xa[0] * t[0] + xa[1] * t[1], syb = xa[1] * t[0] - xa[0] * t[1];
#pragma unroll
      for (int j = 0; j < 3; j++) {
        M[j] = cy * G[j] + sy * G[3 + j] + dt * tb[0] * v[j];
        M[3 + j] = cy * G[3 + j] - sy * G[j] + dt * tb[1] * v[j];
        M[6 + j] = G[6 + j];
        cyb += G[j] * Rb[j] + G[3 + j] * Rb[3 + j];
        syb += G[3 + j] * Rb[j] - G[j] * Rb[3 + j];
      }
      const double q = cyb * sy - syb * cy;
      Rbar[0] += sy * q / h;
      Rbar[3] -= cy * q / h;
      // wv = axial(M Rb^T), d_bar = Jl(d)^T wv
      double N[9], wv[3], dw[3], ddw[3], vbar[3], obar[3];
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int k = 0; k < 3; k++) N[3 * r + k] = M[3 * r] * Rb[3 * k] + M[3 * r + 1] * Rb[3 * k + 1] + M[3 * r + 2] * Rb[3 * k + 2];
      wv[0] = N[7] - N[5];
      wv[1] = N[2] - N[6];
      wv[2] = N[3] - N[1];
      cross3(d, wv, dw);
      cross3(d, dw, ddw);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const double db = wv[k] - A * dw[k] + B * ddw[k];
        vbar[k] = ub[k] + dt * (Rb[k] * tb[0] + Rb[3 + k] * tb[1]);  // Rb^T tb, tb_2 = 0
        obar[k] = rc[k] + xxu[k] + dt * db;
      }
#pragma unroll
      for (int k = 0; k < 3; k++) {
        nb[k] += vbar[k];
        nb[3 + k] += obar[k];
        xb[k] += uxo[k] + (k < 2 ? xa[k] : 0.0);
        xa[k] = b[k] = c[k] = 0.0;  // the record was overwritten
      }
#pragma unroll
      for (int k = 0; k < 9; k++) G[k] = 0.0;
    }
    if (live) {
      const bool nan = fl != 0;  // no gradient: every row of the robot
      double tw[6], held[6];  // the command source
#pragma unroll
      for (int k = 0; k < 6; k++) {
        tw[k] = fresh ? nb[k] : 0.0;
        held[k] = fresh ? 0.0 : nb[k];
      }
      if (a.twist_bar) store_n(a.twist_bar, i, tw, nan);
      if (a.Vb_bar) store_n(a.Vb_bar, i, held, nan);
      if (a.Rwb_bar) store_n(a.Rwb_bar, i, Rbar, nan);
      if (a.x_bar) store_n(a.x_bar, i, xb, nan);
      if (a.Rwb_d_prev_bar) store_n(a.Rwb_d_prev_bar, i, G, nan);
      if (a.x_d_prev_bar) store_n(a.x_d_prev_bar, i, xa, nan);
      if (a.xdot_d_prev_bar) store_n(a.xdot_d_prev_bar, i, b, nan);
      if (a.w_d_prev_bar) store_n(a.w_d_prev_bar, i, c, nan);
      if (a.flags) a.flags[i] = fl;
    }
  }
}

}  // namespace qc
#endif  // __HIPCC__
