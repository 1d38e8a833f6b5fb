// qc_sensitivity_params.hpp - the cotangents of the handle's own parameters: the PD gains, the weights S and W, the friction
// coefficient, the force limits and the controller's mass and Ib (qc_sensitivity_param_batch, include/qc_balance.h).  A third kernel
// behind the adjoint: it reads the BatchIn the solve read, the forces, the cotangent on them and the adjoint z qc_sensitivity_batch
// wrote for that cotangent, and repeats no solve.  The handle holds ONE parameter set for the batch, so the natural output is the
// cotangent summed over the robots (param_bar); the per-robot rows (param_bar_rows) are there for whoever weighs robots differently.
//
// Layout: QC_PARAM_COUNT = 211 doubles in the order of the double members of qc_params - mu, mass, fzmin, fzmax, Ib[9], S[36], W[144],
// kff[6], kp_p[3], kd_p[3], kp_w[3], kd_w[3].  Matrices entrywise and row-major, the entries taken as independent (Rwb_bar's
// convention): S_bar and W_bar are the UNSYMMETRISED forms below, and only their pairing with a symmetric direction means something.
//
// On the active face f = Z y + f0 at fixed codes (qc_sensitivity.hpp), with the minimiser's Z^T g = 0 differentiated for a parameter
// theta that moves the face by dphi = dZ y + df0, the gradient by dg at fixed f and the columns by dZ:
//   df = dphi + Z dy,  Z^T H Z dy = -(Z^T H dphi + dZ^T g + Z^T dg),  so with z = Z lambda, lambda = (Z^T H Z)^-1 Z^T f_bar,
//   theta_bar = <rho, dphi/dtheta> - <z, dg/dtheta> - <(dZ/dtheta) lambda, g>,   rho = f_bar - H z = f_bar - 2 (A^T S A z + W z).
// With u = A f - b, v = S u, g = 2 (A^T v + W f), q = S A z, b_bar = 2 q:
//   S          g = 2 A^T S u:  S_bar = -2 (A z) u^T
//   W          g = ... + 2 W f:  W_bar = -2 z f^T
//   mass, kff, kp_p, kd_p, kp_w, kd_w   b_bar pulled back through wrench_from_state (qc_device.hpp) line by line:
//              a = kp_p o (x_d - x) + kd_p o (xdot_d - xdot) + (kff[0] xdot_d[0], kff[1] xdot_d[1], kff[2] mass 9.81),
//              b_lin = mass (a - (0, 0, 9.81)):  mass_bar = <b_bar_lin, a - (0, 0, 9.81)> + b_bar[2] mass (kff[2] 9.81), and with
//              ab = mass b_bar_lin:  kp_p_bar = ab o (x_d - x), kd_p_bar = ab o (xdot_d - xdot), kff_bar[0..2] = (ab[0] xdot_d[0],
//              ab[1] xdot_d[1], ab[2] mass 9.81);
//              b_ang = Iw al + w_d x (Iw w_d), al = kp_w o e + kd_w o (w_d - w) + (kff[3] w_d[0], kff[4] w_d[1] + kff[5] w_d[2], 0):
//              al_bar = Iw^T ba (ba = b_bar[3:6]), kp_w_bar = al_bar o e, kd_w_bar = al_bar o (w_d - w),
//              kff_bar[3..5] = (al_bar[0] w_d[0], al_bar[1] w_d[1], al_bar[1] w_d[2])   (kff[5] acts on al[1], as the library has it)
//   Ib         Iw = Rwb Ib Rwb^T, Iw_bar = ba al^T + (ba x w_d) w_d^T (the rotation kernel's):  Ib_bar = Rwb^T Iw_bar Rwb
//   mu         over the stance feet without a code 3, with sx, sy in {-1, 0, +1} from the x / y codes 1 / 2 / 0 (a tied or pinned
//              fx = sx mu fz): <rho_l, (sx f_lz, sy f_lz, 0)> - [fz free] z_lz (sx g_lx + sy g_ly)
//   fzmin      a foot with z code 1 sits at f0_l = (sx mu fzmin, sy mu fzmin, fzmin):  <rho_l, (sx mu, sy mu, 1)>
//   fzmax      the same for z code 2
// This is the gradient of the CONTROLLER's use of mass and Ib (the wrench law); a plant that integrates the same body is another
// function of them (qc_plant_adjoint.hpp produces no such cotangent).  A foot with a code 3 on any axis adds nothing to mu_bar,
// fzmin_bar, fzmax_bar (bit 0 of qc_sensitivity_batch's flags marks the robot as one-sided).  A failed robot (all forces zero: every
// stance foot flagged, z = 0) and an all-swing robot give a zero row.  A NaN adjoint (flags bit 1) gives a NaN row: z reaches every
// entry, the three face entries through an explicit 0 * sum(z).  Non-finite inputs propagate; nothing is clamped.
//
// Kernel: one lane per robot, FP64, workgroups of one wave, grid-stride beyond SENSITIVITY_PARAM_MAX_BLOCKS workgroups; tail lanes
// recompute the last robot and take no part in what follows.  Each lane leaves a RECORD of 68 doubles in LDS - the 31 entries that
// are scalars per robot, a 1, and the factors -2 A z, u, -2 z, f of the two outer products - and every one of the 211 entries is then
// one product record[ia] * record[ib] (ia, ib from the entry's index alone; a scalar times the 1).  After the wave's barrier lane e
// owns the entries e, e + 64, e + 128, e + 192: it walks the wave's robots in index order, forms each robot's entry - stored to
// param_bar_rows as 512-byte coalesced pieces - and adds it to its running sum.  The sum never crosses lanes: no shuffles, no
// atomics.  A workgroup leaves its 211 sums as ONE partial in a handle-owned buffer with ordinary vector stores;
// sensitivity_param_sum_kernel, one workgroup of 16 waves, adds the partials - wave w those with index = w mod 16, in rising order,
// then the 16 wave sums in rising order.  The order of the additions is a function of n alone: the sum is bit-reproducible, equal with
// and without the rows, and every partial the finisher reads was written by this launch.  0 B of scratch.
#pragma once
#include "qc_sensitivity_rot.hpp"

namespace qc {

constexpr int PARAM_COUNT = 211;  // QC_PARAM_COUNT

struct SensitivityParamArgs {
  const double *grf_body, *grf_bar, *adjoint;  // [n][4][3], [n][4][3], [n][12]: the adjoint as qc_sensitivity_batch wrote it
  double act_tol;
  double* rows;      // optional OUT [n][211]
  double* partials;  // [gridDim.x][211] or nullptr (no sum asked for)
};

constexpr int SENSITIVITY_PARAM_BLOCK = 64;          // one wave
constexpr int SENSITIVITY_PARAM_MAX_BLOCKS = 1024;   // grid cap = partials in the handle's buffer (four resident workgroups per CU x 256 CUs)
constexpr int SENSITIVITY_PARAM_SUM_BLOCK = 1024;    // the finisher: 16 waves, one slice of the partials each
constexpr int SENSITIVITY_PARAM_SUM_WAVES = SENSITIVITY_PARAM_SUM_BLOCK / 64;
// the record a lane leaves in LDS: [0..12] mu, mass, fzmin, fzmax, Ib; [13..30] kff, kp_p, kd_p, kp_w, kd_w; [31] 1; [32..37] -2 A z;
// [38..43] u; [44..55] -2 z; [56..67] f.  The stride is odd: the lanes' writes of one slot fall on different banks.
constexpr int PARAM_RECORD = 68, PARAM_RECORD_STRIDE = 69;
constexpr int PARAM_ENTRIES_PER_LANE = (PARAM_COUNT + 63) / 64;

// entry e of the layout = record[ia] * record[ib]
constexpr int param_factor_a(int e) { return e < 13 ? e : (e < 49 ? 32 + (e - 13) / 6 : (e < 193 ? 44 + (e - 49) / 12 : 13 + (e - 193))); }
constexpr int param_factor_b(int e) { return e < 13 ? 31 : (e < 49 ? 38 + (e - 13) % 6 : (e < 193 ? 56 + (e - 49) % 12 : 31)); }

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

// 2 (A^T s + W x)_l for the four feet: s a wrench-space vector (lin, ang), x a force vector - the gradient g at (v, f), H z at (q, z)
QC_DEV void hessian_like(const DevParams* Pg, const double (&s)[6], const Wrench<4>& Wr, const double (&x)[4][3], double (&o)[4][3]) {
  const double sl[3] = {s[0], s[1], s[2]}, sa[3] = {s[3], s[4], s[5]};
#pragma unroll
  for (int l = 0; l < 4; l++) {
    double c[3];
    cross3(sa, Wr.r[l], c);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      CParams& Pw = *QC_PARAMS_HERE(Pg);  // one row of W at a time: the scalar loads stay next to their use
      double wx = 0.0;
#pragma unroll
      for (int m = 0; m < 12; m++) wx += Pw.W[12 * (3 * l + k) + m] * x[m / 3][m % 3];
      o[l][k] = 2.0 * ((sl[k] + c[k]) + wx);
    }
  }
}

template <bool KIN>
__global__ __launch_bounds__(SENSITIVITY_PARAM_BLOCK) void sensitivity_param_kernel(const DevParams* __restrict__ Pg, const long n, const BatchIn in,
                                                                                    const SensitivityParamArgs a) {
  __shared__ double rec[SENSITIVITY_PARAM_BLOCK * PARAM_RECORD_STRIDE];
  const int lane = threadIdx.x;
  // this lane's entries and their factors
  int ia[PARAM_ENTRIES_PER_LANE], ib[PARAM_ENTRIES_PER_LANE];
  double acc[PARAM_ENTRIES_PER_LANE];
#pragma unroll
  for (int t = 0; t < PARAM_ENTRIES_PER_LANE; t++) {
    const int e = lane + 64 * t;
    ia[t] = param_factor_a(e < PARAM_COUNT ? e : 0);
    ib[t] = param_factor_b(e < PARAM_COUNT ? e : 0);
    acc[t] = 0.0;
  }
  for (long base = (long)blockIdx.x * SENSITIVITY_PARAM_BLOCK; base < n; base += (long)gridDim.x * SENSITIVITY_PARAM_BLOCK) {
    const long me = base + lane;
    const bool live = me < n;
    const long i = live ? me : n - 1;  // tail lanes: the last robot again; their records are never read
    CParams& P = *QC_PARAMS_HERE(Pg);
    RawState S;
    double fp[12], gb[4][3], gbar[4][3], z[4][3];
    fetch_state<4, KIN>(in, i, 0, S, fp);
#pragma unroll
    for (int l = 0; l < 4; l++) {
      load3(a.grf_body, 4 * i + l, gb[l]);
      load3(a.grf_bar, 4 * i + l, gbar[l]);
      load3(a.adjoint, 4 * i + l, z[l]);
    }
    const uint32_t mask = load_contact_mask(&P, in.stance, in.gait_phase, in.gait_duty, i, true);
    Wrench<4> W;
    (void)wrench_from_state<4, KIN>(P, S, fp, 0, W);
    const double (&R)[9] = S.R;
    const double (&wd)[3] = S.wd;

    // f_l = -Rwb grf_body_l, u = A f - b, f_bar_l = -Rwb grf_bar_l;  A z;  v = S u, q = S A z, b_bar = 2 q
    double f[4][3], fbar[4][3], u[6], az[6], v[6], q[6], bb[6];
    forces_and_residual(R, gb, W, f, u);
#pragma unroll
    for (int k = 0; k < 6; k++) az[k] = 0.0;
    double zsum = 0.0;
#pragma unroll
    for (int l = 0; l < 4; l++) {
      double rb[3], m[3];
      mat_vec(R, gbar[l], rb);
      cross3(W.r[l], z[l], m);
#pragma unroll
      for (int k = 0; k < 3; k++) {
        fbar[l][k] = -rb[k];
        az[k] += z[l][k];
        az[3 + k] += m[k];
        zsum += z[l][k];
      }
    }
    {
      CParams& Ps = *QC_PARAMS_HERE(Pg);
#pragma unroll
      for (int r = 0; r < 6; r++) {
        double sv = 0.0, sq = 0.0;
#pragma unroll
        for (int c = 0; c < 6; c++) {
          sv += Ps.S[6 * r + c] * u[c];
          sq += Ps.S[6 * r + c] * az[c];
        }
        v[r] = sv;
        q[r] = sq;
        bb[r] = 2.0 * sq;
      }
    }
    // g = 2 (A^T v + W f),  rho = f_bar - 2 (A^T q + W z)
    double g[4][3], rho[4][3];
    hessian_like(Pg, v, W, f, g);
    hessian_like(Pg, q, W, z, rho);
#pragma unroll
    for (int l = 0; l < 4; l++)
#pragma unroll
      for (int k = 0; k < 3; k++) rho[l][k] = fbar[l][k] - rho[l][k];

    // the face entries: mu, fzmin, fzmax (a NaN or infinite adjoint reaches them whatever the codes)
    const double poison = zsum * 0.0;
    double mub = poison, fminb = poison, fmaxb = poison;
    {
      CParams& Pc = *QC_PARAMS_HERE(Pg);
      const double mu = Pc.mu, fzmin = Pc.fzmin, fzmax = Pc.fzmax;
#pragma unroll
      for (int l = 0; l < 4; l++) {
        double viol;
        int cx, cy, cz;
        classify_foot(mu, fzmin, fzmax, a.act_tol, f[l][0], f[l][1], f[l][2], viol, cx, cy, cz);
        const bool moves = (mask & (1u << l)) != 0 && !(cx == 3 || cy == 3 || cz == 3);
        const double sx = cx == 1 ? -1.0 : (cx == 2 ? 1.0 : 0.0), sy = cy == 1 ? -1.0 : (cy == 2 ? 1.0 : 0.0);
        const double tie = sx * rho[l][0] + sy * rho[l][1];   // <rho_l, (sx, sy, 0)>
        const double col = cz == 0 ? z[l][2] * (sx * g[l][0] + sy * g[l][1]) : 0.0;
        const double lim = mu * tie + rho[l][2];              // <rho_l, (sx mu, sy mu, 1)>
        mub += moves ? tie * f[l][2] - col : 0.0;
        fminb += (moves && cz == 1) ? lim : 0.0;
        fmaxb += (moves && cz == 2) ? lim : 0.0;
      }
    }

    // b_bar through the PD law: the linear half
    CParams& Pb = *QC_PARAMS_HERE(Pg);
    const double mass = Pb.mass;
    double dx[3], dv[3], acc_lin[3], ab[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      dx[k] = S.xd[k] - S.x[k];
      dv[k] = S.xdotd[k] - S.xdot[k];
      acc_lin[k] = Pb.kp_p[k] * dx[k] + Pb.kd_p[k] * dv[k];
      ab[k] = mass * bb[k];
    }
    acc_lin[0] += Pb.kff[0] * S.xdotd[0];
    acc_lin[1] += Pb.kff[1] * S.xdotd[1];
    acc_lin[2] += Pb.kff[2] * mass * 9.81;
    const double mg = mass * 9.81;
    const double massb = (bb[0] * acc_lin[0] + bb[1] * acc_lin[1]) + (bb[2] * (acc_lin[2] - 9.81) + ab[2] * (Pb.kff[2] * 9.81));

    // ... and the angular half: the rotation error er and al as wrench_from_state forms them; al_bar = Iw^T ba; Ib_bar = (R^T ba)(R^T al)^T + (R^T (ba x wd))(R^T wd)^T
    double Re[9], er[3], al[3], dw[3];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) Re[3 * r + c] = S.Rd[3 * r] * R[3 * c] + S.Rd[3 * r + 1] * R[3 * c + 1] + S.Rd[3 * r + 2] * R[3 * c + 2];
    angle_axis_total(Re, er);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      dw[k] = wd[k] - S.w[k];
      al[k] = Pb.kp_w[k] * er[k] + Pb.kd_w[k] * dw[k];
    }
    al[0] += Pb.kff[3] * wd[0];
    al[1] += Pb.kff[4] * wd[1];
    al[1] += Pb.kff[5] * wd[2];  // sic (index 1), as wrench_from_state
    const double ba[3] = {bb[3], bb[4], bb[5]};
    double bxw[3], t1[3], t2[3], t3[3], t4[3], v1[3], alb[3];
    cross3(ba, wd, bxw);
    mat_t_vec(R, al, t1);
    mat_t_vec(R, wd, t2);
    mat_t_vec(R, ba, t3);
    mat_t_vec(R, bxw, t4);
    mat_t_vec(Pb.Ib, t3, v1);
    mat_vec(R, v1, alb);

    // the record
    double* mine = rec + lane * PARAM_RECORD_STRIDE;
    mine[0] = mub;
    mine[1] = massb;
    mine[2] = fminb;
    mine[3] = fmaxb;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) mine[4 + 3 * r + c] = t3[r] * t1[c] + t4[r] * t2[c];
    mine[13] = ab[0] * S.xdotd[0];
    mine[14] = ab[1] * S.xdotd[1];
    mine[15] = ab[2] * mg;
    mine[16] = alb[0] * wd[0];
    mine[17] = alb[1] * wd[1];
    mine[18] = alb[1] * wd[2];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      mine[19 + k] = ab[k] * dx[k];
      mine[22 + k] = ab[k] * dv[k];
      mine[25 + k] = alb[k] * er[k];
      mine[28 + k] = alb[k] * dw[k];
    }
    mine[31] = 1.0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
      mine[32 + k] = -2.0 * az[k];
      mine[38 + k] = u[k];
    }
#pragma unroll
    for (int l = 0; l < 4; l++)
#pragma unroll
      for (int k = 0; k < 3; k++) {
        mine[44 + 3 * l + k] = -2.0 * z[l][k];
        mine[56 + 3 * l + k] = f[l][k];
      }
    __syncthreads();

    // the wave's robots in index order: lane e forms its entries of each robot's row, stores them and adds them up
    const long rest = n - base;
    const int robots = rest < SENSITIVITY_PARAM_BLOCK ? (int)rest : SENSITIVITY_PARAM_BLOCK;
    for (int j = 0; j < robots; j++) {
      const double* r = rec + j * PARAM_RECORD_STRIDE;
#pragma unroll
      for (int t = 0; t < PARAM_ENTRIES_PER_LANE; t++) {
        const int e = lane + 64 * t;
        if (e < PARAM_COUNT) {
          const double p = r[ia[t]] * r[ib[t]];
          if (a.rows) a.rows[(base + j) * PARAM_COUNT + e] = p;
          acc[t] += p;
        }
      }
    }
    __syncthreads();  // (the next round of the grid stride writes the records again)
  }
  if (a.partials) {
#pragma unroll
    for (int t = 0; t < PARAM_ENTRIES_PER_LANE; t++) {
      const int e = lane + 64 * t;
      if (e < PARAM_COUNT) a.partials[(long)blockIdx.x * PARAM_COUNT + e] = acc[t];
    }
  }
}

// One workgroup adds the partials: wave w those with index w, w + 16, ... in rising order, then thread e < 211 the 16 wave sums.
__global__ __launch_bounds__(SENSITIVITY_PARAM_SUM_BLOCK) void sensitivity_param_sum_kernel(const double* __restrict__ parts, const int nparts,
                                                                                            double* __restrict__ out) {
  __shared__ double waves[SENSITIVITY_PARAM_SUM_WAVES * PARAM_COUNT];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double acc[PARAM_ENTRIES_PER_LANE];
#pragma unroll
  for (int t = 0; t < PARAM_ENTRIES_PER_LANE; t++) acc[t] = 0.0;
  for (int p = w; p < nparts; p += SENSITIVITY_PARAM_SUM_WAVES) {
#pragma unroll
    for (int t = 0; t < PARAM_ENTRIES_PER_LANE; t++) {
      const int e = lane + 64 * t;
      if (e < PARAM_COUNT) acc[t] += parts[(long)p * PARAM_COUNT + e];
    }
  }
#pragma unroll
  for (int t = 0; t < PARAM_ENTRIES_PER_LANE; t++) {
    const int e = lane + 64 * t;
    if (e < PARAM_COUNT) waves[w * PARAM_COUNT + e] = acc[t];
  }
  __syncthreads();
  if (threadIdx.x < PARAM_COUNT) {
    double s = waves[threadIdx.x];
#pragma unroll
    for (int k = 1; k < SENSITIVITY_PARAM_SUM_WAVES; k++) s += waves[k * PARAM_COUNT + threadIdx.x];
    out[threadIdx.x] = s;
  }
}

}  // namespace qc
#endif  // __HIPCC__
