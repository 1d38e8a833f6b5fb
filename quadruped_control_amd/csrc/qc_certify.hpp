// qc_certify.hpp - the solver-independent KKT certificate of a solved batch, on the device: for every robot the gradient of the
// reference's objective at the forces qc_control_batch returned, the primal residual of the constraint rows, the Lagrange
// multipliers in closed form and the stationarity residual - what tests/kkt_batch.py computes on the host from a batch copied
// back, as one kernel next to the solve (qc_certify_batch, include/qc_balance.h), and a second, tiny kernel for the batch summary.
//
// Per robot, from the SAME qc_batch_in the solve read (conventions of qc_plant.hpp):
//   r_i, b         wrench_from_state on fetch_state's loads: r_i = Rwb p_i (p_i from `feet`, or from joint_q by leg_fk), b from the PD
//                  law, angle_axis_total and Iw - the solver's own functions, nothing restated
//   contact mask   load_contact_mask: `stance` bytes, else the phase rule on gait_phase AS IT IS NOW (gait_duty or the handle's
//                  value), else all stance.  gait_dt, swing_* and swing_state are ignored: no clock is advanced, `in` is never written.
//   f_i            = -Rwb grf_body_i (world frame, all four feet: a non-zero swing force enters A f and W f, as in kkt_batch.py)
//   grad           = 2 (A^T S (A f - b) + W f) with the handle's full 6x6 S and full 12x12 W whatever form the solver ran:
//                    u = (sum f_i, sum r_i x f_i) - b,  v = S u,  (A^T v)_i = v_lin + v_ang x r_i
//   primal         max over stance feet of |fx| - mu fz, |fy| - mu fz, fzmin - fz, fz - fzmax (swing feet count 0, as kkt_batch.py)
//   swing flag     any component of a swing foot's force != 0 (a NaN counts)
//   active rows    per stance foot and axis a code 0 none, 1 lower row, 2 upper row, 3 both:
//                    x: lower fx = -mu fz, upper fx = +mu fz, each when its slack <= act_tol (1 + mu |fz|); y alike;
//                    z: lower fz = fzmin when fz - fzmin <= act_tol (1 + fzmin), upper fz = fzmax when fzmax - fz <= act_tol (1 + fzmax)
//   multipliers    one row: lam_x = -s_x g_x, lam_y = -s_y g_y (s = -1 lower, +1 upper), lam_z = s_z (mu (lam_x + lam_y) - g_z);
//                  an axis with no row has lam = 0 and contributes |g| (z: |mu (lam_x + lam_y) - g_z|), one with a row max(0, -lam);
//                  BOTH rows (the apex fz = 0 = fzmin, or fzmin = fzmax): x, y: lam = |g|, carried by the row on the side -sign(g) - the
//                  pair of least sum, the choice that can satisfy the z row - contributing 0; z: the equality leaves lam_z free, it
//                  contributes 0 and lam_z holds the net value mu (lam_x + lam_y) - g_z (upper minus lower)
//   stationarity   the largest contribution over the stance feet / (1 + |grad|_2)
// Non-finite inputs propagate as NaN (max_nan below keeps a NaN where fmax would drop it); nothing is clamped.
// Commander mode is OUT OF SCOPE: its desired state lives in qc_commander_state, not in qc_batch_in, and this kernel reads Rwb_d,
// x_d, xdot_d, w_d.
//
// Kernel: one lane per robot, FP64, no LDS, no scratch, workgroups of one wave; a wave walks the batch with a grid stride once the
// grid is capped at CERTIFY_MAX_PARTIALS workgroups (above 262 144 robots).  Tail lanes recompute the last robot and store nothing.
// For the batch summary every workgroup reduces its robots with wave shuffles and leaves ONE partial in a handle-owned buffer with
// ordinary vector stores - no atomics; certify_summary_kernel, one workgroup, finishes them.  Maxima, minima and integer sums are
// exact, so the summary is deterministic and bit-equal to reducing the per-robot arrays.
#pragma once
#include "qc_device.hpp"

namespace qc {

// mirrors qc_certify_summary (include/qc_balance.h); also the layout of a workgroup's partial
struct CertifySummary {
  int64_t n_fail, n_nonfinite, n_swing_nonzero;
  double worst_primal, worst_stationarity;
  int64_t arg_primal, arg_stationarity;
};

// The kernel's argument struct (by value in the kernarg segment, next to the BatchIn the solve takes).
struct CertifyArgs {
  const double* grf_body;  // [n][4][3]
  double act_tol, primal_tol, stat_tol;
  double *primal, *stationarity, *lambda, *grad;  // optional OUT
  uint8_t* active;                                // optional OUT [n][4]
  int32_t* flags;                                 // optional OUT [n]
  CertifySummary* partials;                       // [gridDim.x] or nullptr (no summary asked for)
};

constexpr int CERTIFY_BLOCK = 64;            // one wave: the workgroup's reduction is a wave reduction
constexpr int CERTIFY_MAX_PARTIALS = 4096;   // grid cap = size of the handle's partial buffer
constexpr int CERTIFY_SUMMARY_BLOCK = 256;

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

QC_DEV double max_nan(double a, double b) { return (a > b || a != a) ? a : b; }  // the larger, a NaN if either is one (numpy's maximum)

// (value, index) of the worst finite value: the larger value, the lower index on a tie; index -1 = none yet (value -inf)
QC_DEV void worst_merge(double& v, int64_t& a, double v2, int64_t a2) {
  const bool take = a2 >= 0 && (a < 0 || v2 > v || (v2 == v && a2 < a));
  v = take ? v2 : v;
  a = take ? a2 : a;
}
QC_DEV void summary_merge(CertifySummary& s, const CertifySummary& o) {
  s.n_fail += o.n_fail;
  s.n_nonfinite += o.n_nonfinite;
  s.n_swing_nonzero += o.n_swing_nonzero;
  worst_merge(s.worst_primal, s.arg_primal, o.worst_primal, o.arg_primal);
  worst_merge(s.worst_stationarity, s.arg_stationarity, o.worst_stationarity, o.arg_stationarity);
}
// all 64 lanes of the wave take part; lane 0 ends with the wave's summary
QC_DEV void summary_wave_reduce(CertifySummary& s) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    CertifySummary o;
    o.n_fail = __shfl_xor((long long)s.n_fail, d);
    o.n_nonfinite = __shfl_xor((long long)s.n_nonfinite, d);
    o.n_swing_nonzero = __shfl_xor((long long)s.n_swing_nonzero, d);
    o.worst_primal = __shfl_xor(s.worst_primal, d);
    o.worst_stationarity = __shfl_xor(s.worst_stationarity, d);
    o.arg_primal = __shfl_xor((long long)s.arg_primal, d);
    o.arg_stationarity = __shfl_xor((long long)s.arg_stationarity, d);
    summary_merge(s, o);
  }
}
QC_DEV CertifySummary summary_empty() {
  return CertifySummary{0, 0, 0, -__builtin_huge_val(), -__builtin_huge_val(), -1, -1};
}

// One axis of the pyramid (x or y) at gradient g: the multiplier, what it adds to lam_x + lam_y, and the residual contribution.
QC_DEV void certify_xy(int code, double g, double& lam, double& res) {
  const double one = code == 1 ? g : -g;  // lower row (s = -1): lam = g; upper row: lam = -g
  lam = code == 0 ? 0.0 : (code == 3 ? fabs(g) : one);
  res = code == 0 ? fabs(g) : (code == 3 ? 0.0 : max_nan(0.0, -one));
}

// One stance foot's rows at the world-frame force (fx, fy, fz): the primal residual and the active codes of the three axes (0 none,
// 1 lower, 2 upper, 3 both) - shared with the sensitivity kernel (qc_sensitivity.hpp), whose face these codes define.
// No contraction here: the residual and the row tests are the expressions of tests/kkt_batch.py to the bit, so a force that sits
// exactly on a face (fx = mu fz as assigned) has slack exactly 0 and is classified the same everywhere.
QC_DEV void classify_foot(double mu, double fzmin, double fzmax, double act_tol, double fx, double fy, double fz, double& viol, int& cx,
                          int& cy, int& cz) {
#pragma clang fp contract(off)
  viol = max_nan(max_nan(fabs(fx) - mu * fz, fabs(fy) - mu * fz), max_nan(fzmin - fz, fz - fzmax));
  const double tol = act_tol * (1.0 + fabs(fz) * mu);
  cx = (mu * fz + fx <= tol ? 1 : 0) | (mu * fz - fx <= tol ? 2 : 0);
  cy = (mu * fz + fy <= tol ? 1 : 0) | (mu * fz - fy <= tol ? 2 : 0);
  cz = (fz - fzmin <= act_tol * (1.0 + fzmin) ? 1 : 0) | (fzmax - fz <= act_tol * (1.0 + fzmax) ? 2 : 0);
}

// The world-frame forces and the wrench residual of a robot: f_l = -Rwb grf_body_l, u = A f - b = (sum f_l, sum r_l x f_l) - b -
// shared with the sensitivity kernel.
QC_DEV void forces_and_residual(const double (&R)[9], const double (&gb)[4][3], const Wrench<4>& W, double (&f)[4][3], double (&u)[6]) {
#pragma unroll
  for (int k = 0; k < 6; k++) u[k] = 0.0;
#pragma unroll
  for (int l = 0; l < 4; l++) {
    double rg[3], m[3];
    mat_vec(R, gb[l], rg);
#pragma unroll
    for (int k = 0; k < 3; k++) f[l][k] = -rg[k];
    cross3(W.r[l], f[l], m);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      u[k] += f[l][k];
      u[3 + k] += m[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 6; k++) u[k] -= W.b[k];
}

template <bool KIN>
__global__ __launch_bounds__(CERTIFY_BLOCK) void certify_kernel(const DevParams* __restrict__ Pg, const long n, const BatchIn in, const CertifyArgs a) {
  CertifySummary acc = summary_empty();
  for (long base = (long)blockIdx.x * CERTIFY_BLOCK; base < n; base += (long)gridDim.x * CERTIFY_BLOCK) {
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

    // f_w,i = -Rwb grf_body_i;  u = A f - b
    double f[4][3], u[6];
    forces_and_residual(S.R, gb, W, f, u);
    // v = S u, grad = 2 (A^T v + W f)
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
    double g[4][3], g2 = 0.0;
    {
      const double vl[3] = {v[0], v[1], v[2]}, va[3] = {v[3], v[4], v[5]};
#pragma unroll
      for (int l = 0; l < 4; l++) {
        double c[3];
        cross3(va, W.r[l], c);
#pragma unroll
        for (int k = 0; k < 3; k++) {
          CParams& Pw = *QC_PARAMS_HERE(Pg);  // one row of W at a time: the scalar loads stay next to their use
          double wf = 0.0;
#pragma unroll
          for (int m = 0; m < 12; m++) wf += Pw.W[12 * (3 * l + k) + m] * f[m / 3][m % 3];
          g[l][k] = 2.0 * ((vl[k] + c[k]) + wf);
          g2 += g[l][k] * g[l][k];
        }
      }
    }
    const double gn = 1.0 + sqrt(g2);

    // per foot: primal residual, active rows, multipliers, stationarity contribution
    CParams& Pc = *QC_PARAMS_HERE(Pg);
    const double mu = Pc.mu, fzmin = Pc.fzmin, fzmax = Pc.fzmax;
    double primal = 0.0, res = 0.0, lam[4][3];
    uint32_t act = 0;
    bool swing_bad = false;
#pragma unroll
    for (int l = 0; l < 4; l++) {
      const double fx = f[l][0], fy = f[l][1], fz = f[l][2];
      if (mask & (1u << l)) {
        // (no contraction in the multipliers either: they were written under classify_foot's rule and stay as they were)
#pragma clang fp contract(off)
        double viol;
        int cx, cy, cz;
        classify_foot(mu, fzmin, fzmax, a.act_tol, fx, fy, fz, viol, cx, cy, cz);
        double rx, ry;
        certify_xy(cx, g[l][0], lam[l][0], rx);
        certify_xy(cy, g[l][1], lam[l][1], ry);
        const double ez = mu * (lam[l][0] + lam[l][1]) - g[l][2];
        lam[l][2] = cz == 0 ? 0.0 : (cz == 1 ? -ez : ez);
        const double rz = cz == 0 ? fabs(ez) : (cz == 3 ? 0.0 : max_nan(0.0, cz == 1 ? ez : -ez));
        primal = l == 0 ? viol : max_nan(primal, viol);
        res = max_nan(res, max_nan(max_nan(rx, ry), rz));
        act |= (uint32_t)(cx | (cy << 2) | (cz << 4)) << (8 * l);
      } else {
        swing_bad = swing_bad || fx != 0.0 || fy != 0.0 || fz != 0.0;
        lam[l][0] = lam[l][1] = lam[l][2] = 0.0;
        primal = l == 0 ? 0.0 : max_nan(primal, 0.0);
        act |= 0x80u << (8 * l);
      }
    }
    const double stat = res / gn;
    const bool fin_p = fabs(primal) < __builtin_huge_val(), fin_s = fabs(stat) < __builtin_huge_val();  // (false for a NaN)
    const int flags = (swing_bad ? 1 : 0) | ((!fin_p || !fin_s) ? 2 : 0);

    if (live) {
      if (a.primal) a.primal[i] = primal;
      if (a.stationarity) a.stationarity[i] = stat;
      if (a.lambda) {
#pragma unroll
        for (int l = 0; l < 4; l++) store3(a.lambda, 4 * i + l, lam[l]);
      }
      if (a.grad) {
#pragma unroll
        for (int l = 0; l < 4; l++) store3(a.grad, 4 * i + l, g[l]);
      }
      if (a.active) *reinterpret_cast<uint32_t*>(a.active + 4 * i) = act;
      if (a.flags) a.flags[i] = flags;
      if (a.partials) {
        CertifySummary one = summary_empty();
        one.n_fail = (!(primal <= a.primal_tol) || !(stat <= a.stat_tol) || swing_bad) ? 1 : 0;
        one.n_nonfinite = (flags & 2) ? 1 : 0;
        one.n_swing_nonzero = swing_bad ? 1 : 0;
        if (fin_p) { one.worst_primal = primal; one.arg_primal = i; }
        if (fin_s) { one.worst_stationarity = stat; one.arg_stationarity = i; }
        summary_merge(acc, one);
      }
    }
  }
  if (a.partials) {  // (uniform over the wave: every lane has left the loop)
    summary_wave_reduce(acc);
    if (threadIdx.x == 0) a.partials[blockIdx.x] = acc;
  }
}

// One workgroup finishes the partials.  No value finite: worst_* = NaN, arg_* = -1.
__global__ __launch_bounds__(CERTIFY_SUMMARY_BLOCK) void certify_summary_kernel(const CertifySummary* __restrict__ parts, const int nparts,
                                                                                CertifySummary* __restrict__ out) {
  __shared__ CertifySummary waves[CERTIFY_SUMMARY_BLOCK / 64];
  CertifySummary acc = summary_empty();
  for (int p = threadIdx.x; p < nparts; p += CERTIFY_SUMMARY_BLOCK) summary_merge(acc, parts[p]);
  summary_wave_reduce(acc);
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < CERTIFY_SUMMARY_BLOCK / 64; w++) summary_merge(acc, waves[w]);
    if (acc.arg_primal < 0) acc.worst_primal = __builtin_nan("");
    if (acc.arg_stationarity < 0) acc.worst_stationarity = __builtin_nan("");
    *out = acc;
  }
}

}  // namespace qc
#endif  // __HIPCC__
