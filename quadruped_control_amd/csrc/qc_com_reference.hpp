// qc_com_reference.hpp - the desired COM position of a step from the virtual support polygon (qc_com_reference_batch,
// include/qc_balance.h) and its reverse pass (qc_com_reference_adjoint_batch): what turns the polygon of qc_support_polygon.hpp into
// the x_d a tick tracks, so that a rollout leans over the feet that stay.
//
// FORWARD, per robot.  The polygon in world mode by its own device functions (support_load, support_point): P_l the x, y of
// Rwb p_l + x, v_l the four virtual points, com_xy = (((v_FL + v_FR) + v_RL) + v_RR) / 4 - the expression of support_polygon_kernel,
// so that com_xy equals qc_support_polygon_batch's bit for bit.  Then
//   QC_COM_REPLACE   x_d_out = (com_xy, x_d_in.z)                                             gain is not read
//   QC_COM_OFFSET    x_d_out = (x_d_in.xy + gain (com_xy - centroid_xy), x_d_in.z),   centroid_xy = (((P_FL + P_FR) + P_RL) + P_RR) / 4
// All weights 1 make every v_l = P_l: the offset is the lean alone.  z is copied.  A robot the polygon flags (a denominator zero or
// not finite, the reference's 0/0) gets NaN in x_d_out's x and y; com_xy is what the arithmetic gives, as the polygon kernel's.
//
// REVERSE.  Nothing is saved by the forward launch.  With o = x_d_out_bar and s = 1 (REPLACE) or gain (OFFSET):
//   x_d_in_bar = (0, 0, o.z) (REPLACE),  o (OFFSET)
//   g = s o.xy / 4 is the polygon's vb_l;  Pb_l starts at 0 (REPLACE) or at -g (OFFSET: the centroid's -gain o.xy / 4 on every P_l)
// and support_reverse (below: the polygon adjoint's own lines) carries on to feet_bar (body frame), Rwb_bar (entrywise), x_bar,
// phase_bar and the schedule_bar rows, on top of their `_in` rows.  gain gets no cotangent.  A flagged robot gets NaN in every output row, x_d_in_bar's
// included.
//
// schedule_bar_sum [16]: the schedule_bar rows AS STORED (the `_in` rows included, NaN for a flagged robot) summed over the batch in
// an order that is a function of n alone - no atomics, no shuffles.  With B = min(ceil(n / 64), COM_SUM_MAX_BLOCKS) workgroups of one
// wave, all sums starting from 0.0:
//   1. partial[b][e], b < B: for r = 0, 1, ... while (b + r B) 64 < n, for j = 0 .. 63 while i = (b + r B) 64 + j < n, in that order:
//      partial[b][e] += row[i][e]
//   2. group[w][e], w < 16: for p = w, w + 16, w + 32, ... < B, in rising order: group[w][e] += partial[p][e]
//   3. sum[e] = group[0][e]; for w = 1 .. 15: sum[e] += group[w][e]
// (tests/com_reference_restatement.py: ordered_sum repeats it in numpy.)  Step 1 is the reverse kernel's second instantiation: each
// lane leaves its 16 numbers in LDS at a stride of 17 doubles (odd: the lanes' writes of one slot fall on different banks), after the
// barrier lane e < 16 walks the wave's robots in index order into an accumulator that lives across the grid stride, and the
// workgroup leaves ONE partial in a handle-owned buffer with ordinary vector stores.  Steps 2 and 3 are com_schedule_sum_kernel, one
// workgroup of 256 threads: thread t holds e = t mod 16 of group t / 16.  Every partial the finisher reads was written by this
// launch.  Tail lanes leave a record nobody reads.  Because the buffer is the handle's, two calls that ask for the sum do not overlap
// on different streams (qc_sensitivity_param_batch's rule).
//
// Kernels: ONE LANE PER ROBOT, FP64, 0 B scratch, no atomics (profiles/com_reference_kernel_resources.txt); no LDS but for the
// summing instantiation's 8704 B.  Launch geometry, the "n beyond one launch" refusal and the tail lanes (the index clamped, nothing
// stored) are qc_support_polygon.hpp's; the summing instantiation caps its grid at COM_SUM_MAX_BLOCKS.  All read every input of a
// robot before they write any of its outputs, and a lane writes its own robot only: x_d_out may be x_d_in, x_d_in_bar may be
// x_d_out_bar, each `_in` array its output.
#pragma once
#include "qc_support_polygon.hpp"

namespace qc {

constexpr int COM_REPLACE = 0, COM_OFFSET = 1;  // QC_COM_REPLACE, QC_COM_OFFSET

struct ComReferenceArgs : SupportIn {  // (always world mode)
  const double* x_d_in;  // [n][3]
  int mode;
  double gain;
  double *x_d_out, *com_xy;  // [n][3], [n][2] optional
  int32_t* flags;            // [n] optional
};

// (flat, not on SupportIn: its `mode` sits in the padding behind `shared`, and a base struct's padding is not reused - the base would move
// every field behind it and with them the kernarg loads of both reverse kernels)
struct ComReferenceAdjointArgs {
  const double *feet, *joint_q, *gait_phase;
  const uint8_t* stance;
  const double* gait_duty;
  const double *Rwb, *x;
  const double* schedule;
  int shared;
  int mode;
  double gain;
  const double* x_d_out_bar;                                                            // [n][3]
  const double *feet_bar_in, *Rwb_bar_in, *x_bar_in, *phase_bar_in, *schedule_bar_in;   // optional
  double *x_d_in_bar, *feet_bar, *Rwb_bar, *x_bar, *phase_bar, *schedule_bar;           // optional OUT
  double* partials;                                                                     // [gridDim.x][16]: the summing instantiation
  int32_t* flags;                                                                       // [n] optional OUT
};

#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Winvalid-offsetof"  // (a struct with a base is not standard-layout; the compilers this builds with lay it out as C would)
static_assert(sizeof(ComReferenceArgs) == 120 && offsetof(ComReferenceArgs, x_d_in) == 72 && sizeof(ComReferenceAdjointArgs) == 192 &&
                  offsetof(ComReferenceAdjointArgs, mode) == 68,
              "SupportIn leads ComReferenceArgs; ComReferenceAdjointArgs keeps its nine fields and its layout");
#pragma GCC diagnostic pop

constexpr int COM_SUM_MAX_BLOCKS = 1024;  // grid cap of the summing instantiation = partials in the handle's buffer
constexpr int COM_SUM_STRIDE = 17;        // a lane's 16 numbers in LDS, at an odd stride
constexpr int COM_SUM_GROUPS = 16;        // the finisher: 16 groups of 16 threads
constexpr int COM_SUM_FINISH_BLOCK = 16 * COM_SUM_GROUPS;

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

__global__ __launch_bounds__(SENSITIVITY_BLOCK) void com_reference_kernel(const DevParams* __restrict__ Pg, const long n, const ComReferenceArgs a) {
  for (long base = (long)blockIdx.x * SENSITIVITY_BLOCK; base < n; base += (long)gridDim.x * SENSITIVITY_BLOCK) {
    const long me = base + threadIdx.x;
    const bool live = me < n;
    const long i = live ? me : n - 1;  // tail lanes: the last robot again, nothing stored
    CParams& P = *QC_PARAMS_HERE(Pg);
    // every input of the robot first: x_d_out may be x_d_in
    SupportRobot S;
    support_load(P, a, i, S);
    double xd[3];
    load3(a.x_d_in, i, xd);
    double v[4][2];
    int fl = 0;
#pragma unroll
    for (int l = 0; l < 4; l++) {
      double D, zm[2], zp[2];
      if (support_point(S, l, D, zm, zp, v[l])) fl |= 1 << l;
    }
    double com[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
      com[k] = (((v[SUPPORT_SUM_ORDER[0]][k] + v[SUPPORT_SUM_ORDER[1]][k]) + v[SUPPORT_SUM_ORDER[2]][k]) + v[SUPPORT_SUM_ORDER[3]][k]) / 4.0;
      double o = com[k];
      if (a.mode == COM_OFFSET) {
        const double cen = (((S.P[SUPPORT_SUM_ORDER[0]][k] + S.P[SUPPORT_SUM_ORDER[1]][k]) + S.P[SUPPORT_SUM_ORDER[2]][k]) + S.P[SUPPORT_SUM_ORDER[3]][k]) / 4.0;
        o = xd[k] + a.gain * (com[k] - cen);
      }
      xd[k] = fl ? __builtin_nan("") : o;
    }
    if (live) {
      store3(a.x_d_out, i, xd);
      if (a.com_xy) {
        a.com_xy[2 * i] = com[0];
        a.com_xy[2 * i + 1] = com[1];
      }
      if (a.flags) a.flags[i] = fl;
    }
  }
}

// The polygon's reverse pass of one robot from g = vb_l (a quarter of the cotangent on the mean of the four virtual points): the body
// of support_polygon_adjoint_kernel, line by line, REPEATED here and not shared - one body for both changed the registers or the
// instruction mix of one of the three kernels in each of the three variants tried (profiles/reference_fold.md) -, its world-mode
// branch alone.  Pb arrives holding what the centroid left there (zero in REPLACE mode) and the five accumulators their `_in` rows.
// Returns the forward rule's flags.
QC_DEV int support_reverse(const SupportRobot& S, const double (&g)[2], double (&Pb)[4][2], double (&fb)[12], double (&Rb)[9],
                           double (&xb)[3], double (&pb)[4], double (&sb)[16]) {
  double wb[4] = {0.0, 0.0, 0.0, 0.0};
  int fl = 0;
#pragma unroll
  for (int l = 0; l < 4; l++) {
    const int m = SUPPORT_MINUS[l], p = SUPPORT_PLUS[l];
    double D, zm[2], zp[2], v[2];
    if (support_point(S, l, D, zm, zp, v)) fl |= 1 << l;
    const double w = S.ramp[l].w, wm = S.ramp[m].w, wp = S.ramp[p].w;
    const double Nb[2] = {g[0] / D, g[1] / D};
    const double Db = -(g[0] * v[0] + g[1] * v[1]) / D;
    double dl = 0.0, dm = 0.0, dp = 0.0;
#pragma unroll
    for (int k = 0; k < 2; k++) {
      dl += Nb[k] * (S.P[l][k] + wm * (S.P[l][k] - S.P[m][k]) + wp * (S.P[l][k] - S.P[p][k]));
      dm += Nb[k] * zm[k];
      dp += Nb[k] * zp[k];
      Pb[l][k] += (w + w * wm + w * wp) * Nb[k];
      Pb[m][k] += wm * (1.0 - w) * Nb[k];
      Pb[p][k] += wp * (1.0 - w) * Nb[k];
    }
    wb[l] += Db + dl;
    wb[m] += Db + dm;
    wb[p] += Db + dp;
  }
#pragma unroll
  for (int l = 0; l < 4; l++) {
    const bool st = (S.stance >> l) & 1u;
    const SupportRamp& r = S.ramp[l];
    const double e1 = exp_neg_sq(r.a1) * SUPPORT_INV_SQRT_PI, e2 = exp_neg_sq(r.a2) * SUPPORT_INV_SQRT_PI;
    const double ph = wb[l] * (e1 / r.d1 - e2 / r.d2);
    pb[l] += st ? ph : -ph;
    const double b1 = -wb[l] * e1 * r.a1 * SUPPORT_ROOT2 / r.d1, b2 = -wb[l] * e2 * r.a2 * SUPPORT_ROOT2 / r.d2;
    sb[4 * l] += st ? b1 : 0.0;
    sb[4 * l + 1] += st ? b2 : 0.0;
    sb[4 * l + 2] += st ? 0.0 : b1;
    sb[4 * l + 3] += st ? 0.0 : b2;
    const double pw[3] = {Pb[l][0], Pb[l][1], 0.0};
    double ft[3];
    mat_t_vec(S.R, pw, ft);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      fb[3 * l + k] += ft[k];
      Rb[k] += pw[0] * S.pb[l][k];
      Rb[3 + k] += pw[1] * S.pb[l][k];
    }
    xb[0] += pw[0];
    xb[1] += pw[1];
  }
  return fl;
}

template <bool SUM>
__global__ __launch_bounds__(SENSITIVITY_BLOCK) void com_reference_adjoint_kernel(const DevParams* __restrict__ Pg, const long n,
                                                                                  const ComReferenceAdjointArgs a) {
  __shared__ double rec[SUM ? SENSITIVITY_BLOCK * COM_SUM_STRIDE : 1];
  const int lane = threadIdx.x;
  double acc = 0.0;  // lane e < 16: entry e of this workgroup's partial
  for (long base = (long)blockIdx.x * SENSITIVITY_BLOCK; base < n; base += (long)gridDim.x * SENSITIVITY_BLOCK) {
    const long me = base + lane;
    const bool live = me < n;
    const long i = live ? me : n - 1;  // tail lanes: the last robot again, nothing stored
    CParams& P = *QC_PARAMS_HERE(Pg);
    // every input of the robot first: an output may be one of these arrays
    SupportRobot S;
    support_load(P, a, i, S);
    double ob[3], fb[12], Rb[9], xb[3], pb[4], sb[16];
    load3(a.x_d_out_bar, i, ob);
    load_or_zero(a.feet_bar_in, i, fb);
    load_or_zero(a.Rwb_bar_in, i, Rb);
    load_or_zero(a.x_bar_in, i, xb);
    load_or_zero(a.phase_bar_in, i, pb);
    load_or_zero(a.schedule_bar_in, i, sb);
    const bool offset = a.mode == COM_OFFSET;
    const double g[2] = {(offset ? a.gain * ob[0] : ob[0]) / 4.0, (offset ? a.gain * ob[1] : ob[1]) / 4.0};  // the polygon's vb_l
    const double c[2] = {offset ? -g[0] : 0.0, offset ? -g[1] : 0.0};                                      // the centroid's share of every P_l
    double Pb[4][2] = {{c[0], c[1]}, {c[0], c[1]}, {c[0], c[1]}, {c[0], c[1]}};
    const int fl = support_reverse(S, g, Pb, fb, Rb, xb, pb, sb);
    const bool nan = fl != 0;  // no gradient: every row of the robot
    if (!offset) ob[0] = ob[1] = 0.0;
    if (live) {
      if (a.x_d_in_bar) store_n(a.x_d_in_bar, i, ob, nan);
      if (a.feet_bar) store_n(a.feet_bar, i, fb, nan);
      if (a.Rwb_bar) store_n(a.Rwb_bar, i, Rb, nan);
      if (a.x_bar) store_n(a.x_bar, i, xb, nan);
      if (a.phase_bar) store_n(a.phase_bar, i, pb, nan);
      if (a.schedule_bar) store_n(a.schedule_bar, i, sb, nan);
      if (a.flags) a.flags[i] = fl;
    }
    if constexpr (SUM) {
#pragma unroll
      for (int e = 0; e < 16; e++) rec[lane * COM_SUM_STRIDE + e] = nan ? __builtin_nan("") : sb[e];
      __syncthreads();
      // the wave's robots in index order (a tail lane's record is never read)
      const long rest = n - base;
      const int robots = rest < SENSITIVITY_BLOCK ? (int)rest : SENSITIVITY_BLOCK;
      if (lane < 16)
        for (int j = 0; j < robots; j++) acc += rec[j * COM_SUM_STRIDE + lane];
      __syncthreads();  // (the next round of the grid stride writes the records again)
    }
  }
  if constexpr (SUM) {
    if (lane < 16) a.partials[(long)blockIdx.x * 16 + lane] = acc;
  }
}

// One workgroup adds the partials: thread t = 16 w + e those with index w, w + 16, ... in rising order, then thread e < 16 the 16
// group sums in rising order.
__global__ __launch_bounds__(COM_SUM_FINISH_BLOCK) void com_schedule_sum_kernel(const double* __restrict__ parts, const int nparts,
                                                                                double* __restrict__ out) {
  __shared__ double groups[COM_SUM_FINISH_BLOCK];
  const int e = threadIdx.x & 15, w = threadIdx.x >> 4;
  double acc = 0.0;
  for (int p = w; p < nparts; p += COM_SUM_GROUPS) acc += parts[(long)p * 16 + e];
  groups[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < 16) {
    double s = groups[threadIdx.x];
#pragma unroll
    for (int k = 1; k < COM_SUM_GROUPS; k++) s += groups[16 * k + threadIdx.x];
    out[threadIdx.x] = s;
  }
}

}  // namespace qc
#endif  // __HIPCC__
