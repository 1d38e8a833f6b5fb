// qc_support_polygon.hpp - the virtual support polygon of the reference (SupportPolygon::position, trajectory.cpp:73-147) as a launch
// of its own (qc_support_polygon_batch, include/qc_balance.h) and its reverse pass (qc_support_polygon_adjoint_batch): from the
// scheduled gait, the x, y position at which the COM should be held.
//
// FORWARD, per robot, the reference in its evaluation order.  Legs RL, FL, RR, FR = 0, 1, 2, 3; leg l has a clockwise neighbour
// m = SUPPORT_MINUS[l] and a counter-clockwise one p = SUPPORT_PLUS[l] (trajectory.cpp:75-78).  With phi_l the RAW gait phase of the
// leg (gait_map.second - not a sub-phase of the stance or the swing), the leg's four widths (c0, cf, s0, sf) = LegScheduledPhases'
// (stance_start, stance_end, swing_start, swing_end) - the sigma of the ramps, whatever their names say - and root2 = sqrt(2):
//   stance leg  a1 = phi / (c0 root2 + 1e-12),   a2 = (1 - phi) / (cf root2 + 1e-12),  w_l = 0.5 (erf a1 + erf a2)             (:102-103)
//   swing leg   a1 = -phi / (s0 root2 + 1e-12),  a2 = (phi - 1) / (sf root2 + 1e-12),  w_l = 0.5 ((2 + erf a1) + erf a2)       (:111-112)
//   P_l = the foot's x, y: body frame, or - `world` - of Rwb p_l + x
//   zm_l = P_l w_l + P_m (1 - w_l),  zp_l = P_l w_l + P_p (1 - w_l),  D_l = (w_l + w_m) + w_p
//   v_l = (1 / D_l) ((w_l P_l + w_m zm_l) + w_p zp_l)                                                                          (:131-138)
//   com_xy = (((v_FL + v_FR) + v_RL) + v_RR) / 4         the order of the reference's std::map
// The stance / swing decision is the contact mask every entry point resolves: `stance` bytes, else the phase rule.  erf is erf_f64.
// `flags` bit l: D_l is zero or not finite - the reference's 0/0; the arithmetic is reproduced (com_xy comes out NaN), nothing is
// clamped.
//
// REVERSE.  Nothing is saved by the forward launch: the same inputs are read and the forward quantities recomputed.  A cotangent of v
// is vb; g = com_xy_bar.  Per leg l, in the order 0, 1, 2, 3, with m, p its neighbours:
//   vb_l = g / 4,  Nb = vb_l / D_l,  Db = -<vb_l, v_l> / D_l
//   wb_l += Db + <Nb, P_l> + w_m <Nb, P_l - P_m> + w_p <Nb, P_l - P_p>,  wb_m += Db + <Nb, zm_l>,  wb_p += Db + <Nb, zp_l>
//   Pb_l += (w_l + w_l w_m + w_l w_p) Nb,  Pb_m += w_m (1 - w_l) Nb,  Pb_p += w_p (1 - w_l) Nb
// then, per leg, with e_i = exp_neg_sq(a_i) / sqrt(pi) (the derivative of 0.5 erf), d_i the two denominators above, sgn = +1 for a
// stance leg and -1 for a swing leg:
//   phase_bar_l = wb_l sgn (e1 / d1 - e2 / d2)
//   width_bar   = -wb_l e_i a_i root2 / d_i     on (c0, cf) of a stance leg, on (s0, sf) of a swing leg; the other two get 0
//   body mode   feet_bar_l = (Pb_l, 0)
//   world mode  feet_bar_l = Rwb^T (Pb_l, 0),  Rwb_bar += (Pb_l, 0) p_l^T (entrywise, row-major),  x_bar += (Pb_l, 0)
// The `_in` arrays are added in; each may be its output.  The contact mask is HELD: a phase exactly on the stance / swing boundary
// gets the gradient of the branch the forward pass took.  With a shared schedule, schedule_bar is still one [4][4] block per robot
// (not summed over the batch).  A robot flagged by the forward rule gets NaN in every output row.
//
// Kernels: ONE LANE PER ROBOT, FP64, no LDS, no atomics, 0 B scratch (profiles/support_polygon_kernel_resources.txt); the four legs
// are unrolled so that every per-leg array is indexed by constants.  Launch geometry, the "n beyond one launch" refusal and the tail
// lanes (the index clamped, nothing stored) are qc_swing_reference.hpp's.  Both read every input of a robot before they write any of
// its outputs, and a lane writes its own robot only: an output may be the same array as its `_in` input.
#pragma once
#include <cstddef>

#include "qc_swing_reference.hpp"

namespace qc {

// adjacent_leg_map_ (trajectory.cpp:75-78) on the legs RL, FL, RR, FR = 0, 1, 2, 3: (first, second) = (clockwise, counter-clockwise)
constexpr int SUPPORT_MINUS[4] = {1, 3, 0, 2};  // RL: FL, FL: FR, RR: RL, FR: RR
constexpr int SUPPORT_PLUS[4] = {2, 0, 3, 1};   // RL: RR, FL: RL, RR: FR, FR: FL
// the order in which the reference's std::map<std::string, ...> visits the legs: "FL" < "FR" < "RL" < "RR"
constexpr int SUPPORT_SUM_ORDER[4] = {1, 3, 0, 2};

// what the polygon and COM kernels read of a robot: the base of their four argument structs (as BodyConst is of the plant's)
struct SupportIn {
  const double *feet, *joint_q;  // [n][4][3]: joint_q if given, else feet
  const double* gait_phase;      // [n][4]
  const uint8_t* stance;         // [n][4] or NULL: the phase rule
  const double* gait_duty;       // [n] or NULL
  const double *Rwb, *x;         // [n][9], [n][3]: world mode, else NULL
  const double* schedule;        // [n][4][4], or [4][4] if shared
  int shared;
};

struct SupportPolygonArgs : SupportIn {
  double *com_xy, *weights;      // [n][2], [n][4] optional OUT
  int32_t* flags;                // [n] optional OUT
};

struct SupportPolygonAdjointArgs : SupportIn {
  const double* com_xy_bar;                                                               // [n][2]
  const double *feet_bar_in, *Rwb_bar_in, *x_bar_in, *phase_bar_in, *schedule_bar_in;     // optional
  double *feet_bar, *Rwb_bar, *x_bar, *phase_bar, *schedule_bar;                          // optional OUT
  int32_t* flags;                                                                         // [n] optional OUT
};

// (a derived struct's own fields start behind the base's padded size: the layout is the one the flat structs had)
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Winvalid-offsetof"  // (a struct with a base is not standard-layout; the compilers this builds with lay it out as C would)
static_assert(sizeof(SupportIn) == 72 && sizeof(SupportPolygonArgs) == 96 && offsetof(SupportPolygonArgs, com_xy) == 72 &&
                  sizeof(SupportPolygonAdjointArgs) == 168 && offsetof(SupportPolygonAdjointArgs, com_xy_bar) == 72,
              "SupportIn leads the polygon's argument structs");
#pragma GCC diagnostic pop

}  // namespace qc

#ifdef __HIPCC__
namespace qc {

constexpr double SUPPORT_ROOT2 = 1.4142135623730951;        // std::sqrt(2.0)
constexpr double SUPPORT_INV_SQRT_PI = 0.5641895835477563;  // 1 / sqrt(pi)

// one leg's ramp: the two erf arguments, their denominators and the weight
struct SupportRamp {
  double a1, a2, d1, d2, w;
};
QC_DEV SupportRamp support_ramp(bool st, double ph, const double (&c)[4]) {
  SupportRamp r;
  r.d1 = (st ? c[0] : c[2]) * SUPPORT_ROOT2 + 1.0e-12;  // add epsilon to prevent division by 0
  r.d2 = (st ? c[1] : c[3]) * SUPPORT_ROOT2 + 1.0e-12;
  r.a1 = (st ? ph : -ph) / r.d1;
  r.a2 = (st ? 1.0 - ph : ph - 1.0) / r.d2;
  const double e1 = erf_f64(r.a1), e2 = erf_f64(r.a2);
  r.w = st ? 0.5 * (e1 + e2) : 0.5 * ((2.0 + e1) + e2);
  return r;
}

// what both kernels read of a robot and make of it: the four points, the ramps, the body-frame feet (world mode and the reverse pass)
struct SupportRobot {
  double P[4][2], pb[4][3], R[9];
  SupportRamp ramp[4];
  uint32_t stance;
};
template <class Args>
QC_DEV void support_load(CParams& P, const Args& a, long i, SupportRobot& S) {
  const bool world = a.Rwb != nullptr;
  double x[3] = {0.0, 0.0, 0.0}, ph[4];
  if (world) {
    load9(a.Rwb, i, S.R);
    load3(a.x, i, x);
  }
#pragma unroll
  for (int l = 0; l < 4; l++) ph[l] = a.gait_phase[4 * i + l];
  const uint32_t sw = a.stance ? *reinterpret_cast<const uint32_t*>(a.stance + 4 * i) : 0u;
  const double duty = a.gait_duty ? a.gait_duty[i] : P.stance_phase;
  S.stance = contact_mask(a.stance != nullptr, sw, true, ph, duty, true);
  const double* sched = a.schedule + (a.shared ? 0 : 16 * i);
#pragma unroll
  for (int l = 0; l < 4; l++) {
    if (a.joint_q) {
      const double ql[3] = {a.joint_q[12 * i + 3 * l], a.joint_q[12 * i + 3 * l + 1], a.joint_q[12 * i + 3 * l + 2]};
      leg_fk(P, l, leg_trig(ql), S.pb[l]);
    } else {
      S.pb[l][0] = a.feet[12 * i + 3 * l];
      S.pb[l][1] = a.feet[12 * i + 3 * l + 1];
      S.pb[l][2] = world ? a.feet[12 * i + 3 * l + 2] : 0.0;  // (the body-frame polygon reads x and y only)
    }
    if (world) {
      double r[3];
      mat_vec(S.R, S.pb[l], r);
      S.P[l][0] = r[0] + x[0];
      S.P[l][1] = r[1] + x[1];
    } else {
      S.P[l][0] = S.pb[l][0];
      S.P[l][1] = S.pb[l][1];
    }
    const double c[4] = {sched[4 * l], sched[4 * l + 1], sched[4 * l + 2], sched[4 * l + 3]};
    S.ramp[l] = support_ramp((S.stance >> l) & 1u, ph[l], c);
  }
}

// the virtual point of leg l (trajectory.cpp:125-138) and whether its denominator is the reference's 0/0
QC_DEV bool support_point(const SupportRobot& S, int l, double& D, double (&zm)[2], double (&zp)[2], double (&v)[2]) {
  const int m = SUPPORT_MINUS[l], p = SUPPORT_PLUS[l];
  const double w = S.ramp[l].w, wm = S.ramp[m].w, wp = S.ramp[p].w;
  D = (w + wm) + wp;
  const double inv = 1.0 / D;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    zm[k] = S.P[l][k] * w + S.P[m][k] * (1.0 - w);
    zp[k] = S.P[l][k] * w + S.P[p][k] * (1.0 - w);
    v[k] = inv * ((w * S.P[l][k] + wm * zm[k]) + wp * zp[k]);
  }
  return !(D != 0.0 && fabs(D) < __builtin_inf());
}

__global__ __launch_bounds__(SENSITIVITY_BLOCK) void support_polygon_kernel(const DevParams* __restrict__ Pg, const long n, const SupportPolygonArgs a) {
  for (long base = (long)blockIdx.x * SENSITIVITY_BLOCK; base < n; base += (long)gridDim.x * SENSITIVITY_BLOCK) {
    const long me = base + threadIdx.x;
    const bool live = me < n;
    const long i = live ? me : n - 1;  // tail lanes: the last robot again, nothing stored
    CParams& P = *QC_PARAMS_HERE(Pg);
    SupportRobot S;
    support_load(P, a, i, S);
    double v[4][2];
    int fl = 0;
#pragma unroll
    for (int l = 0; l < 4; l++) {
      double D, zm[2], zp[2];
      if (support_point(S, l, D, zm, zp, v[l])) fl |= 1 << l;
    }
    if (live) {
      if (a.com_xy) {
#pragma unroll
        for (int k = 0; k < 2; k++)
          a.com_xy[2 * i + k] = (((v[SUPPORT_SUM_ORDER[0]][k] + v[SUPPORT_SUM_ORDER[1]][k]) + v[SUPPORT_SUM_ORDER[2]][k]) + v[SUPPORT_SUM_ORDER[3]][k]) / 4.0;
      }
      if (a.weights) {
#pragma unroll
        for (int l = 0; l < 4; l++) a.weights[4 * i + l] = S.ramp[l].w;
      }
      if (a.flags) a.flags[i] = fl;
    }
  }
}

__global__ __launch_bounds__(SENSITIVITY_BLOCK) void support_polygon_adjoint_kernel(const DevParams* __restrict__ Pg, const long n,
                                                                                    const SupportPolygonAdjointArgs a) {
  for (long base = (long)blockIdx.x * SENSITIVITY_BLOCK; base < n; base += (long)gridDim.x * SENSITIVITY_BLOCK) {
    const long me = base + threadIdx.x;
    const bool live = me < n;
    const long i = live ? me : n - 1;  // tail lanes: the last robot again, nothing stored
    CParams& P = *QC_PARAMS_HERE(Pg);
    const bool world = a.Rwb != nullptr;
    // every input of the robot first: an output may be one of these arrays
    SupportRobot S;
    support_load(P, a, i, S);
    double fb[12], Rb[9], xb[3], pb[4], sb[16];
    load_or_zero(a.feet_bar_in, i, fb);
    load_or_zero(a.Rwb_bar_in, i, Rb);
    load_or_zero(a.x_bar_in, i, xb);
    load_or_zero(a.phase_bar_in, i, pb);
    load_or_zero(a.schedule_bar_in, i, sb);
    const double g[2] = {a.com_xy_bar[2 * i] / 4.0, a.com_xy_bar[2 * i + 1] / 4.0};  // vb_l, the same for every leg
    double wb[4] = {0.0, 0.0, 0.0, 0.0}, Pb[4][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
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
      if (world) {
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
      } else {
        fb[3 * l] += pw[0];
        fb[3 * l + 1] += pw[1];
      }
    }
    if (live) {
      const bool nan = fl != 0;  // no gradient: every row of the robot
      if (a.feet_bar) store_n(a.feet_bar, i, fb, nan);
      if (a.Rwb_bar) store_n(a.Rwb_bar, i, Rb, nan);
      if (a.x_bar) store_n(a.x_bar, i, xb, nan);
      if (a.phase_bar) store_n(a.phase_bar, i, pb, nan);
      if (a.schedule_bar) store_n(a.schedule_bar, i, sb, nan);
      if (a.flags) a.flags[i] = fl;
    }
  }
}

}  // namespace qc
#endif  // __HIPCC__
