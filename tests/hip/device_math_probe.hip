// Device-math probe (test infrastructure, not the product): one primitive of quadruped_control_amd/csrc/qc_device.hpp per
// thread over arrays, so tests/test_gpu_device_math.py can hold each hand-written primitive against a high-precision
// reference.  The wrappers call the header's functions as they are; nothing here restates them.  The working-set recalculations
// (EqpDiagW, EqpDense, EqpDense4: one robot per lane group, whole waves) and clamp_foot / the foot code are probed the same way for
// tests/test_gpu_eqp.py.
//
// Every launcher takes device pointers (torch tensors), n and a stream and returns the hipError_t of its launch.  No
// allocation and no copies: the constants the kinematic primitives read live in a __device__ DevParams that
// qcp_set_params fills by a one-block kernel (qcp_set_qp_params: from the product's own derive_params), and the kernels read it
// through QC_PARAMS_HERE as the product does.
// Built by __graft_entry__.build_device_probe() with the product's own HIP_FLAGS (contraction and inlining as in the library).
#include "../../quadruped_control_amd/csrc/qc_device.hpp"
#include "../../quadruped_control_amd/csrc/qc_host.hpp"  // derive_params: the product's own derivation of the QP constants

#include <cstring>

using namespace qc;

namespace {

constexpr int kBlock = 64;
__device__ DevParams g_params;

inline dim3 grid_for(int n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }
__device__ __forceinline__ int tid() { return (int)(blockIdx.x * blockDim.x + threadIdx.x); }
__device__ __forceinline__ CParams& params() { return *QC_PARAMS_HERE(&g_params); }

__global__ void k_set_params(DevParams p) {
  const double* src = reinterpret_cast<const double*>(&p);
  double* dst = reinterpret_cast<double*>(&g_params);
  constexpr int nd = (int)(sizeof(DevParams) / sizeof(double));
  static_assert(sizeof(DevParams) % sizeof(double) == 0, "DevParams is a whole number of doubles");
  for (int i = threadIdx.x; i < nd; i += blockDim.x) dst[i] = src[i];
}

__global__ void k_sincos(const double* x, double* s, double* c, int n) {
  const int i = tid();
  if (i < n) sincos_joint(x[i], &s[i], &c[i]);
}
__global__ void k_rsqrt_rcp(const double* x, double* rs, double* rc, int n) {
  const int i = tid();
  if (i < n) { rs[i] = rsqrt_nr(x[i]); rc[i] = rcp_nr(x[i]); }
}
__global__ void k_angle_axis(const double* m, double* out, int n) {
  const int i = tid();
  if (i >= n) return;
  double a[9], o[3];
  for (int k = 0; k < 9; k++) a[k] = m[9 * i + k];
  angle_axis_total(a, o);
  for (int k = 0; k < 3; k++) out[3 * i + k] = o[k];
}
// out[4 i ..]: wrap_2PI, wrap_PI, normalize_angle_2PI, normalize_angle_PI
__global__ void k_wraps(const double* x, double* out, int n) {
  const int i = tid();
  if (i >= n) return;
  out[4 * i] = wrap_2PI(x[i]);
  out[4 * i + 1] = wrap_PI(x[i]);
  out[4 * i + 2] = normalize_angle_2PI(x[i]);
  out[4 * i + 3] = normalize_angle_PI(x[i]);
}
// trig[6 i ..]: s1 c1 s2 c2 s23 c23; p = FK; tau = J^T f through both leg_jt_force overloads
__global__ void k_leg(const int* leg, const double* q, const double* f, double* trig, double* p, double* tau_c, double* tau_g, int n) {
  const int i = tid();
  if (i >= n) return;
  const int l = leg[i];
  if (l < 0 || l > 3) return;
  const LegTrig t = leg_trig(q + 3 * i);
  trig[6 * i] = t.s1; trig[6 * i + 1] = t.c1; trig[6 * i + 2] = t.s2; trig[6 * i + 3] = t.c2; trig[6 * i + 4] = t.s23; trig[6 * i + 5] = t.c23;
  double pp[3], ff[3] = {f[3 * i], f[3 * i + 1], f[3 * i + 2]}, tc[3], tg[3];
  leg_fk(params(), l, t, pp);
  leg_jt_force(params(), l, t, ff, tc);
  leg_jt_force(leg_geom(params(), l), t, ff, tg);
  for (int k = 0; k < 3; k++) { p[3 * i + k] = pp[k]; tau_c[3 * i + k] = tc[k]; tau_g[3 * i + k] = tg[k]; }
}
__global__ void k_pinv3(const double* J, const double* v, double* x, int n) {
  const int i = tid();
  if (i >= n) return;
  double a[9], b[3] = {v[3 * i], v[3 * i + 1], v[3 * i + 2]}, o[3];
  for (int k = 0; k < 9; k++) a[k] = J[9 * i + k];
  pinv3_apply(a, b, o);
  for (int k = 0; k < 3; k++) x[3 * i + k] = o[k];
}
__global__ void k_swing_torque(const int* leg, const double* pb, const double* vb, const double* q, const double* qdot, double* tau, int n) {
  const int i = tid();
  if (i >= n) return;
  const int l = leg[i];
  if (l < 0 || l > 3) return;
  const double p[3] = {pb[3 * i], pb[3 * i + 1], pb[3 * i + 2]}, v[3] = {vb[3 * i], vb[3 * i + 1], vb[3 * i + 2]};
  double t[3];
  leg_swing_torque(params(), leg_geom(params(), l), p, v, q + 3 * i, qdot + 3 * i, t);
  for (int k = 0; k < 3; k++) tau[3 * i + k] = t[k];
}
// swing_pd<true> and <false> at the reference angles qr (J from leg_trig(qr)), vb = 0, qdot = 0: with kp = 1, kd = kff = 0 in
// the constants the torques are the wrapped PD errors e of the two forms
__global__ void k_swing_pd(const int* leg, const double* qr, const double* q, double* tau_fast, double* tau_ref, int n) {
  const int i = tid();
  if (i >= n) return;
  const int l = leg[i];
  if (l < 0 || l > 3) return;
  const double r[3] = {qr[3 * i], qr[3 * i + 1], qr[3 * i + 2]}, vb[3] = {0.0, 0.0, 0.0}, qd[3] = {0.0, 0.0, 0.0};
  const LegGeom g = leg_geom(params(), l);
  const LegTrig t = leg_trig(r);
  double tf[3], tr[3];
  swing_pd<true>(params(), g, t, r, vb, q + 3 * i, qd, tf);
  swing_pd<false>(params(), g, t, r, vb, q + 3 * i, qd, tr);
  for (int k = 0; k < 3; k++) { tau_fast[3 * i + k] = tf[k]; tau_ref[3 * i + k] = tr[k]; }
}
__global__ void k_track_swing(const double* phase, const double* p0, const double* pf, double* pos, double* vel, int n) {
  const int i = tid();
  if (i >= n) return;
  const double a[3] = {p0[3 * i], p0[3 * i + 1], p0[3 * i + 2]}, b[3] = {pf[3 * i], pf[3 * i + 1], pf[3 * i + 2]};
  double ps[3], vl[3];
  track_swing(params(), phase[i], a, b, ps, vl);
  for (int k = 0; k < 3; k++) { pos[3 * i + k] = ps[k]; vel[3 * i + k] = vl[k]; }
}
// wrench_from_state<4, KIN> of one robot per thread: st[36 i ..] = Rwb[9] Rwb_d[9] x x_d xdot xdot_d w w_d, fp[12 i ..] = body-frame feet
// (KIN = false) or joint angles (KIN = true).  out[19 i ..]: b[6], r[4][3], the returned finiteness value.
template <bool KIN>
__global__ void k_wrench(const double* st, const double* fp, double* out, int n) {
  const int i = tid();
  if (i >= n) return;
  const double* s = st + 36 * (long)i;
  RawState S;
  for (int k = 0; k < 9; k++) { S.R[k] = s[k]; S.Rd[k] = s[9 + k]; }
  for (int k = 0; k < 3; k++) {
    S.x[k] = s[18 + k]; S.xd[k] = s[21 + k]; S.xdot[k] = s[24 + k]; S.xdotd[k] = s[27 + k]; S.w[k] = s[30 + k]; S.wd[k] = s[33 + k];
  }
  double f[12];
  for (int k = 0; k < 12; k++) f[k] = fp[12 * (long)i + k];
  Wrench<4> W;
  const double fin = wrench_from_state<4, KIN>(params(), S, f, 0, W);
  double* o = out + 19 * (long)i;
  for (int k = 0; k < 6; k++) o[k] = W.b[k];
  for (int j = 0; j < 4; j++)
    for (int k = 0; k < 3; k++) o[6 + 3 * j + k] = W.r[j][k];
  o[18] = fin;
}
// plan_foothold of one leg per thread: in[24 i ..] = Rwb[9] x xdot w xdot_d pc (pc = Rwb foot_body, the lever arm)
__global__ void k_foothold(const int* leg, const double* in, double* fh, int n) {
  const int i = tid();
  if (i >= n) return;
  const int l = leg[i];
  if (l < 0 || l > 3) return;
  const double* s = in + 24 * (long)i;
  double R[9], x[3], xdot[3], w[3], xdd[3], pc[3], o[3];
  for (int k = 0; k < 9; k++) R[k] = s[k];
  for (int k = 0; k < 3; k++) { x[k] = s[9 + k]; xdot[k] = s[12 + k]; w[k] = s[15 + k]; xdd[k] = s[18 + k]; pc[k] = s[21 + k]; }
  plan_foothold(params(), l, R, x, xdot, w, xdd, pc, o);
  for (int k = 0; k < 3; k++) fh[3 * (long)i + k] = o[k];
}
// M: packed lower triangles (index r (r + 1) / 2 + c), x: right-hand sides in, solutions out
template <int N>
__global__ void k_ldlt(const double* M, double* x, int* ok, int n) {
  const int i = tid();
  if (i >= n) return;
  constexpr int T = N * (N + 1) / 2;
  double a[T], b[N];
  for (int k = 0; k < T; k++) a[k] = M[(long)T * i + k];
  for (int k = 0; k < N; k++) b[k] = x[(long)N * i + k];
  ok[i] = ldlt_solve<N>(a, b) ? 1 : 0;
  for (int k = 0; k < N; k++) x[(long)N * i + k] = b[k];
}
__global__ void k_tag(const double* v, const int* code, const int* free_face, const double* slack, const double* nd, double* tagged,
                      int* code_back, double* cand, int n) {
  const int i = tid();
  if (i >= n) return;
  const int c = code[i] & 31;
  tagged[i] = tag(v[i], c);
  code_back[i] = tag_code(tagged[i]);
  cand[i] = step_cand(free_face[i] != 0, slack[i], nd[i], c);
}
// One value per lane of whole waves (n a multiple of 64, every lane active: the DPP / permlane / MFMA reductions read
// their neighbours).  out[5 i ..]: group_sum, group_sum_add(v, addend[i]), group_min, group_max, and the bits of group_or.
template <int G, bool S>
__global__ void k_group(const double* v, const double* addend, const int* bits, double* out, int n) {
  const int i = tid();
  const bool in = i < n;  // (n is a multiple of the block: always true, kept so a short array cannot be overrun)
  const double x = in ? v[i] : 0.0, a = in ? addend[i] : 0.0;
  const int b = in ? bits[i] : 0;
  const double s = group_sum<G, S>(x);
  const double sa = group_sum_add<G, S>(x, a);
  const double mn = group_min<G, S>(x);
  const double mx = group_max<G, S>(x);
  const int o = group_or<G, S>(b);
  if (in) {
    out[5 * i] = s; out[5 * i + 1] = sa; out[5 * i + 2] = mn; out[5 * i + 3] = mx;
    out[5 * i + 4] = __longlong_as_double((long long)(unsigned)o);
  }
}

// ---------------------------------------------------------------- working-set recalculations (EQPs)
// One robot per lane group, whole waves with every lane active (the group reductions and the LDS exchange read their neighbours):
// the launchers refuse an n that does not fill its blocks.  Inputs per robot: b[6], r[4][3], a 4-bit stance mask and the cube
// (sx, sy, sz) of each foot.  A lane's robot and member come from lane_group / lane_member, foot0 = member (4 / G), as in the kernels.
template <int FPL>
__device__ __forceinline__ void load_robot(const double* b, const double* r, const int* cube, long robot, int foot0, double sign_b, Wrench<FPL>& Wr,
                                           Cube<FPL>& C) {
#pragma unroll
  for (int k = 0; k < 6; k++) Wr.b[k] = sign_b * b[6 * robot + k];
#pragma unroll
  for (int i = 0; i < FPL; i++) {
#pragma unroll
    for (int k = 0; k < 3; k++) Wr.r[i][k] = r[12 * robot + 3 * (foot0 + i) + k];
    C.sx[i] = cube[12 * robot + 3 * (foot0 + i)];
    C.sy[i] = cube[12 * robot + 3 * (foot0 + i) + 1];
    C.sz[i] = cube[12 * robot + 3 * (foot0 + i) + 2];
  }
}
// EqpDiagW<UNIFORM, G>: setup, then solve.  UC: the constants travel as a UConst (load_uconst + pin_uconst, mode 2's carrier).
// Out: every member writes the f and g of its own feet into row `robot` and its gscale and ok into [robot][member].
template <bool UNIFORM, int G, bool UC>
__global__ void k_eqp_diagw(const double* b, const double* r, const int* stance, const int* cube, double* f, double* g, double* gscale, int* ok, int n) {
  using Eqp = EqpDiagW<UNIFORM, G>;
  constexpr bool S = Eqp::kStrided;
  constexpr int FPL = 4 / G;
  const int lane = (int)threadIdx.x;
  const int member = lane_member<G, S>(lane);
  const long robot = (long)blockIdx.x * (kBlock / G) + lane_group<G, S>(lane);  // < n: the launcher takes whole blocks only
  const int foot0 = member * FPL;
  Wrench<FPL> Wr;
  Cube<FPL> C;
  load_robot<FPL>(b, r, cube, robot, foot0, -1.0, Wr, C);  // -b: the 6x6 forms keep the NEGATED wrench target in Wr.b (Eqp::kNegB)
  static_assert(Eqp::kNegB, "the 6x6 forms take -b");
  const uint32_t st = (uint32_t)stance[robot] & 15u;
  Eqp eqp(nullptr);
  eqp.setup(params(), Wr, foot0);
  double fo[3 * FPL], go[3 * FPL];
  bool pd;
  if constexpr (UC) {
    UConst uc = load_uconst(params());
    pin_uconst(uc);
    pd = eqp.solve(uc, Wr, C, st, foot0, fo, go);
  } else {
    pd = eqp.solve(params(), Wr, C, st, foot0, fo, go);
  }
#pragma unroll
  for (int k = 0; k < 3 * FPL; k++) { f[12 * robot + 3 * foot0 + k] = fo[k]; g[12 * robot + 3 * foot0 + k] = go[k]; }
  gscale[4 * robot + member] = eqp.gscale;
  ok[4 * robot + member] = pd ? 1 : 0;
  (void)n;
}
// EqpDense: one robot per lane, its own 78 x 64 doubles of dynamic LDS per block
__global__ void k_eqp_dense(const double* b, const double* r, const int* stance, const int* cube, double* f, double* g, int* ok, int n) {
  extern __shared__ __attribute__((aligned(16))) double probe_lds[];
  const int lane = (int)threadIdx.x;
  const long robot = (long)blockIdx.x * kBlock + lane;
  Wrench<4> Wr;
  Cube<4> C;
  load_robot<4>(b, r, cube, robot, 0, 1.0, Wr, C);
  static_assert(!EqpDense::kNegB, "the dense forms take b");
  const uint32_t st = (uint32_t)stance[robot] & 15u;
  EqpDense eqp(probe_lds + lane);
  eqp.setup(params(), Wr, 0);
  double fo[12], go[12];
  const bool pd = eqp.solve(params(), Wr, C, st, 0, fo, go);
#pragma unroll
  for (int k = 0; k < 12; k++) { f[12 * robot + k] = fo[k]; g[12 * robot + k] = go[k]; }
  ok[robot] = pd ? 1 : 0;
  (void)n;
}
// EqpDense4: X_DOUBLES of dynamic LDS per wave; setup once, then solve on cube and on cube2 for the same robot (the second
// recalculation reads the tile the first one left).  f, g: [2][n][12], ok: [2][n][4].
__global__ void k_eqp_dense4(const double* b, const double* r, const int* stance, const int* cube, const int* cube2, double* f, double* g, int* ok, int n) {
  extern __shared__ __attribute__((aligned(16))) double probe_lds[];
  const int lane = (int)threadIdx.x;
  const int member = lane_member<4, true>(lane);
  const long robot = (long)blockIdx.x * 16 + lane_group<4, true>(lane);
  Wrench<1> Wr;
  Cube<1> C, C2;
  load_robot<1>(b, r, cube, robot, member, 1.0, Wr, C);
  load_robot<1>(b, r, cube2, robot, member, 1.0, Wr, C2);
  static_assert(!EqpDense4::kNegB, "the dense forms take b");
  const uint32_t st = (uint32_t)stance[robot] & 15u;
  EqpDense4 eqp(probe_lds + lane);
  eqp.setup(params(), Wr, member);
  double fo[3], go[3];
  bool pd = eqp.solve(params(), Wr, C, st, member, fo, go);
#pragma unroll
  for (int k = 0; k < 3; k++) { f[12 * robot + 3 * member + k] = fo[k]; g[12 * robot + 3 * member + k] = go[k]; }
  ok[4 * robot + member] = pd ? 1 : 0;
  pd = eqp.solve(params(), Wr, C2, st, member, fo, go);
  const long o = 12 * (long)n;
#pragma unroll
  for (int k = 0; k < 3; k++) { f[o + 12 * robot + 3 * member + k] = fo[k]; g[o + 12 * robot + 3 * member + k] = go[k]; }
  ok[4 * (long)n + 4 * robot + member] = pd ? 1 : 0;
}
// clamp_foot and the foot code.  in[6 i ..] = mu lo hi fx fy fz, w[3 i ..] = the kept state (wx, wy, wz).
// out[3 i ..] = the clamped point, state[7 i ..] = sx sy sz, moved, then dec2 of the three fields of encode_foot(sx, sy, sz).
__global__ void k_clamp_foot(const double* in, const int* w, double* out, int* state, int n) {
  const int i = tid();
  if (i >= n) return;
  const double* a = in + 6 * (long)i;
  double fx = a[3], fy = a[4], fz = a[5];
  int sx, sy, sz;
  const bool moved = clamp_foot(a[0], a[1], a[2], w[3 * i], w[3 * i + 1], w[3 * i + 2], fx, fy, fz, sx, sy, sz);
  out[3 * (long)i] = fx; out[3 * (long)i + 1] = fy; out[3 * (long)i + 2] = fz;
  const uint32_t code = encode_foot(sx, sy, sz);
  int* s = state + 7 * (long)i;
  s[0] = sx; s[1] = sy; s[2] = sz; s[3] = moved ? 1 : 0;
  s[4] = dec2(code); s[5] = dec2(code >> 2); s[6] = dec2(code >> 4);
}

template <class K, class... A>
hipError_t launch(K kernel, int n, hipStream_t st, A... args) {
  if (n < 0) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(kernel, grid_for(n), dim3(kBlock), 0, st, args..., n);
  return hipGetLastError();
}

}  // namespace

extern "C" {

// The constants of the kinematic primitives and of the wrench assembly / foothold planner, from flat arrays (gains[12] = kp_p kd_p
// kp_w kd_w); every other field of DevParams stays zero.
hipError_t qcp_set_params(const double* hip, const double* links, const double* jc_kff, const double* jc_kp, const double* jc_kd,
                          const double* traj_basis, double t_swing, double t_stance, double swing_height, const double* gains,
                          const double* kff, double mass, const double* Ib, const double* planner_hip, double planner_k, hipStream_t st) {
  DevParams p;
  std::memset(&p, 0, sizeof(p));
  std::memcpy(p.hip, hip, sizeof(p.hip));
  std::memcpy(p.links, links, sizeof(p.links));
  std::memcpy(p.jc_kff, jc_kff, sizeof(p.jc_kff));
  std::memcpy(p.jc_kp, jc_kp, sizeof(p.jc_kp));
  std::memcpy(p.jc_kd, jc_kd, sizeof(p.jc_kd));
  std::memcpy(p.traj_basis, traj_basis, sizeof(p.traj_basis));
  p.t_swing = t_swing;
  p.t_stance = t_stance;
  p.swing_height = swing_height;
  std::memcpy(p.kp_p, gains, sizeof(p.kp_p));
  std::memcpy(p.kd_p, gains + 3, sizeof(p.kd_p));
  std::memcpy(p.kp_w, gains + 6, sizeof(p.kp_w));
  std::memcpy(p.kd_w, gains + 9, sizeof(p.kd_w));
  std::memcpy(p.kff, kff, sizeof(p.kff));
  p.mass = mass;
  std::memcpy(p.Ib, Ib, sizeof(p.Ib));
  std::memcpy(p.planner_hip, planner_hip, sizeof(p.planner_hip));
  p.planner_k = planner_k;
  hipLaunchKernelGGL(k_set_params, dim3(1), dim3(kBlock), 0, st, p);
  return hipGetLastError();
}

hipError_t qcp_sincos(const double* x, double* s, double* c, int n, hipStream_t st) { return launch(k_sincos, n, st, x, s, c); }
hipError_t qcp_rsqrt_rcp(const double* x, double* rs, double* rc, int n, hipStream_t st) { return launch(k_rsqrt_rcp, n, st, x, rs, rc); }
hipError_t qcp_angle_axis(const double* m, double* out, int n, hipStream_t st) { return launch(k_angle_axis, n, st, m, out); }
hipError_t qcp_wraps(const double* x, double* out, int n, hipStream_t st) { return launch(k_wraps, n, st, x, out); }
hipError_t qcp_leg(const int* leg, const double* q, const double* f, double* trig, double* p, double* tau_c, double* tau_g, int n,
                   hipStream_t st) {
  return launch(k_leg, n, st, leg, q, f, trig, p, tau_c, tau_g);
}
hipError_t qcp_pinv3(const double* J, const double* v, double* x, int n, hipStream_t st) { return launch(k_pinv3, n, st, J, v, x); }
hipError_t qcp_swing_torque(const int* leg, const double* pb, const double* vb, const double* q, const double* qdot, double* tau, int n,
                            hipStream_t st) {
  return launch(k_swing_torque, n, st, leg, pb, vb, q, qdot, tau);
}
hipError_t qcp_swing_pd(const int* leg, const double* qr, const double* q, double* tau_fast, double* tau_ref, int n, hipStream_t st) {
  return launch(k_swing_pd, n, st, leg, qr, q, tau_fast, tau_ref);
}
hipError_t qcp_track_swing(const double* phase, const double* p0, const double* pf, double* pos, double* vel, int n, hipStream_t st) {
  return launch(k_track_swing, n, st, phase, p0, pf, pos, vel);
}
// kin = 0: wrench_from_state<4, false> (fp = body-frame feet), 1: <4, true> (fp = joint angles)
hipError_t qcp_wrench(int kin, const double* st, const double* fp, double* out, int n, hipStream_t s) {
  return kin ? launch(k_wrench<true>, n, s, st, fp, out) : launch(k_wrench<false>, n, s, st, fp, out);
}
hipError_t qcp_foothold(const int* leg, const double* in, double* fh, int n, hipStream_t st) { return launch(k_foothold, n, st, leg, in, fh); }
hipError_t qcp_ldlt6(const double* M, double* x, int* ok, int n, hipStream_t st) { return launch(k_ldlt<6>, n, st, M, x, ok); }
hipError_t qcp_ldlt12(const double* M, double* x, int* ok, int n, hipStream_t st) { return launch(k_ldlt<12>, n, st, M, x, ok); }
hipError_t qcp_tag(const double* v, const int* code, const int* free_face, const double* slack, const double* nd, double* tagged, int* code_back,
                   double* cand, int n, hipStream_t st) {
  return launch(k_tag, n, st, v, code, free_face, slack, nd, tagged, code_back, cand);
}
// variant 0: (G, S) = (2, false), 2: (4, true): the two lane layouts of the kernels
hipError_t qcp_group(int variant, const double* v, const double* addend, const int* bits, double* out, int n, hipStream_t st) {
  if (n % kBlock != 0) return hipErrorInvalidValue;
  switch (variant) {
    case 0: return launch(k_group<2, false>, n, st, v, addend, bits, out);
    case 2: return launch(k_group<4, true>, n, st, v, addend, bits, out);
    default: return hipErrorInvalidValue;
  }
}

// The QP's constants (mu, fzmin, fzmax, S, V, w, W, inv_wx, inv_wy, inv_bz, Vd, w_u, inv_w_u, inv_bz_u - and everything else
// qc_create derives) by the product's own derive_params (qc_host.hpp), into the probe's constants.  Also reports what the host
// rule makes of the parameters: flags[0] = W diagonal, [1] = uniform, [2] = small_w (the 6x6 forms are routed to the dense form),
// [3] = the form the handle would run (QC_FORM_*).  A parameter set derive_params refuses returns hipErrorInvalidValue.
hipError_t qcp_set_qp_params(const qc_params* p, int* flags, hipStream_t st) {
  DevParams d;
  Tuning t;
  if (derive_params(p, d, t) != QC_OK) return hipErrorInvalidValue;
  if (flags) { flags[0] = t.cfg_diag_w; flags[1] = t.cfg_uniform; flags[2] = t.small_w; flags[3] = form_of(t); }
  hipLaunchKernelGGL(k_set_params, dim3(1), dim3(kBlock), 0, st, d);
  return hipGetLastError();
}
// the host rule's threshold on max diag(S) / min diag(W) (qc_host.hpp)
double qcp_dense_ratio(void) { return QC_DENSE_RATIO; }

// variant: 0-2 uniform G = 1, 2, 4; 3-5 general G = 1, 2, 4; 6 uniform G = 4 with the constants in a UConst (mode 2).  n robots, a
// multiple of the robots of a block (64 / G).
hipError_t qcp_eqp_diagw(int variant, const double* b, const double* r, const int* stance, const int* cube, double* f, double* g, double* gscale,
                         int* ok, int n, hipStream_t st) {
  const int G = variant == 6 ? 4 : 1 << (variant % 3);
  if (variant < 0 || variant > 6 || n <= 0 || n % (kBlock / G) != 0) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(n / (kBlock / G)));
#define QCP_DIAGW(U, GG, UC) hipLaunchKernelGGL((k_eqp_diagw<U, GG, UC>), grid, dim3(kBlock), 0, st, b, r, stance, cube, f, g, gscale, ok, n)
  switch (variant) {
    case 0: QCP_DIAGW(true, 1, false); break;
    case 1: QCP_DIAGW(true, 2, false); break;
    case 2: QCP_DIAGW(true, 4, false); break;
    case 3: QCP_DIAGW(false, 1, false); break;
    case 4: QCP_DIAGW(false, 2, false); break;
    case 5: QCP_DIAGW(false, 4, false); break;
    default: QCP_DIAGW(true, 4, true); break;
  }
#undef QCP_DIAGW
  return hipGetLastError();
}
hipError_t qcp_eqp_dense(const double* b, const double* r, const int* stance, const int* cube, double* f, double* g, int* ok, int n, hipStream_t st) {
  if (n <= 0 || n % kBlock != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_eqp_dense, dim3((unsigned)(n / kBlock)), dim3(kBlock), sizeof(double) * EqpDense::kLdsDoubles, st, b, r, stance, cube, f, g, ok, n);
  return hipGetLastError();
}
hipError_t qcp_eqp_dense4(const double* b, const double* r, const int* stance, const int* cube, const int* cube2, double* f, double* g, int* ok, int n,
                          hipStream_t st) {
  if (n <= 0 || n % 16 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_eqp_dense4, dim3((unsigned)(n / 16)), dim3(kBlock), sizeof(double) * EqpDense4::X_DOUBLES, st, b, r, stance, cube, cube2, f, g, ok, n);
  return hipGetLastError();
}
hipError_t qcp_clamp_foot(const double* in, const int* w, double* out, int* state, int n, hipStream_t st) { return launch(k_clamp_foot, n, st, in, w, out, state); }

}  // extern "C"
