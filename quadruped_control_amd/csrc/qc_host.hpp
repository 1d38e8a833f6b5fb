// qc_host.hpp - the host logic behind the C ABI that needs no device (C++17, no HIP): qc_balance.hip includes it for the
// library, tests/cpp/host_logic_test.cpp compiles it with the host compiler alone.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>

#include "../../include/qc_balance.h"
#include "../../include/qc_tangent.h"
#include "../../include/qc_plant_model.h"
#include "qc_device.hpp"
#include "qc_plant.hpp"
#include "qc_plant_adjoint.hpp"
#include "qc_leg_plant.hpp"
#include "qc_leg_plant_adjoint.hpp"
#include "qc_certify.hpp"
#include "qc_sensitivity.hpp"
#include "qc_sensitivity_rot.hpp"
#include "qc_sensitivity_params.hpp"
#include "qc_sensitivity_kin.hpp"
#include "qc_sensitivity_swing.hpp"
#include "qc_swing_reference.hpp"
#include "qc_commander.hpp"
#include "qc_support_polygon.hpp"
#include "qc_com_reference.hpp"
#include "qc_tangent.hpp"
#include "qc_plant_tangent.hpp"
#include "qc_swing_tangent.hpp"
#include "qc_torque_tangent.hpp"
#include "qc_leg_plant_tangent.hpp"
#include "qc_swing_reference_tangent.hpp"
#include "qc_command_tangent.hpp"
#include "qc_param_tangent.hpp"
#include "qc_plant_model.hpp"

namespace qc {

// The 6x6 forms solve the DUAL system M = S^-1 + A~ B^-1 A~^T, whose B^-1 = O(1/w) part has rank = the number of free force
// coordinates: with fewer than six of them free, M is a rank-k term of size 1/w on top of an S^-1 of order one and the forces
// (1/w) A~^T v come out with an absolute error of eps (S/w) |b| - 1e-5 N at S/w = 1e9 (the parameter campaigns' 1.4e-5 ... 2.4e-5
// at w ~ 1e-7, S ~ 100: profiles/r06_fuzz_campaigns.log), 1e-8 N at the reference's S/w = 1e6 (commander_node.cpp:305-307).  The
// dense 12x12 form factorises the PRIMAL reduced Hessian, which is well-conditioned exactly there (tests/test_gpu_parity.py::
// test_small_w_golden: < 5e-6 where the dual forms are at 2.4e-5), at three to five times the time.  Above this ratio a handle
// therefore runs the dense form: accuracy before speed for regularisation weights this far below the reference's.
#ifndef QC_DENSE_RATIO
#define QC_DENSE_RATIO 3.0e8
#endif

inline thread_local std::string g_err;
inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// Two refusals every versioned entry point shares (`who`: the entry point, for the message).  A struct of another revision of the
// header: `got` is its struct_size field, `want` this library's sizeof, `default_fn_name` the function that sets the field.
inline int check_struct_size(const char* who, const char* struct_name, const char* default_fn_name, size_t got, size_t want) {
  if (got == want) return QC_OK;
  char msg[192];
  std::snprintf(msg, sizeof(msg), "%s: %s.struct_size is %zu, this library's %s has %zu B (%s sets it)", who, struct_name, got, struct_name, want, default_fn_name);
  return fail(QC_ERR_INVALID, msg);
}
// One lane per robot in blocks of `block`: a launch holds fewer than 2^32 threads.
inline int check_one_launch(const char* who, size_t n, int block) {
  if (n > (size_t)0xFFFFFF * (size_t)block) return fail(QC_ERR_INVALID, std::string(who) + ": n is beyond one launch");
  return QC_OK;
}
// How an entry point with an io record opens: the handle and the batch (`others`) and the record are there, in this library's revision.
template <class Io>
int check_io(const char* who, bool others, const Io* io, const char* struct_name, const char* default_fn_name) {
  if (!others || !io) return fail(QC_ERR_INVALID, std::string(who) + ": null argument");
  return check_struct_size(who, struct_name, default_fn_name, io->struct_size, sizeof(Io));
}
// workgroups of a per-robot kernel for n robots: `block` robots each, capped at `cap` (the waves stride beyond it)
inline unsigned capped_blocks(size_t n, int block, int cap) {
  const size_t b = (n + (size_t)block - 1) / (size_t)block;
  return (unsigned)(b < (size_t)cap ? b : (size_t)cap);
}

// What qc_create derived from its parameters about the formulation, and the overrides of qc_set_tuning.
struct Tuning {
  bool diag_w = false;   // W diagonal -> 6x6 formulation
  bool uniform = false;  // additionally S diagonal and W = w*I -> scalar-constant specialisation
  // what qc_create was given: the tuning overrides (force_general / force_dense / max_iter / probe_batch_load) restore from these
  bool cfg_diag_w = false, cfg_uniform = false;
  bool small_w = false;    // qc_create's rule: max diag(S) / min diag(W) above QC_DENSE_RATIO - the 6x6 dual forms lose digits that matter there
  bool auto_dense = true;  // ... and such a handle runs the dense 12x12 form (qc_set_tuning "auto_dense", default on)
  int cfg_max_iter = 0;
  bool force_general = false, force_dense = false, probing = false;
  // launch heuristics (defaults from measurements; qc_set_tuning overrides them)
  long chunk_override = 0;      // > 0: robots per wave (at most one fill, 64 / G)
  int group_override = 0;       // 1, 2, 4: lanes per robot
  int wave_slots_override = 0;  // > 0: resident workgroups assumed for every kernel instead of the occupancy query
  int race_override = -1;       // -1 heuristic; 0 / 1: no racing strategies; 2, 4: at most that many per robot
  int pair_override = -1;       // MODE 3 (paired waves): -1 heuristic, 0 never, 1 whenever the form allows it
  int pair_th = 0;              // hand-over threshold (0: heuristic)
  int pair_refill = 0;          // free lane groups that trigger a refill (0: heuristic)
  int pair_solo = 1;            // 1: the last round of workgroups keeps each wave's stragglers in the wave (default), 0: pairs everywhere
};

// the formulation a handle runs, from what qc_create was given and the tuning flags - in one place, whatever the order of the calls
inline void resolve_form(Tuning& t) {
  t.diag_w = t.cfg_diag_w && !t.force_dense && !(t.small_w && t.auto_dense);
  t.uniform = t.cfg_uniform && !t.force_general;
}
// the formulation a handle runs (resolve_form)
inline int form_of(const Tuning& t) { return !t.diag_w ? QC_FORM_DENSE : (t.uniform ? QC_FORM_UNIFORM : QC_FORM_GENERAL); }

// Cholesky-based inverse of a small SPD matrix (host, once per handle)
inline bool spd_inverse(const double* A, int n, double* inv) {
  double L[36];
  for (int i = 0; i < n; i++)
    for (int j = 0; j <= i; j++) {
      double s = A[i * n + j];
      for (int k = 0; k < j; k++) s -= L[i * n + k] * L[j * n + k];
      if (i == j) {
        if (!(s > 0.0)) return false;
        L[i * n + i] = std::sqrt(s);
      } else {
        L[i * n + j] = s / L[j * n + j];
      }
    }
  for (int c = 0; c < n; c++) {
    double y[6], x[6];
    for (int i = 0; i < n; i++) {
      double s = (i == c) ? 1.0 : 0.0;
      for (int k = 0; k < i; k++) s -= L[i * n + k] * y[k];
      y[i] = s / L[i * n + i];
    }
    for (int i = n - 1; i >= 0; i--) {
      double s = y[i];
      for (int k = i + 1; k < n; k++) s -= L[k * n + i] * x[k];
      x[i] = s / L[i * n + i];
    }
    for (int i = 0; i < n; i++) inv[i * n + c] = x[i];
  }
  return true;
}

// Columns 0..2 of the inverse of FootTrajectory::initSystem()'s 7x7 matrix (trajectory.cpp:256-277):
// the responses of the sextic coefficients to p_start, p_final and p_centre.  basis[3*j + k].
inline void sextic_basis(double* basis) {
  double A[7][7] = {{1, 0, 0, 0, 0, 0, 0}, {1, 1, 1, 1, 1, 1, 1}, {1, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625},
                    {0, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6}, {0, 0, 2, 0, 0, 0, 0}, {0, 0, 2, 6, 12, 20, 30}};
  double M[7][10];
  for (int i = 0; i < 7; i++) {
    for (int j = 0; j < 7; j++) M[i][j] = A[i][j];
    for (int k = 0; k < 3; k++) M[i][7 + k] = (i == k) ? 1.0 : 0.0;
  }
  for (int c = 0; c < 7; c++) {
    int p = c;
    for (int r = c + 1; r < 7; r++) if (std::fabs(M[r][c]) > std::fabs(M[p][c])) p = r;
    for (int j = 0; j < 10; j++) std::swap(M[c][j], M[p][j]);
    const double piv = M[c][c];
    for (int j = 0; j < 10; j++) M[c][j] /= piv;
    for (int r = 0; r < 7; r++) {
      if (r == c) continue;
      const double m = M[r][c];
      for (int j = 0; j < 10; j++) M[r][j] -= m * M[c][j];
    }
  }
  for (int j = 0; j < 7; j++)
    for (int k = 0; k < 3; k++) basis[3 * j + k] = M[j][7 + k];
}

inline void default_kinematics(qc_kinematics* k) {  // qc_default_kinematics
  if (!k) return;
  // QuadrupedKinematics::QuadrupedKinematics(), kinematics.cpp:20-47
  const double xbh = 0.196, ybh = 0.050, zbh = 0.0, l1 = 0.077, l2 = 0.211, l3 = 0.230;
  const double hip[12] = {-xbh, ybh, zbh, xbh, ybh, zbh, -xbh, -ybh, zbh, xbh, -ybh, zbh};  // RL FL RR FR
  const double links[12] = {l1, -l2, -l3, l1, -l2, -l3, -l1, -l2, -l3, -l1, -l2, -l3};    // left, left, right, right
  std::memcpy(k->hip, hip, sizeof(hip));
  std::memcpy(k->links, links, sizeof(links));
  k->tau_min = -20.0;  // commander_node.cpp:324-325
  k->tau_max = 20.0;
  const double kff[3] = {0.0, 0.0, 0.0}, kp[3] = {40.0, 40.0, 50.0}, kd[3] = {1.0, 1.0, 1.0};  // mit_cheetah_config.yaml:50-53
  std::memcpy(k->jc_kff, kff, sizeof(kff));
  std::memcpy(k->jc_kp, kp, sizeof(kp));
  std::memcpy(k->jc_kd, kd, sizeof(kd));
  const double xbt = 0.196, ybt = 0.127, zbt = 0.0;  // foot_planner.cpp:27-42
  const double phip[12] = {-xbt, ybt, zbt, xbt, ybt, zbt, -xbt, -ybt, zbt, xbt, -ybt, zbt};
  std::memcpy(k->planner_hip, phip, sizeof(phip));
  k->planner_k = 0.01;     // foot_planner.cpp:25
  k->swing_height = 0.08;  // gait/height, commander_node.cpp:247
}

// the kinematic model and the swing planner's constants of a qc_kinematics, into the device constants
inline void copy_kinematics(DevParams& d, const qc_kinematics& k) {
  std::memcpy(d.hip, k.hip, sizeof(k.hip));
  std::memcpy(d.links, k.links, sizeof(k.links));
  d.tau_min = k.tau_min;
  d.tau_max = k.tau_max;
  std::memcpy(d.jc_kff, k.jc_kff, sizeof(k.jc_kff));
  std::memcpy(d.jc_kp, k.jc_kp, sizeof(k.jc_kp));
  std::memcpy(d.jc_kd, k.jc_kd, sizeof(k.jc_kd));
  std::memcpy(d.planner_hip, k.planner_hip, sizeof(k.planner_hip));
  d.planner_k = k.planner_k;
  d.swing_height = k.swing_height;
}

// ---------------------------------------------------------------- qc_create: validation and derived constants
// what qc_create refuses about its parameters without looking at a device
inline int check_params(const qc_params* p) {
  if (!(p->mu > 0.0) || !(p->mass > 0.0)) return fail(QC_ERR_INVALID, "qc_create: mu and mass must be > 0");
  if (!(p->fzmin >= 0.0) || !(p->fzmax >= p->fzmin)) return fail(QC_ERR_INVALID, "qc_create: need 0 <= fzmin <= fzmax");
  // The cone rows of the reference are two-sided with +-1e6 on the far side (BC.cpp:296-301: -1e6 <= fx - mu fz <= 0, ...).
  // Inside the cone |fx -+ mu fz| <= 2 mu fz <= 2 mu fzmax, so those sides cannot bind - and this solver does not carry
  // them - as long as 2 mu fzmax < 1e6.  Parameters beyond that would make the reference's QP a different one: refused.
  // (the hand-over records of the re-packed tails carry the recalculation count in 16 bits)
  if (p->max_iter > QC_MAX_ITER_LIMIT) return fail(QC_ERR_INVALID, "qc_create: max_iter must be <= 65535");
  if (!(2.0 * p->mu * p->fzmax < 1.0e6))
    return fail(QC_ERR_INVALID, "qc_create: need 2 * mu * fzmax < 1e6 (the +-1e6 sides of the reference's cone rows, balance_controller.cpp:296-301, are not carried)");
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < i; j++)
      if (std::fabs(p->S[6 * i + j] - p->S[6 * j + i]) > 1e-12 * (std::fabs(p->S[6 * i + i]) + std::fabs(p->S[6 * j + j])))
        return fail(QC_ERR_INVALID, "qc_create: S must be symmetric");
  for (int i = 0; i < 12; i++)
    if (!(p->W[12 * i + i] > 0.0)) return fail(QC_ERR_INVALID, "qc_create: W must be positive definite");
  for (int i = 0; i < 12; i++)
    for (int j = 0; j < i; j++)
      if (std::fabs(p->W[12 * i + j] - p->W[12 * j + i]) > 1e-12 * (p->W[12 * i + i] + p->W[12 * j + j]))
        return fail(QC_ERR_INVALID, "qc_create: W must be symmetric");
  return QC_OK;
}

// the device constants and the formulation flags of validated parameters (fails on an S that is not positive definite)
inline int derive_params(const qc_params* p, DevParams& d, Tuning& t) {
  bool diag = true;
  for (int i = 0; i < 12; i++)
    for (int j = 0; j < 12; j++)
      if (i != j && p->W[12 * i + j] != 0.0) diag = false;
  std::memset(&d, 0, sizeof(d));
  d.mu = p->mu; d.mass = p->mass; d.fzmin = p->fzmin; d.fzmax = p->fzmax;
  std::memcpy(d.Ib, p->Ib, sizeof(d.Ib));
  std::memcpy(d.S, p->S, sizeof(d.S));
  if (!spd_inverse(p->S, 6, d.V)) return fail(QC_ERR_INVALID, "qc_create: S must be positive definite");
  for (int i = 0; i < 12; i++) d.w[i] = p->W[12 * i + i];
  std::memcpy(d.W, p->W, sizeof(d.W));
  for (int i = 0; i < 4; i++) {
    d.inv_wx[i] = 1.0 / d.w[3 * i];
    d.inv_wy[i] = 1.0 / d.w[3 * i + 1];
    for (int a = 0; a < 2; a++)
      for (int b = 0; b < 2; b++)
        d.inv_bz[4 * i + 2 * a + b] = 1.0 / (d.w[3 * i + 2] + p->mu * p->mu * (a * d.w[3 * i] + b * d.w[3 * i + 1]));
  }
  bool uni = diag;
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++)
      if (i != j && p->S[6 * i + j] != 0.0) uni = false;
  for (int i = 1; i < 12; i++)
    if (p->W[12 * i + i] != p->W[0]) uni = false;
  t.cfg_diag_w = diag;
  t.cfg_uniform = uni;
  {
    double smax = 0.0, wmin = p->W[0];
    for (int i = 0; i < 6; i++) smax = std::fmax(smax, p->S[6 * i + i]);
    for (int i = 1; i < 12; i++) wmin = std::fmin(wmin, p->W[12 * i + i]);
    t.small_w = diag && smax > QC_DENSE_RATIO * wmin;
  }
  resolve_form(t);
  for (int i = 0; i < 6; i++) d.Vd[i] = d.V[6 * i + i];
  d.w_u = p->W[0];
  d.inv_w_u = 1.0 / p->W[0];
  for (int k = 0; k < 3; k++) d.inv_bz_u[k] = 1.0 / (p->W[0] * (1.0 + p->mu * p->mu * k));
  std::memcpy(d.kff, p->kff, sizeof(d.kff));
  std::memcpy(d.kp_p, p->kp_p, sizeof(d.kp_p));
  std::memcpy(d.kd_p, p->kd_p, sizeof(d.kd_p));
  std::memcpy(d.kp_w, p->kp_w, sizeof(d.kp_w));
  std::memcpy(d.kd_w, p->kd_w, sizeof(d.kd_w));
  {
    qc_kinematics k;
    default_kinematics(&k);
    copy_kinematics(d, k);
    d.t_swing = 0.18;  // mit_cheetah_config.yaml:17-18
    d.t_stance = 0.8;
    sextic_basis(d.traj_basis);
  }
  d.stance_phase = 0.8 / (0.18 + 0.8);  // mit_cheetah_config.yaml:17-18
  // Multiplier tolerance, relative to max(1, |grad|_inf).  It has to sit just above the rounding noise of the
  // multipliers, not at a "reasonable" 1e-9: along a weakly active face the objective curves only with 2w, so a
  // multiplier accepted at -tol*|g| leaves the force tol*|g|/(2w) away from the minimiser (w = 2.8e-7, |g| ~ 1e6:
  // 1e-12 gave 0.2 N = 2e-3 relative in the parameter fuzz; 1e-13 ... 1e-15 all agree with the NNLS restatement
  // and change neither the recalculation counts of 1 M robots nor anything else measurable).
  d.tol_d = 1e-14;
  d.tol_start = d.tol_d;  // (polish on)
  d.max_iter = p->max_iter > 0 ? p->max_iter : 200;
  t.cfg_max_iter = d.max_iter;
  d.clamp_steps = 0;  // 0: per kernel (clamp_steps_for)
  d.tail_race = 1;
  d.polish = 1;  // the polish at acceptance (Lane::iterate)
  return QC_OK;
}

// ---------------------------------------------------------------- qc_set_tuning
// `upload`: the key changed a device constant, the caller rewrites the device copy
inline int set_tuning(Tuning& t, DevParams& dp, const char* key, double value, bool* upload) {
  const std::string k(key);
  bool params = false;
  if (k == "group") {
    const int g = (int)value;
    if (g != 0 && g != 1 && g != 2 && g != 4) return fail(QC_ERR_INVALID, "qc_set_tuning: group is 0 (heuristic), 1, 2 or 4");
    t.group_override = g;
  } else if (k == "one_fill") {  // (-1 heuristic / 1 always: every launch is one fill per wave, the key stays for existing callers)
    if (value == 0) return fail(QC_ERR_INVALID, "qc_set_tuning: one_fill = 0 asked for the persistent-wave kernels, which were removed");
  }
  else if (k == "chunk") t.chunk_override = value > 0 ? (long)value : 0;
  else if (k == "wave_slots") t.wave_slots_override = value > 0 ? (int)value : 0;
  else if (k == "race") {  // (0 / 1 also switch the race in the 4-lane tail of the wider kernels off)
    t.race_override = value < 0 ? -1 : (int)value;
    dp.tail_race = (value < 0 || value >= 2) ? 1 : 0;
    params = true;
  }
  else if (k == "pair") t.pair_override = value < 0 ? -1 : (value != 0 ? 1 : 0);
  else if (k == "pair_th") t.pair_th = value > 0 ? (int)value : 0;
  else if (k == "pair_refill") t.pair_refill = value > 0 ? (int)value : 0;
  else if (k == "pair_solo") t.pair_solo = value != 0 ? 1 : 0;
  else if (k == "force_general" || k == "force_dense") {
    // general 6x6 form on uniform weights / dense 12x12 form on a diagonal W (same minimiser).  The form follows from what
    // qc_create was given and the two flags, in one place, whatever the order of the calls.
    (k == "force_general" ? t.force_general : t.force_dense) = value != 0;
    resolve_form(t);
  } else if (k == "auto_dense") {  // 0: a diagonal W keeps its 6x6 form however small it is (QC_DENSE_RATIO above)
    t.auto_dense = value != 0;
    resolve_form(t);
  } else if (k == "tol_d") { dp.tol_d = value; dp.tol_start = dp.polish ? value : -value; params = true; }
  else if (k == "max_iter") {  // <= 0: back to the handle's own cap (qc_params.max_iter)
    if (value > (double)QC_MAX_ITER_LIMIT) return fail(QC_ERR_INVALID, "qc_set_tuning: max_iter must be <= 65535");
    t.probing = false;
    dp.max_iter = value > 0 ? (int)value : t.cfg_max_iter; params = true;
  }
  else if (k == "clamp_steps") { dp.clamp_steps = value >= 1 ? (int)value : 0; params = true; }
  else if (k == "polish") {  // 0: round 5's acceptance rule
    dp.polish = value != 0 ? 1 : 0;
    dp.tol_start = dp.polish ? dp.tol_d : -dp.tol_d;
    params = true;
  }
  else if (k == "probe_batch_load") {
    // measurement probe: load -> assemble -> store only (every robot reports QC_MAX_ITER); 0 restores the handle's own cap
    t.probing = value != 0;
    dp.max_iter = t.probing ? 0 : t.cfg_max_iter; params = true;
  } else return fail(QC_ERR_INVALID, "qc_set_tuning: unknown key '" + k + "'");
  *upload = params;
  return QC_OK;
}

// ---------------------------------------------------------------- launch planning
// One wave per 64-thread block; a group of G lanes per robot.  The group width trades latency for throughput
// (instructions per steady recalculation: 487 per 16 robots at G = 4, 730 per 32 at G = 2, ~1170 per 64 at G = 1):
// the planner takes the widest group with which the batch still fits ONE wave per SIMD - such a batch cannot fill
// the chip anyway and the slowest robot's serial chain is what is timed - i.e. G = 4 up to CUs x 4 x 16 robots
// (16 384), G = 2 up to twice that, and one lane per robot above (tools/size_scan.py: the cross-overs sit exactly
// there, cold and warm).  Every width finishes its last <= 16 running robots on the 4-lane body.  Every launch gives
// each wave one fill (mode 1 / 2) - the hardware scheduler refills the chip with the next workgroup - or, for the
// one-lane 6x6 kernels of large batches, a workgroup of two waves (mode 3, balance_pair_kernel); a chunk beyond one fill
// is an error at launch.
struct LaunchPlan {
  int kernel;  // index into KERNEL_KEYS (form, G, mode, race) and into the library's table of entry points
  unsigned blocks;
  long chunk;
  int p_th, p_refill;  // mode 3
  long resident;
};

// the instantiation that serves (form, G, mode, race): its index in KERNEL_KEYS, or -1
inline int find_kernel(int form, int G, int mode, int race = 1) {
  for (int i = 0; i < N_KERNELS; i++) {
    const KernelKey& k = KERNEL_KEYS[i];
    if (k.form == form && k.G == G && k.mode == mode && k.race == race) return i;
  }
  return -1;
}

// `resident(kernel, kin)`: workgroups of KERNEL_KEYS[kernel] (its joint_q variant with `kin`) the device holds at once
template <class Resident>
int plan_launch(int form, long n, bool kin, bool warm, const Tuning& t, int cus, Resident&& resident, LaunchPlan* lp) {
  // (a kernel that is not instantiated is an error, never another kernel in its place)
  const auto no_kernel = [] { return fail(QC_ERR_INVALID, "plan_launch: no kernel instantiation serves this form, group width, mode and race"); };
  int G = 1;
  const long simds = (long)cus * 4;
  const int r4 = find_kernel(form, 4, 1);
  if (r4 < 0) return no_kernel();
  const long cap4 = resident(r4, kin) * 16;
  if (form != QC_FORM_DENSE) {
    G = n <= 16 * simds ? 4 : (n <= 32 * simds ? 2 : 1);
    if (t.group_override) G = t.group_override;
  } else {
    // dense form: four lanes per robot while the batch fits the resident waves - the latency regime; one lane per robot
    // with the LDS-staged Hessian above that
    G = n <= cap4 ? 4 : 1;
    if (t.group_override) G = t.group_override == 4 ? 4 : 1;
    // a chunk of 17 ... 64 robots is more than a four-lane wave holds and exactly what a one-lane one-fill wave does (ADVICE r5:
    // rounds 2-4 served such a request on the one-lane kernel; it must not become an error because the four-lane one would have been picked)
    if (!t.group_override && G == 4 && t.chunk_override > 16 && t.chunk_override <= 64) G = 1;
  }
  // A request the kernels cannot honour is an error, not a silent change of the launch: a wave holds one fill.
  if (t.chunk_override > 64 / G)
    return fail(QC_ERR_INVALID, "qc_set_tuning: a chunk beyond one fill (64 / lanes per robot) asks for more robots than a wave holds");
  // MODE 3 (paired waves): 6x6 forms, one lane per robot, batches of at least four rounds of one-fill workgroups (524 288
  // robots): measured -5 % there and nothing below (profiles/r03_paired_waves.log) - with few rounds the consumer of two
  // waves' stragglers is mostly a longer chain at the end of the launch.  (Not the joint_q variants: they always run as
  // one-fill workgroups.)
  if (form != QC_FORM_DENSE && G == 1 && !kin && t.chunk_override <= 0) {
    const int r1 = find_kernel(form, 1, 1), rp = find_kernel(form, 1, 3);
    if (r1 < 0 || rp < 0) return no_kernel();
    const long res1 = resident(r1, kin);
    bool use_pair = n >= 4 * res1 * 64;
    if (t.pair_override >= 0) use_pair = t.pair_override != 0;
    if (use_pair) {
      const int p_th = t.pair_th > 0 ? (t.pair_th < PAIR_CAP ? t.pair_th : PAIR_CAP) : 24;
      // (1 ... 16 free lane groups: beyond 16 the refill test of the consumer could never fire and it would spin on a full list)
      const int p_refill = t.pair_refill > 0 ? (t.pair_refill < 16 ? t.pair_refill : 16) : 4;
      // (resident: two-wave workgroups of the pair kernel itself - its own registers and 26 KB of static LDS -, not half of the one-fill figure)
      *lp = LaunchPlan{rp, (unsigned)((n + 127) / 128), 128, p_th, p_refill, resident(rp, false)};
      return QC_OK;
    }
  }
  const long rpw = 64 / G;  // robots per wave fill
  const int rg = find_kernel(form, G, 1);
  if (rg < 0) return no_kernel();
  const long res = resident(rg, kin);
  long chunk = t.chunk_override > 0 ? t.chunk_override : rpw;
  const long blocks = (n + chunk - 1) / chunk;
  // one wave per SIMD is enough: the recalculation's constants stay resident in VGPRs (uniform G = 4 form)
  const int mode = (form == QC_FORM_UNIFORM && G == 4 && blocks <= (long)cus * 4) ? 2 : 1;
  // ... and when even that leaves SIMDs idle the 4-lane kernels (all three forms) race pivoting strategies on the
  // same robot (Lane: RACE): four per robot up to CUs x 4 x 4 robots (4 096)
  int race = 1;
  if (G == 4 && t.chunk_override <= 0 && (mode == 2 || form != QC_FORM_UNIFORM)) {
    // (a 2-way race up to 8 192 robots is built and selectable - qc_set_tuning("race", 2) - but measured neutral on
    // average: its two fewer recalculations pay for the heavier body, tools/race_scan.py)
    // (cold batches: a warm-started one has little chain to shorten - 10-17 us either way, 0.2-0.6 us dearer with the race,
    // tools/warm_race_scan.py)
    race = (!warm && n <= 4 * simds) ? 4 : 1;
    if (t.race_override >= 0) race = (t.race_override == 4 && n <= 4 * simds) ? 4 : ((t.race_override >= 2 && n <= 8 * simds) ? 2 : 1);
    chunk = 16 / race;
  }
  const int rk = find_kernel(form, G, mode, race);
  if (rk < 0) return no_kernel();
  *lp = LaunchPlan{rk, (unsigned)((n + chunk - 1) / chunk), chunk, 0, 0, res};
  return QC_OK;
}

// ---------------------------------------------------------------- argument checks of the batch entry points
// The argument check the batch entry points share (`who`: the entry point, for the message; built only on failure).  The two
// have always tested the required outputs and "joint_tau needs joint_q" in opposite orders; `outputs_first` keeps each its own.
inline int check_batch_args(const char* who, const qc_handle* h, size_t n, const qc_batch_in* in, const qc_batch_out* out, bool outputs_first) {
  const auto bad = [who](const char* what) { return fail(QC_ERR_INVALID, std::string(who) + what); };
  if (!h || !in || !out) return bad(": null argument");
  if (n == 0) return QC_OK;
  if (!in->Rwb || !in->Rwb_d || !in->x || !in->xdot || !in->w || !in->x_d || !in->xdot_d || !in->w_d || (!in->feet && !in->joint_q))
    return bad(": null input array");
  const bool no_outputs = !out->grf_body || !out->status, tau_alone = out->joint_tau && !in->joint_q;
  if (outputs_first && no_outputs) return bad(": grf_body and status are required");
  if (tau_alone) return bad(": joint_tau needs joint_q");
  if (no_outputs) return bad(": grf_body and status are required");
  return QC_OK;
}

// qc_control_batch: which of the optional swing and gait arrays go together (after check_batch_args)
inline int check_swing_gait_args(const qc_batch_in* in, const qc_batch_out* out) {
  const int n_sw = (in->swing_pos ? 1 : 0) + (in->swing_vel ? 1 : 0) + (in->joint_qdot ? 1 : 0);
  if (!in->swing_state && n_sw != 0 && (n_sw != 3 || !in->joint_q || !out->joint_tau))
    return fail(QC_ERR_INVALID, "qc_control_batch: swing_pos, swing_vel and joint_qdot go together and need joint_q and joint_tau");
  if (in->gait_dt && (!in->gait_phase || in->stance)) return fail(QC_ERR_INVALID, "qc_control_batch: gait_dt advances gait_phase (needed, and stance must be NULL)");
  if (in->swing_state && (!in->joint_q || !in->joint_qdot || !in->gait_phase || !out->joint_tau || in->swing_pos || in->swing_vel))
    return fail(QC_ERR_INVALID, "qc_control_batch: swing_state needs joint_q, joint_qdot, gait_phase and joint_tau, and excludes swing_pos/swing_vel");
  return QC_OK;
}

// qc_tick_batch
inline int check_tick_args(const qc_handle* h, const qc_batch_in* in, const qc_command_in* cmd, const qc_batch_out* out) {
  if (const int rc = check_io("qc_tick_batch", h && in && out, cmd, "qc_command_in", "qc_default_command"); rc != QC_OK) return rc;
  if (!in->Rwb || !in->x || !in->xdot || !in->w || !in->joint_q || !in->joint_qdot || !in->gait_phase || !in->gait_dt || !in->swing_state)
    return fail(QC_ERR_INVALID, "qc_tick_batch: the complete tick needs Rwb, x, xdot, w, joint_q, joint_qdot, gait_phase, gait_dt and swing_state");
  if (in->Rwb_d || in->x_d || in->xdot_d || in->w_d)
    return fail(QC_ERR_INVALID, "qc_tick_batch: Rwb_d, x_d, xdot_d and w_d must be NULL (the desired state lives in qc_command_in.state)");
  if (in->stance || in->swing_pos || in->swing_vel)
    return fail(QC_ERR_INVALID, "qc_tick_batch: stance, swing_pos and swing_vel must be NULL (the gait clock and the planner make them)");
  if (!out->grf_body || !out->status || !out->joint_tau) return fail(QC_ERR_INVALID, "qc_tick_batch: grf_body, status and joint_tau are required");
  if (!cmd->state) return fail(QC_ERR_INVALID, "qc_tick_batch: qc_command_in.state is required");
  if (cmd->fresh && !cmd->twist) return fail(QC_ERR_INVALID, "qc_tick_batch: qc_command_in.fresh needs twist");
  if (!std::isfinite(cmd->stand_height) || !(cmd->stand_tol >= 0.0) || !std::isfinite(cmd->stand_tol) || !std::isfinite(cmd->cmd_dt))
    return fail(QC_ERR_INVALID, "qc_tick_batch: stand_height, stand_tol (>= 0) and cmd_dt must be finite");
  return QC_OK;
}

// ---------------------------------------------------------------- qc_plant_step_batch
// Ib^-1 for the plant step.  qc_create reads Ib only through the wrench law, which needs nothing of it, and keeps accepting what it
// always has; a rigid body that is to be integrated needs a finite, symmetric positive definite inertia, so the plant refuses the rest.
inline int plant_inertia_inverse(const double* Ib, double* Ib_inv, const char* who = "qc_plant_step_batch") {
  const auto bad = [who](const char* what) { return fail(QC_ERR_INVALID, std::string(who) + what); };
  for (int i = 0; i < 9; i++)
    if (!std::isfinite(Ib[i])) return bad(": the handle's Ib is not finite");
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < i; j++)
      if (std::fabs(Ib[3 * i + j] - Ib[3 * j + i]) > 1e-12 * (std::fabs(Ib[3 * i + i]) + std::fabs(Ib[3 * j + j]))) return bad(": the handle's Ib is not symmetric");
  if (!spd_inverse(Ib, 3, Ib_inv)) return bad(": the handle's Ib is not positive definite");
  for (int i = 0; i < 9; i++)  // (an Ib whose entries are finite but whose inverse overflows)
    if (!std::isfinite(Ib_inv[i])) return bad(": the handle's Ib is not positive definite");
  return QC_OK;
}

// the body's constants of both plant kernels from the handle's mass and Ib and the call's dt, refused under the entry point's name
inline int body_constants(const char* who, double mass, const double* Ib, double dt, BodyConst& b) {
  if (!std::isfinite(mass) || !(mass > 0.0)) return fail(QC_ERR_INVALID, std::string(who) + ": the handle's mass is not finite and > 0");
  if (const int rc = plant_inertia_inverse(Ib, b.Ib_inv, who); rc != QC_OK) return rc;
  b.mass = mass;
  std::memcpy(b.Ib, Ib, sizeof(b.Ib));
  b.g = PLANT_G;
  b.dt = dt;
  return QC_OK;
}
inline int plant_constants(double mass, const double* Ib, double dt, PlantArgs& a) { return body_constants("qc_plant_step_batch", mass, Ib, dt, a); }
// the kernel's arguments: the body's constants and the call's arrays
inline int plant_constants(double mass, const double* Ib, const qc_plant_io* io, PlantArgs& a) {
  if (const int rc = plant_constants(mass, Ib, io->dt, a); rc != QC_OK) return rc;
  a.Rwb = io->Rwb; a.x = io->x; a.xdot = io->xdot; a.w = io->w; a.grf_body = io->grf_body; a.foot_world = io->foot_world; a.feet = io->feet;
  return QC_OK;
}

// What the three plant-type calls refuse after check_io, in this order: dt; `own`, the call's first refusal about its other scalars
// and optional arrays (nullptr: none); for n > 0 the state arrays, the call's other required arrays (`others`) and the launch bound.
template <class Io>
int check_plant_io(const char* who, size_t n, const Io* io, const char* own, bool others, const char* others_msg, int block) {
  const auto bad = [who](const char* what) { return fail(QC_ERR_INVALID, std::string(who) + what); };
  if (!std::isfinite(io->dt) || !(io->dt > 0.0)) return bad(": dt must be finite and > 0");
  if (own) return bad(own);
  if (n == 0) return QC_OK;
  if (!io->Rwb || !io->x || !io->xdot || !io->w) return bad(": the state arrays Rwb, x, xdot and w are required");
  if (!others) return bad(others_msg);
  return check_one_launch(who, n, block);
}

inline int check_plant_args(const qc_handle* h, size_t n, const qc_plant_io* io) {
  const char* who = "qc_plant_step_batch";
  if (const int rc = check_io(who, h != nullptr, io, "qc_plant_io", "qc_default_plant"); rc != QC_OK) return rc;
  return check_plant_io(who, n, io, nullptr, io->grf_body && io->foot_world, ": grf_body and foot_world are required", PLANT_BLOCK);
}

// ---------------------------------------------------------------- qc_plant_step_adjoint_batch
// What is wrong with the call itself; the handle's mass and Ib are judged by plant_adjoint_constants, through the plant's own checks.
inline int check_plant_adjoint_args(const qc_handle* h, size_t n, const qc_plant_adjoint_io* io) {
  const char* who = "qc_plant_step_adjoint_batch";
  if (const int rc = check_io(who, h != nullptr, io, "qc_plant_adjoint_io", "qc_default_plant_adjoint"); rc != QC_OK) return rc;
  const char* own = nullptr;
  if (!io->Rwb_next_bar && !io->x_next_bar && !io->xdot_next_bar && !io->w_next_bar && !io->feet_next_bar)
    own = ": no input cotangent given (Rwb_next_bar, x_next_bar, xdot_next_bar, w_next_bar, feet_next_bar are all NULL)";
  else if (!io->Rwb_bar && !io->x_bar && !io->xdot_bar && !io->w_bar && !io->grf_bar && !io->foot_world_bar)
    own = ": no output requested (Rwb_bar, x_bar, xdot_bar, w_bar, grf_bar, foot_world_bar are all NULL)";
  return check_plant_io(who, n, io, own, io->grf_body && io->foot_world, ": grf_body and foot_world are required", PLANT_BLOCK);
}

// the kernel's arguments: the body's constants (body_constants, under this entry point's name) and the call's arrays
inline int plant_adjoint_constants(double mass, const double* Ib, const qc_plant_adjoint_io* io, PlantAdjointArgs& a) {
  if (const int rc = body_constants("qc_plant_step_adjoint_batch", mass, Ib, io->dt, a); rc != QC_OK) return rc;
  a.Rwb = io->Rwb; a.x = io->x; a.xdot = io->xdot; a.w = io->w; a.grf_body = io->grf_body; a.foot_world = io->foot_world;
  a.Rwb_next_bar = io->Rwb_next_bar; a.x_next_bar = io->x_next_bar; a.xdot_next_bar = io->xdot_next_bar; a.w_next_bar = io->w_next_bar;
  a.feet_next_bar = io->feet_next_bar;
  a.Rwb_bar = io->Rwb_bar; a.x_bar = io->x_bar; a.xdot_bar = io->xdot_bar; a.w_bar = io->w_bar; a.grf_bar = io->grf_bar; a.foot_world_bar = io->foot_world_bar;
  return QC_OK;
}

// ---------------------------------------------------------------- qc_leg_plant_step_batch
// What is wrong with the call itself; the handle's mass and Ib are judged by leg_plant_constants, through the plant's own checks.
inline int check_leg_plant_args(const qc_handle* h, size_t n, const qc_leg_plant_io* io) {
  const char* who = "qc_leg_plant_step_batch";
  if (const int rc = check_io(who, h != nullptr, io, "qc_leg_plant_io", "qc_default_leg_plant"); rc != QC_OK) return rc;
  const char* own = nullptr;
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(io->leg_inertia[k]) || !(io->leg_inertia[k] > 0.0))
      own = ": leg_inertia (hip, thigh, calf) must be finite and > 0; qc_default_leg_plant leaves it at 0, the caller gives it";
  return check_plant_io(who, n, io, own, io->joint_q && io->joint_qdot && io->joint_tau, ": joint_q, joint_qdot and joint_tau are required", LEG_PLANT_BLOCK);
}

// What LegPlantArgs and LegPlantAdjointArgs share: the body's constants (body_constants, under the entry point's name), the call's leg
// inertia, the state, the torques and the contact inputs.
template <class Io, class Args>
int leg_plant_shared(const char* who, double mass, const double* Ib, const Io* io, Args& a) {
  if (const int rc = body_constants(who, mass, Ib, io->dt, a); rc != QC_OK) return rc;
  for (int k = 0; k < 3; k++) a.leg_inertia[k] = io->leg_inertia[k];
  a.Rwb = io->Rwb; a.x = io->x; a.xdot = io->xdot; a.w = io->w; a.joint_q = io->joint_q; a.joint_qdot = io->joint_qdot; a.joint_tau = io->joint_tau;
  a.stance = io->stance; a.gait_phase = io->gait_phase; a.gait_duty = io->gait_duty; a.cmd_state = reinterpret_cast<const CmdState*>(io->cmd_state);
  return QC_OK;
}

// the kernel's arguments: what the two leg-plant calls share (leg_plant_shared) and the step's two outputs
inline int leg_plant_constants(double mass, const double* Ib, const qc_leg_plant_io* io, LegPlantArgs& a) {
  if (const int rc = leg_plant_shared("qc_leg_plant_step_batch", mass, Ib, io, a); rc != QC_OK) return rc;
  a.foot_world = io->foot_world; a.flags = io->flags;
  return QC_OK;
}

// ---------------------------------------------------------------- qc_leg_plant_step_adjoint_batch
// What is wrong with the call itself; the handle's mass and Ib are judged by leg_plant_adjoint_constants, through the plant's own checks.
inline int check_leg_plant_adjoint_args(const qc_handle* h, size_t n, const qc_leg_plant_adjoint_io* io) {
  const char* who = "qc_leg_plant_step_adjoint_batch";
  if (const int rc = check_io(who, h != nullptr, io, "qc_leg_plant_adjoint_io", "qc_default_leg_plant_adjoint"); rc != QC_OK) return rc;
  const char* own = nullptr;
  if (!io->Rwb_next_bar && !io->x_next_bar && !io->xdot_next_bar && !io->w_next_bar && !io->joint_q_next_bar && !io->joint_qdot_next_bar)
    own = ": no input cotangent given (Rwb_next_bar, x_next_bar, xdot_next_bar, w_next_bar, joint_q_next_bar, joint_qdot_next_bar are all NULL)";
  else if (!io->Rwb_bar && !io->x_bar && !io->xdot_bar && !io->w_bar && !io->joint_q_bar && !io->joint_qdot_bar && !io->joint_tau_bar && !io->flags)
    own = ": no output requested (Rwb_bar, x_bar, xdot_bar, w_bar, joint_q_bar, joint_qdot_bar, joint_tau_bar, flags are all NULL)";
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(io->leg_inertia[k]) || !(io->leg_inertia[k] > 0.0))
      own = ": leg_inertia (hip, thigh, calf) must be finite and > 0; qc_default_leg_plant_adjoint leaves it at 0, the caller gives the step's";
  return check_plant_io(who, n, io, own, io->joint_q && io->joint_qdot && io->joint_tau, ": joint_q, joint_qdot and joint_tau are required", LEG_PLANT_BLOCK);
}

// the kernel's arguments: what the two leg-plant calls share (leg_plant_shared), the cotangents and the outputs
inline int leg_plant_adjoint_constants(double mass, const double* Ib, const qc_leg_plant_adjoint_io* io, LegPlantAdjointArgs& a) {
  if (const int rc = leg_plant_shared("qc_leg_plant_step_adjoint_batch", mass, Ib, io, a); rc != QC_OK) return rc;
  a.Rwb_next_bar = io->Rwb_next_bar; a.x_next_bar = io->x_next_bar; a.xdot_next_bar = io->xdot_next_bar; a.w_next_bar = io->w_next_bar;
  a.joint_q_next_bar = io->joint_q_next_bar; a.joint_qdot_next_bar = io->joint_qdot_next_bar;
  a.Rwb_bar = io->Rwb_bar; a.x_bar = io->x_bar; a.xdot_bar = io->xdot_bar; a.w_bar = io->w_bar;
  a.joint_q_bar = io->joint_q_bar; a.joint_qdot_bar = io->joint_qdot_bar; a.joint_tau_bar = io->joint_tau_bar; a.flags = io->flags;
  return QC_OK;
}

// ---------------------------------------------------------------- qc_certify_batch, qc_sensitivity_batch, qc_sensitivity_rot_batch, qc_sensitivity_param_batch
// What the four calls that only read a solved batch refuse after check_io, in this order: `own`, the call's first refusal about its
// scalars and outputs (nullptr: none); for n > 0 the call's input arrays (`inputs`), the state, feet or joint_q and the launch bound.
inline int check_readonly_batch(const char* who, size_t n, const qc_batch_in* in, const char* own, bool inputs, const char* inputs_msg, int block) {
  const auto bad = [who](const char* what) { return fail(QC_ERR_INVALID, std::string(who) + what); };
  if (own) return bad(own);
  if (n == 0) return QC_OK;
  if (!inputs) return bad(inputs_msg);
  if (!in->Rwb || !in->Rwb_d || !in->x || !in->xdot || !in->w || !in->x_d || !in->xdot_d || !in->w_d)
    return bad(": the state arrays Rwb, Rwb_d, x, xdot, w, x_d, xdot_d and w_d are required (commander mode is out of scope)");
  if (!in->feet && !in->joint_q) return bad(": feet or joint_q is required");
  return check_one_launch(who, n, block);
}

// The argument check of the certificate: what is wrong with the call itself (message prefix "qc_certify_batch:").
inline int check_certify_args(const qc_handle* h, size_t n, const qc_batch_in* in, const qc_certify_io* io) {
  const char* who = "qc_certify_batch";
  if (const int rc = check_io(who, h && in, io, "qc_certify_io", "qc_default_certify"); rc != QC_OK) return rc;
  const auto tol_ok = [](double t) { return std::isfinite(t) && t >= 0.0; };
  const char* own = nullptr;
  if (!tol_ok(io->act_tol) || !tol_ok(io->primal_tol) || !tol_ok(io->stat_tol)) own = ": act_tol, primal_tol and stat_tol must be finite and >= 0";
  else if (!io->primal && !io->stationarity && !io->lambda && !io->grad && !io->active && !io->flags && !io->summary)
    own = ": no output requested (primal, stationarity, lambda, grad, active, flags, summary are all NULL)";
  return check_readonly_batch(who, n, in, own, io->grf_body != nullptr, ": grf_body is required", CERTIFY_BLOCK);
}

// workgroups of certify_kernel for n robots: one wave each, capped at the handle's partial buffer
inline unsigned certify_blocks(size_t n) { return capped_blocks(n, CERTIFY_BLOCK, CERTIFY_MAX_PARTIALS); }

// The argument check of the adjoint: what is wrong with the call itself (message prefix "qc_sensitivity_batch:").
inline int check_sensitivity_args(const qc_handle* h, size_t n, const qc_batch_in* in, const qc_sensitivity_io* io) {
  const char* who = "qc_sensitivity_batch";
  if (const int rc = check_io(who, h && in, io, "qc_sensitivity_io", "qc_default_sensitivity"); rc != QC_OK) return rc;
  const char* own = nullptr;
  if (!std::isfinite(io->act_tol) || !(io->act_tol >= 0.0)) own = ": act_tol must be finite and >= 0";
  else if (!io->adjoint && !io->b_bar && !io->feet_bar && !io->x_bar && !io->xdot_bar && !io->w_bar && !io->x_d_bar && !io->xdot_d_bar && !io->w_d_bar && !io->flags)
    own = ": no output requested (adjoint, b_bar, feet_bar, x_bar, xdot_bar, w_bar, x_d_bar, xdot_d_bar, w_d_bar, flags are all NULL)";
  return check_readonly_batch(who, n, in, own, io->grf_body && io->grf_bar, ": grf_body and grf_bar are required", SENSITIVITY_BLOCK);
}

// workgroups of sensitivity_kernel and sensitivity_rot_kernel for n robots: one wave each, capped
inline unsigned sensitivity_blocks(size_t n) { return capped_blocks(n, SENSITIVITY_BLOCK, SENSITIVITY_MAX_BLOCKS); }

// The argument check of the rotation cotangents: what is wrong with the call itself (message prefix "qc_sensitivity_rot_batch:").
inline int check_sensitivity_rot_args(const qc_handle* h, size_t n, const qc_batch_in* in, const qc_sensitivity_rot_io* io) {
  const char* who = "qc_sensitivity_rot_batch";
  if (const int rc = check_io(who, h && in, io, "qc_sensitivity_rot_io", "qc_default_sensitivity_rot"); rc != QC_OK) return rc;
  const bool no_out = !io->Rwb_bar && !io->Rwb_d_bar && !io->Rwb_rot_bar && !io->Rwb_d_rot_bar;
  const char* own = no_out ? ": no output requested (Rwb_bar, Rwb_d_bar, Rwb_rot_bar, Rwb_d_rot_bar are all NULL)" : nullptr;
  return check_readonly_batch(who, n, in, own, io->grf_body && io->grf_bar && io->b_bar && io->feet_bar, ": grf_body, grf_bar, b_bar and feet_bar are required", SENSITIVITY_BLOCK);
}

// The argument check of the parameter cotangents: what is wrong with the call itself (message prefix "qc_sensitivity_param_batch:").
inline int check_sensitivity_param_args(const qc_handle* h, size_t n, const qc_batch_in* in, const qc_sensitivity_param_io* io) {
  const char* who = "qc_sensitivity_param_batch";
  if (const int rc = check_io(who, h && in, io, "qc_sensitivity_param_io", "qc_default_sensitivity_param"); rc != QC_OK) return rc;
  const char* own = nullptr;
  if (!std::isfinite(io->act_tol) || !(io->act_tol >= 0.0)) own = ": act_tol must be finite and >= 0";
  else if (!io->param_bar_rows && !io->param_bar) own = ": no output requested (param_bar_rows and param_bar are both NULL)";
  return check_readonly_batch(who, n, in, own, io->grf_body && io->grf_bar && io->adjoint, ": grf_body, grf_bar and adjoint are required", SENSITIVITY_PARAM_BLOCK);
}

// workgroups of sensitivity_param_kernel for n robots: one wave each, capped at the handle's partial buffer
inline unsigned sensitivity_param_blocks(size_t n) { return capped_blocks(n, SENSITIVITY_PARAM_BLOCK, SENSITIVITY_PARAM_MAX_BLOCKS); }

// ---------------------------------------------------------------- qc_sensitivity_kin_batch
// The argument check of the joint-angle cotangents: what is wrong with the call itself (message prefix "qc_sensitivity_kin_batch:").
// The kernel reads joint_q and the contact mask of `in` and none of the state arrays: they are not asked for.
inline int check_sensitivity_kin_args(const qc_handle* h, size_t n, const qc_batch_in* in, const qc_sensitivity_kin_io* io) {
  const char* who = "qc_sensitivity_kin_batch";
  if (const int rc = check_io(who, h && in, io, "qc_sensitivity_kin_io", "qc_default_sensitivity_kin"); rc != QC_OK) return rc;
  const auto bad = [who](const char* what) { return fail(QC_ERR_INVALID, std::string(who) + what); };
  if (!io->grf_bar && !io->joint_q_bar) return bad(": no output requested (grf_bar and joint_q_bar are both NULL)");
  if (!io->joint_tau_bar && !io->feet_bar && !io->joint_q_bar_in) return bad(": no cotangent given (joint_tau_bar, feet_bar and joint_q_bar_in are all NULL)");
  if (io->joint_tau_bar && (!io->grf_body || !io->status)) return bad(": joint_tau_bar needs grf_body and status");
  if (io->grf_bar && !io->joint_tau_bar) return bad(": grf_bar needs joint_tau_bar");
  if (n == 0) return QC_OK;
  if (!in->joint_q) return bad(": joint_q is required");
  return check_one_launch(who, n, SENSITIVITY_BLOCK);
}

// workgroups of sensitivity_kin_kernel for n robots: one wave of 16 robots' legs each, capped
inline unsigned sensitivity_kin_blocks(size_t n) { return capped_blocks(4 * n, SENSITIVITY_BLOCK, SENSITIVITY_MAX_BLOCKS); }

// ---------------------------------------------------------------- qc_sensitivity_swing_batch
// The argument check of the swing-leg torque adjoint: what is wrong with the call itself (message prefix "qc_sensitivity_swing_batch:").
// The kernel reads six arrays of `in` and the contact mask as it is now; what would plan or advance (swing_state, gait_dt) is refused.
inline int check_sensitivity_swing_args(const qc_handle* h, size_t n, const qc_batch_in* in, const qc_sensitivity_swing_io* io) {
  const char* who = "qc_sensitivity_swing_batch";
  if (const int rc = check_io(who, h && in, io, "qc_sensitivity_swing_io", "qc_default_sensitivity_swing"); rc != QC_OK) return rc;
  const auto bad = [who](const char* what) { return fail(QC_ERR_INVALID, std::string(who) + what); };
  if (in->swing_state) return bad(": swing_state must be NULL (the planner's references are out of scope: give swing_pos and swing_vel)");
  if (in->gait_dt) return bad(": gait_dt must be NULL (the gait clock is out of scope: the contact mask is read as it is now)");
  if (!io->swing_pos_bar && !io->swing_vel_bar && !io->joint_q_bar && !io->joint_qdot_bar && !io->gain_bar && !io->Rwb_bar && !io->x_bar && !io->flags)
    return bad(": no output requested (swing_pos_bar, swing_vel_bar, joint_q_bar, joint_qdot_bar, gain_bar, Rwb_bar, x_bar, flags are all NULL)");
  if (n == 0) return QC_OK;
  if (!io->joint_tau_bar) return bad(": joint_tau_bar is required");
  if (!in->Rwb || !in->x || !in->joint_q || !in->joint_qdot || !in->swing_pos || !in->swing_vel)
    return bad(": Rwb, x, joint_q, joint_qdot, swing_pos and swing_vel are required");
  return check_one_launch(who, n, SENSITIVITY_BLOCK);
}

// workgroups of sensitivity_swing_kernel for n robots: one wave of 16 robots' legs each, capped
inline unsigned sensitivity_swing_blocks(size_t n) { return capped_blocks(4 * n, SENSITIVITY_BLOCK, SENSITIVITY_MAX_BLOCKS); }

// ---------------------------------------------------------------- qc_swing_reference_batch, qc_swing_reference_adjoint_batch
// What the two calls refuse about `in` before their own arrays, in this order: references that are already there, feet in place of
// joint_q (as the tick refuses them for a batch with swing_state).
inline int check_swing_reference_batch(const char* who, const qc_batch_in* in) {
  const auto bad = [who](const char* what) { return fail(QC_ERR_INVALID, std::string(who) + what); };
  if (in->swing_pos || in->swing_vel) return bad(": swing_pos and swing_vel must be NULL (this call makes them)");
  if (in->feet && !in->joint_q) return bad(": feet without joint_q (the planner starts from the forward kinematics of joint_q)");
  return QC_OK;
}

// The argument check of the swing references: what is wrong with the call itself (message prefix "qc_swing_reference_batch:").
inline int check_swing_reference_args(const qc_handle* h, size_t n, const qc_batch_in* in, const qc_swing_reference_io* io) {
  const char* who = "qc_swing_reference_batch";
  if (const int rc = check_io(who, h && in, io, "qc_swing_reference_io", "qc_default_swing_reference"); rc != QC_OK) return rc;
  const auto bad = [who](const char* what) { return fail(QC_ERR_INVALID, std::string(who) + what); };
  if (const int rc = check_swing_reference_batch(who, in); rc != QC_OK) return rc;
  if (in->gait_dt && in->stance) return bad(": gait_dt advances gait_phase (stance must be NULL)");
  if (!io->swing_pos && !io->swing_vel && !io->planned) return bad(": no output requested (swing_pos, swing_vel, planned are all NULL)");
  if (n == 0) return QC_OK;
  if (!in->Rwb || !in->x || !in->xdot || !in->w || !in->xdot_d || !in->joint_q || !in->gait_phase || !in->swing_state)
    return bad(": Rwb, x, xdot, w, xdot_d, joint_q, gait_phase and swing_state are required");
  return check_one_launch(who, n, SENSITIVITY_BLOCK);
}

// The argument check of their reverse pass (message prefix "qc_swing_reference_adjoint_batch:").
inline int check_swing_reference_adjoint_args(const qc_handle* h, size_t n, const qc_batch_in* in, const qc_swing_reference_adjoint_io* io) {
  const char* who = "qc_swing_reference_adjoint_batch";
  if (const int rc = check_io(who, h && in, io, "qc_swing_reference_adjoint_io", "qc_default_swing_reference_adjoint"); rc != QC_OK) return rc;
  const auto bad = [who](const char* what) { return fail(QC_ERR_INVALID, std::string(who) + what); };
  if (const int rc = check_swing_reference_batch(who, in); rc != QC_OK) return rc;
  if (in->gait_dt) return bad(": gait_dt must be NULL (the reverse pass advances no clock: gait_phase is read as the forward call left it)");
  if (!io->swing_pos_bar && !io->swing_vel_bar && !io->p_start_next_bar && !io->p_final_next_bar)
    return bad(": no cotangent given (swing_pos_bar, swing_vel_bar, p_start_next_bar, p_final_next_bar are all NULL)");
  if (!io->Rwb_bar && !io->x_bar && !io->xdot_bar && !io->w_bar && !io->xdot_d_bar && !io->joint_q_bar && !io->p_start_bar && !io->p_final_bar && !io->flags)
    return bad(": no output requested (Rwb_bar, x_bar, xdot_bar, w_bar, xdot_d_bar, joint_q_bar, p_start_bar, p_final_bar, flags are all NULL)");
  if (n == 0) return QC_OK;
  if (!io->state_before) return bad(": state_before is required (the swing records from before the forward call)");
  if (!in->Rwb || !in->x || !in->xdot || !in->w || !in->joint_q || !in->gait_phase) return bad(": Rwb, x, xdot, w, joint_q and gait_phase are required");
  return check_one_launch(who, n, SENSITIVITY_BLOCK);
}

// workgroups of the two kernels for n robots: one wave each, capped
inline unsigned swing_reference_blocks(size_t n) { return capped_blocks(n, SENSITIVITY_BLOCK, SENSITIVITY_MAX_BLOCKS); }

// ---------------------------------------------------------------- qc_commander_step_batch, qc_commander_step_adjoint_batch
// What the two calls refuse about `cmd` and the scalars after their own outputs (`own`: the call's first refusal about its arrays,
// nullptr: none; `state`: the records the call reads - cmd->state or io->state_before - and what it calls them), as qc_tick_batch does.
inline int check_commander_step_batch(const char* who, size_t n, const qc_batch_in* in, const qc_command_in* cmd, const char* own, bool state, const char* state_msg) {
  const auto bad = [who](const char* what) { return fail(QC_ERR_INVALID, std::string(who) + what); };
  if (own) return bad(own);
  if (cmd->fresh && !cmd->twist) return bad(": qc_command_in.fresh needs twist");
  if (!std::isfinite(cmd->stand_height) || !(cmd->stand_tol >= 0.0) || !std::isfinite(cmd->stand_tol) || !std::isfinite(cmd->cmd_dt))
    return bad(": stand_height, stand_tol (>= 0) and cmd_dt must be finite");
  if (n == 0) return QC_OK;
  if (!state) return bad(state_msg);
  if (!in->Rwb || !in->x) return bad(": Rwb and x are required");
  return check_one_launch(who, n, SENSITIVITY_BLOCK);
}

// The argument check of the commander step: what is wrong with the call itself (message prefix "qc_commander_step_batch:").
inline int check_commander_step_args(const qc_handle* h, size_t n, const qc_batch_in* in, const qc_command_in* cmd, const qc_commander_step_io* io) {
  const char* who = "qc_commander_step_batch";
  if (const int rc = check_io(who, h && in && io, cmd, "qc_command_in", "qc_default_command"); rc != QC_OK) return rc;
  if (const int rc = check_io(who, true, io, "qc_commander_step_io", "qc_default_commander_step"); rc != QC_OK) return rc;
  return check_commander_step_batch(who, n, in, cmd, nullptr, cmd->state != nullptr, ": qc_command_in.state is required");
}

// The argument check of its reverse pass (message prefix "qc_commander_step_adjoint_batch:").
inline int check_commander_step_adjoint_args(const qc_handle* h, size_t n, const qc_batch_in* in, const qc_command_in* cmd, const qc_commander_step_adjoint_io* io) {
  const char* who = "qc_commander_step_adjoint_batch";
  if (const int rc = check_io(who, h && in && io, cmd, "qc_command_in", "qc_default_command"); rc != QC_OK) return rc;
  if (const int rc = check_io(who, true, io, "qc_commander_step_adjoint_io", "qc_default_commander_step_adjoint"); rc != QC_OK) return rc;
  const char* own = nullptr;
  if (!io->Rwb_d_bar && !io->x_d_bar && !io->xdot_d_bar && !io->w_d_bar && !io->Vb_next_bar)
    own = ": no cotangent given (Rwb_d_bar, x_d_bar, xdot_d_bar, w_d_bar, Vb_next_bar are all NULL)";
  else if (!io->twist_bar && !io->Vb_bar && !io->Rwb_bar && !io->x_bar && !io->Rwb_d_prev_bar && !io->x_d_prev_bar && !io->xdot_d_prev_bar && !io->w_d_prev_bar && !io->flags)
    own = ": no output requested (twist_bar, Vb_bar, Rwb_bar, x_bar, Rwb_d_prev_bar, x_d_prev_bar, xdot_d_prev_bar, w_d_prev_bar, flags are all NULL)";
  return check_commander_step_batch(who, n, in, cmd, own, io->state_before != nullptr, ": state_before is required (the commander records from before the forward call)");
}

// workgroups of the two kernels for n robots: one wave each, capped
inline unsigned commander_step_blocks(size_t n) { return capped_blocks(n, SENSITIVITY_BLOCK, SENSITIVITY_MAX_BLOCKS); }

// ---------------------------------------------------------------- qc_support_polygon_batch, qc_support_polygon_adjoint_batch
// What the two calls refuse after check_io, in this order: what would advance, plan or track (`in`); `own`, the call's first refusal
// about its outputs and cotangent (nullptr: none); for n > 0 the schedule, the phases, the feet, the pose of world mode and the
// launch bound.
inline int check_support_polygon_batch(const char* who, size_t n, const qc_batch_in* in, const char* own, const double* schedule, bool world) {
  const auto bad = [who](const char* what) { return fail(QC_ERR_INVALID, std::string(who) + what); };
  if (in->gait_dt) return bad(": gait_dt must be NULL (no clock is advanced: gait_phase is read as it is now)");
  if (in->swing_state) return bad(": swing_state must be NULL (nothing is planned here)");
  if (in->swing_pos || in->swing_vel) return bad(": swing_pos and swing_vel must be NULL (the polygon reads the feet, not the swing references)");
  if (own) return bad(own);
  if (n == 0) return QC_OK;
  if (!schedule) return bad(": schedule is required (the widths of the ramps, [n][4][4] or one shared [4][4])");
  if (!in->gait_phase) return bad(": gait_phase is required");
  if (!in->feet && !in->joint_q) return bad(": feet or joint_q is required");
  if (world && (!in->Rwb || !in->x)) return bad(": world needs Rwb and x");
  return check_one_launch(who, n, SENSITIVITY_BLOCK);
}

// The argument check of the support polygon: what is wrong with the call itself (message prefix "qc_support_polygon_batch:").
inline int check_support_polygon_args(const qc_handle* h, size_t n, const qc_batch_in* in, const qc_support_polygon_io* io) {
  const char* who = "qc_support_polygon_batch";
  if (const int rc = check_io(who, h && in, io, "qc_support_polygon_io", "qc_default_support_polygon"); rc != QC_OK) return rc;
  const char* own = !io->com_xy && !io->weights && !io->flags ? ": no output requested (com_xy, weights, flags are all NULL)" : nullptr;
  return check_support_polygon_batch(who, n, in, own, io->schedule, io->world != 0);
}

// The argument check of its reverse pass (message prefix "qc_support_polygon_adjoint_batch:").
inline int check_support_polygon_adjoint_args(const qc_handle* h, size_t n, const qc_batch_in* in, const qc_support_polygon_adjoint_io* io) {
  const char* who = "qc_support_polygon_adjoint_batch";
  if (const int rc = check_io(who, h && in, io, "qc_support_polygon_adjoint_io", "qc_default_support_polygon_adjoint"); rc != QC_OK) return rc;
  const char* own = nullptr;
  if (!io->feet_bar && !io->Rwb_bar && !io->x_bar && !io->phase_bar && !io->schedule_bar && !io->flags)
    own = ": no output requested (feet_bar, Rwb_bar, x_bar, phase_bar, schedule_bar, flags are all NULL)";
  else if (n > 0 && !io->com_xy_bar)
    own = ": com_xy_bar is required";
  return check_support_polygon_batch(who, n, in, own, io->schedule, io->world != 0);
}

// workgroups of the two kernels for n robots: one wave each, capped
inline unsigned support_polygon_blocks(size_t n) { return capped_blocks(n, SENSITIVITY_BLOCK, SENSITIVITY_MAX_BLOCKS); }

// ---------------------------------------------------------------- qc_com_reference_batch, qc_com_reference_adjoint_batch
// The polygon's refusals (always world mode: Rwb and x are required), behind the call's own about its mode, gain and arrays.
inline int check_com_reference_batch(const char* who, size_t n, const qc_batch_in* in, const char* own, const double* schedule) {
  if (const int rc = check_support_polygon_batch(who, n, in, own, schedule, false); rc != QC_OK || n == 0) return rc;
  if (!in->Rwb || !in->x) return fail(QC_ERR_INVALID, std::string(who) + ": Rwb and x are required (the polygon is that of Rwb p + x)");
  return QC_OK;
}
inline const char* check_com_mode(int32_t mode, double gain) {
  if (mode != COM_REPLACE && mode != COM_OFFSET) return ": mode must be QC_COM_REPLACE or QC_COM_OFFSET";
  if (!std::isfinite(gain)) return ": gain must be finite";
  return nullptr;
}

// The argument check of the COM reference: what is wrong with the call itself (message prefix "qc_com_reference_batch:").
inline int check_com_reference_args(const qc_handle* h, size_t n, const qc_batch_in* in, const qc_com_reference_io* io) {
  const char* who = "qc_com_reference_batch";
  if (const int rc = check_io(who, h && in, io, "qc_com_reference_io", "qc_default_com_reference"); rc != QC_OK) return rc;
  const char* own = check_com_mode(io->mode, io->gain);
  if (!own && !io->x_d_out) own = ": x_d_out is required";
  if (!own && n > 0 && !io->x_d_in) own = ": x_d_in is required";
  return check_com_reference_batch(who, n, in, own, io->schedule);
}

// The argument check of its reverse pass (message prefix "qc_com_reference_adjoint_batch:").
inline int check_com_reference_adjoint_args(const qc_handle* h, size_t n, const qc_batch_in* in, const qc_com_reference_adjoint_io* io) {
  const char* who = "qc_com_reference_adjoint_batch";
  if (const int rc = check_io(who, h && in, io, "qc_com_reference_adjoint_io", "qc_default_com_reference_adjoint"); rc != QC_OK) return rc;
  const char* own = check_com_mode(io->mode, io->gain);
  if (!own && !io->x_d_in_bar && !io->feet_bar && !io->Rwb_bar && !io->x_bar && !io->phase_bar && !io->schedule_bar && !io->schedule_bar_sum && !io->flags)
    own = ": no output requested (x_d_in_bar, feet_bar, Rwb_bar, x_bar, phase_bar, schedule_bar, schedule_bar_sum, flags are all NULL)";
  if (!own && n > 0 && !io->x_d_out_bar) own = ": x_d_out_bar is required";
  return check_com_reference_batch(who, n, in, own, io->schedule);
}

// what the polygon and COM kernels read of the batch (SupportIn): the feet, the phases and the contact mask as it is now, the pose in
// world mode, the schedule - nothing of `in` is written
inline SupportIn support_in(const qc_batch_in* in, const double* schedule, int32_t schedule_shared, bool world) {
  return SupportIn{in->feet, in->joint_q, in->gait_phase, in->stance, in->gait_duty, world ? in->Rwb : nullptr, world ? in->x : nullptr, schedule,
                   schedule_shared != 0};
}

// workgroups of the kernels for n robots: one wave each, capped - the reverse pass that sums at the partials of the handle's buffer
inline unsigned com_reference_blocks(size_t n, bool sum) { return capped_blocks(n, SENSITIVITY_BLOCK, sum ? COM_SUM_MAX_BLOCKS : SENSITIVITY_MAX_BLOCKS); }

// ---------------------------------------------------------------- qc_tangent_batch
// The argument check of the forward mode: what is wrong with the call itself (message prefix "qc_tangent_batch:").
inline int check_tangent_args(const qc_handle* h, size_t n, const qc_batch_in* in, const qc_tangent_io* io) {
  const char* who = "qc_tangent_batch";
  if (const int rc = check_io(who, h && in, io, "qc_tangent_io", "qc_default_tangent"); rc != QC_OK) return rc;
  const char* own = nullptr;
  if (!std::isfinite(io->act_tol) || !(io->act_tol >= 0.0)) own = ": act_tol must be finite and >= 0";
  else if (io->n_dir == 0) own = ": n_dir must be >= 1";
  else if (!io->grf_tan && !io->b_tan) own = ": no output requested (grf_tan and b_tan are both NULL)";
  else if (!io->x_tan && !io->xdot_tan && !io->w_tan && !io->x_d_tan && !io->xdot_d_tan && !io->w_d_tan && !io->Rwb_rot_tan && !io->Rwb_d_rot_tan &&
           !io->feet_tan && !io->joint_q_tan)
    own = ": no tangent given (x_tan, xdot_tan, w_tan, x_d_tan, xdot_d_tan, w_d_tan, Rwb_rot_tan, Rwb_d_rot_tan, feet_tan, joint_q_tan are all NULL)";
  else if (io->joint_q_tan && !in->joint_q) own = ": joint_q_tan needs joint_q";
  return check_readonly_batch(who, n, in, own, io->grf_body != nullptr, ": grf_body is required", TANGENT_BLOCK);
}

// the kernel's arguments: the record's scalars and arrays
inline TangentArgs tangent_constants(const qc_tangent_io* io) {
  return TangentArgs{io->grf_body, io->act_tol, (long)io->n_dir, io->x_tan, io->xdot_tan, io->w_tan, io->x_d_tan, io->xdot_d_tan, io->w_d_tan,
                     io->Rwb_rot_tan, io->Rwb_d_rot_tan, io->feet_tan, io->joint_q_tan, io->grf_tan, io->b_tan, io->flags};
}

// workgroups of tangent_kernel for n robots: one wave each, capped (a grid cap of its own)
inline unsigned tangent_blocks(size_t n) { return capped_blocks(n, TANGENT_BLOCK, TANGENT_MAX_BLOCKS); }

// ---------------------------------------------------------------- qc_param_tangent_batch
// The argument check of the forward mode in the parameters: what is wrong with the call itself (message prefix
// "qc_param_tangent_batch:").  One lane per robot, whatever K is: the robots must fit a launch.
inline int check_param_tangent_args(const qc_handle* h, size_t n, const qc_batch_in* in, const qc_param_tangent_io* io) {
  const char* who = "qc_param_tangent_batch";
  if (const int rc = check_io(who, h && in, io, "qc_param_tangent_io", "qc_default_param_tangent"); rc != QC_OK) return rc;
  const char* own = nullptr;
  if (!std::isfinite(io->act_tol) || !(io->act_tol >= 0.0)) own = ": act_tol must be finite and >= 0";
  else if (io->n_dir == 0) own = ": n_dir must be >= 1";
  else if (!io->param_tan) own = ": param_tan is required";
  else if (!io->grf_tan && !io->b_tan) own = ": no output requested (grf_tan and b_tan are both NULL)";
  else if (io->grf_tan_in && !io->grf_tan) own = ": grf_tan_in needs grf_tan";
  else if (io->b_tan_in && !io->b_tan) own = ": b_tan_in needs b_tan";
  return check_readonly_batch(who, n, in, own, io->grf_body != nullptr, ": grf_body is required", PARAM_TANGENT_BLOCK);
}

// the kernel's arguments: the record's scalars and arrays
inline ParamTangentArgs param_tangent_constants(const qc_param_tangent_io* io) {
  return ParamTangentArgs{io->grf_body, io->act_tol, (long)io->n_dir, io->param_tan, io->grf_tan_in, io->b_tan_in, io->grf_tan, io->b_tan, io->flags};
}

// workgroups of param_tangent_kernel for n robots: one wave each, capped (a grid cap of its own)
inline unsigned param_tangent_blocks(size_t n) { return capped_blocks(n, PARAM_TANGENT_BLOCK, PARAM_TANGENT_MAX_BLOCKS); }

// ---------------------------------------------------------------- qc_plant_step_tangent_batch
// What is wrong with the call itself (message prefix "qc_plant_step_tangent_batch:"); the handle's mass and Ib are judged by
// plant_tangent_constants, through the plant's own checks.  One lane per (robot, direction): the pairs, not the robots, must fit a launch.
inline int check_plant_tangent_args(const qc_handle* h, size_t n, const qc_plant_tangent_io* io) {
  const char* who = "qc_plant_step_tangent_batch";
  if (const int rc = check_io(who, h != nullptr, io, "qc_plant_tangent_io", "qc_default_plant_tangent"); rc != QC_OK) return rc;
  const char* own = nullptr;
  if (io->n_dir == 0) own = ": n_dir must be >= 1";
  else if (!io->Rwb_rot_tan && !io->x_tan && !io->xdot_tan && !io->w_tan && !io->grf_tan && !io->foot_world_tan)
    own = ": no tangent given (Rwb_rot_tan, x_tan, xdot_tan, w_tan, grf_tan, foot_world_tan are all NULL)";
  else if (!io->Rwb_rot_next_tan && !io->x_next_tan && !io->xdot_next_tan && !io->w_next_tan && !io->feet_next_tan)
    own = ": no output requested (Rwb_rot_next_tan, x_next_tan, xdot_next_tan, w_next_tan, feet_next_tan are all NULL)";
  if (const int rc = check_plant_io(who, n, io, own, io->grf_body && io->foot_world, ": grf_body and foot_world are required", PLANT_TANGENT_BLOCK); rc != QC_OK || n == 0)
    return rc;
  if (io->n_dir > (size_t)0xFFFFFF * (size_t)PLANT_TANGENT_BLOCK / n) return fail(QC_ERR_INVALID, std::string(who) + ": n * n_dir is beyond one launch");
  return QC_OK;
}

// the kernel's arguments: the body's constants (body_constants, under this entry point's name) and the call's arrays
inline int plant_tangent_constants(double mass, const double* Ib, const qc_plant_tangent_io* io, PlantTangentArgs& a) {
  if (const int rc = body_constants("qc_plant_step_tangent_batch", mass, Ib, io->dt, a); rc != QC_OK) return rc;
  a.Rwb = io->Rwb; a.x = io->x; a.xdot = io->xdot; a.w = io->w; a.grf_body = io->grf_body; a.foot_world = io->foot_world;
  a.n_dir = (long)io->n_dir;
  a.Rwb_rot_tan = io->Rwb_rot_tan; a.x_tan = io->x_tan; a.xdot_tan = io->xdot_tan; a.w_tan = io->w_tan; a.grf_tan = io->grf_tan;
  a.foot_world_tan = io->foot_world_tan;
  a.Rwb_rot_next_tan = io->Rwb_rot_next_tan; a.x_next_tan = io->x_next_tan; a.xdot_next_tan = io->xdot_next_tan; a.w_next_tan = io->w_next_tan;
  a.feet_next_tan = io->feet_next_tan;
  return QC_OK;
}

// workgroups of plant_step_tangent_kernel for n robots and K directions: one wave of pairs each, capped (a grid cap of its own)
inline unsigned plant_tangent_blocks(size_t n, size_t n_dir) { return capped_blocks(n * n_dir, PLANT_TANGENT_BLOCK, PLANT_TANGENT_MAX_BLOCKS); }

// ---------------------------------------------------------------- qc_torque_tangent_batch
// What is wrong with the call itself (message prefix "qc_torque_tangent_batch:").  The kernel reads joint_q and the contact mask of
// `in` and none of the state arrays: they are not asked for.  One lane per (direction, robot, leg): the rows must fit a launch.
inline int check_torque_tangent_args(const qc_handle* h, size_t n, const qc_batch_in* in, const qc_torque_tangent_io* io) {
  const char* who = "qc_torque_tangent_batch";
  if (const int rc = check_io(who, h && in, io, "qc_torque_tangent_io", "qc_default_torque_tangent"); rc != QC_OK) return rc;
  const auto bad = [who](const char* what) { return fail(QC_ERR_INVALID, std::string(who) + what); };
  if (io->n_dir == 0) return bad(": n_dir must be >= 1");
  if (!io->joint_tau_tan) return bad(": no output requested (joint_tau_tan is NULL)");
  if (!io->grf_tan && !io->joint_q_tan) return bad(": no tangent given (grf_tan and joint_q_tan are both NULL)");
  if (!io->grf_body || !io->status) return bad(": joint_tau_tan needs grf_body and status");
  if (n == 0) return QC_OK;
  if (!in->joint_q) return bad(": joint_q is required");
  if (n > (size_t)0xFFFFFF * (size_t)TORQUE_TANGENT_BLOCK / 4 || io->n_dir > (size_t)0xFFFFFF * (size_t)TORQUE_TANGENT_BLOCK / (4 * n))
    return bad(": 4 * n * n_dir is beyond one launch");
  return QC_OK;
}

// the kernel's arguments: joint_q and the contact inputs of `in`, the record's arrays
inline TorqueTangentArgs torque_tangent_constants(const qc_batch_in* in, const qc_torque_tangent_io* io) {
  return TorqueTangentArgs{in->joint_q, in->stance, in->gait_phase, in->gait_duty, io->grf_body, io->status, (long)io->n_dir, io->grf_tan, io->joint_q_tan,
                           io->joint_tau_tan};
}

// workgroups of torque_tangent_kernel for n robots and K directions: one wave of rows each, capped (a grid cap of its own)
inline unsigned torque_tangent_blocks(size_t n, size_t n_dir) { return capped_blocks(4 * n * n_dir, TORQUE_TANGENT_BLOCK, TORQUE_TANGENT_MAX_BLOCKS); }

// ---------------------------------------------------------------- qc_swing_torque_tangent_batch
// What is wrong with the call itself (message prefix "qc_swing_torque_tangent_batch:").  The kernel reads the six arrays of `in` that
// qc_sensitivity_swing_batch reads and the contact mask as it is now; what would plan or advance (swing_state, gait_dt) is refused.
// One lane per (direction, robot, leg): the rows must fit a launch.
inline int check_swing_tangent_args(const qc_handle* h, size_t n, const qc_batch_in* in, const qc_swing_tangent_io* io) {
  const char* who = "qc_swing_torque_tangent_batch";
  if (const int rc = check_io(who, h && in, io, "qc_swing_tangent_io", "qc_default_swing_tangent"); rc != QC_OK) return rc;
  const auto bad = [who](const char* what) { return fail(QC_ERR_INVALID, std::string(who) + what); };
  if (io->n_dir == 0) return bad(": n_dir must be >= 1");
  if (!io->Rwb_rot_tan && !io->x_tan && !io->swing_pos_tan && !io->swing_vel_tan && !io->joint_q_tan && !io->joint_qdot_tan && !io->joint_tau_tan_in)
    return bad(": no tangent given (Rwb_rot_tan, x_tan, swing_pos_tan, swing_vel_tan, joint_q_tan, joint_qdot_tan, joint_tau_tan_in are all NULL)");
  if (!io->joint_tau_tan && !io->flags) return bad(": no output requested (joint_tau_tan and flags are both NULL)");
  if (in->swing_state) return bad(": swing_state must be NULL (the planner's references have no forward mode: give swing_pos and swing_vel)");
  if (in->gait_dt) return bad(": gait_dt must be NULL (the gait clock has no forward mode: the contact mask is read as it is now)");
  if (n == 0) return QC_OK;
  if (!in->Rwb || !in->x || !in->joint_q || !in->joint_qdot || !in->swing_pos || !in->swing_vel)
    return bad(": Rwb, x, joint_q, joint_qdot, swing_pos and swing_vel are required");
  if (n > (size_t)0xFFFFFF * (size_t)SWING_TANGENT_BLOCK / 4 || io->n_dir > (size_t)0xFFFFFF * (size_t)SWING_TANGENT_BLOCK / (4 * n))
    return bad(": 4 * n * n_dir is beyond one launch");
  return QC_OK;
}

// the directions the kernel walks: the flags come from the forward chain alone, so a call without joint_tau_tan walks one
inline size_t swing_tangent_dirs(const qc_swing_tangent_io* io) { return io->joint_tau_tan ? io->n_dir : 1; }

// the kernel's arguments: the six arrays and the contact inputs of `in`, the record's arrays
inline SwingTangentArgs swing_tangent_constants(const qc_batch_in* in, const qc_swing_tangent_io* io) {
  return SwingTangentArgs{in->Rwb, in->x, in->joint_q, in->joint_qdot, in->swing_pos, in->swing_vel, in->stance, in->gait_phase, in->gait_duty,
                          (long)swing_tangent_dirs(io), io->Rwb_rot_tan, io->x_tan, io->swing_pos_tan, io->swing_vel_tan, io->joint_q_tan, io->joint_qdot_tan,
                          io->joint_tau_tan_in, io->joint_tau_tan, io->flags};
}

// workgroups of swing_tangent_kernel for n robots and K directions: one wave of rows each, capped (a grid cap of its own)
inline unsigned swing_tangent_blocks(size_t n, size_t n_dir) { return capped_blocks(4 * n * n_dir, SWING_TANGENT_BLOCK, SWING_TANGENT_MAX_BLOCKS); }

// ---------------------------------------------------------------- qc_leg_plant_step_tangent_batch
// What is wrong with the call itself (message prefix "qc_leg_plant_step_tangent_batch:"); the handle's mass and Ib are judged by
// leg_plant_tangent_constants, through the plant's own checks.  One lane per (robot, direction): the pairs must fit a launch.
inline int check_leg_plant_tangent_args(const qc_handle* h, size_t n, const qc_leg_plant_tangent_io* io) {
  const char* who = "qc_leg_plant_step_tangent_batch";
  if (const int rc = check_io(who, h != nullptr, io, "qc_leg_plant_tangent_io", "qc_default_leg_plant_tangent"); rc != QC_OK) return rc;
  const char* own = nullptr;
  if (io->n_dir == 0) own = ": n_dir must be >= 1";
  else if (!io->Rwb_rot_tan && !io->x_tan && !io->xdot_tan && !io->w_tan && !io->joint_q_tan && !io->joint_qdot_tan && !io->joint_tau_tan)
    own = ": no tangent given (Rwb_rot_tan, x_tan, xdot_tan, w_tan, joint_q_tan, joint_qdot_tan, joint_tau_tan are all NULL)";
  else if (!io->Rwb_rot_next_tan && !io->x_next_tan && !io->xdot_next_tan && !io->w_next_tan && !io->joint_q_next_tan && !io->joint_qdot_next_tan && !io->flags)
    own = ": no output requested (Rwb_rot_next_tan, x_next_tan, xdot_next_tan, w_next_tan, joint_q_next_tan, joint_qdot_next_tan, flags are all NULL)";
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(io->leg_inertia[k]) || !(io->leg_inertia[k] > 0.0))
      own = ": leg_inertia (hip, thigh, calf) must be finite and > 0; qc_default_leg_plant_tangent leaves it at 0, the caller gives the step's";
  if (const int rc = check_plant_io(who, n, io, own, io->joint_q && io->joint_qdot && io->joint_tau, ": joint_q, joint_qdot and joint_tau are required", LEG_PLANT_TANGENT_BLOCK);
      rc != QC_OK || n == 0)
    return rc;
  if (io->n_dir > (size_t)0xFFFFFF * (size_t)LEG_PLANT_TANGENT_BLOCK / n) return fail(QC_ERR_INVALID, std::string(who) + ": n * n_dir is beyond one launch");
  return QC_OK;
}

// the kernel's arguments: what the leg-plant calls share (leg_plant_shared), the tangents and the outputs
inline int leg_plant_tangent_constants(double mass, const double* Ib, const qc_leg_plant_tangent_io* io, LegPlantTangentArgs& a) {
  if (const int rc = leg_plant_shared("qc_leg_plant_step_tangent_batch", mass, Ib, io, a); rc != QC_OK) return rc;
  a.n_dir = (long)io->n_dir;
  a.Rwb_rot_tan = io->Rwb_rot_tan; a.x_tan = io->x_tan; a.xdot_tan = io->xdot_tan; a.w_tan = io->w_tan;
  a.joint_q_tan = io->joint_q_tan; a.joint_qdot_tan = io->joint_qdot_tan; a.joint_tau_tan = io->joint_tau_tan;
  a.Rwb_rot_next_tan = io->Rwb_rot_next_tan; a.x_next_tan = io->x_next_tan; a.xdot_next_tan = io->xdot_next_tan; a.w_next_tan = io->w_next_tan;
  a.joint_q_next_tan = io->joint_q_next_tan; a.joint_qdot_next_tan = io->joint_qdot_next_tan; a.flags = io->flags;
  return QC_OK;
}

// workgroups of leg_plant_step_tangent_kernel for n robots and K directions: one wave of pairs each, capped (a grid cap of its own)
inline unsigned leg_plant_tangent_blocks(size_t n, size_t n_dir) { return capped_blocks(n * n_dir, LEG_PLANT_TANGENT_BLOCK, LEG_PLANT_TANGENT_MAX_BLOCKS); }

// ---------------------------------------------------------------- qc_swing_reference_tangent_batch
// What is wrong with the call itself (message prefix "qc_swing_reference_tangent_batch:").  The contract of `in` is
// qc_swing_reference_adjoint_batch's: what that call refuses about `in` is refused here in its words.  One lane per (direction,
// robot): the pairs must fit a launch.
inline int check_swing_reference_tangent_args(const qc_handle* h, size_t n, const qc_batch_in* in, const qc_swing_reference_tangent_io* io) {
  const char* who = "qc_swing_reference_tangent_batch";
  if (const int rc = check_io(who, h && in, io, "qc_swing_reference_tangent_io", "qc_default_swing_reference_tangent"); rc != QC_OK) return rc;
  const auto bad = [who](const char* what) { return fail(QC_ERR_INVALID, std::string(who) + what); };
  if (io->n_dir == 0) return bad(": n_dir must be >= 1");
  if (!io->Rwb_rot_tan && !io->x_tan && !io->xdot_tan && !io->w_tan && !io->xdot_d_tan && !io->joint_q_tan && !io->p_start_tan && !io->p_final_tan)
    return bad(": no tangent given (Rwb_rot_tan, x_tan, xdot_tan, w_tan, xdot_d_tan, joint_q_tan, p_start_tan, p_final_tan are all NULL)");
  if (!io->swing_pos_tan && !io->swing_vel_tan && !io->p_start_next_tan && !io->p_final_next_tan && !io->flags)
    return bad(": no output requested (swing_pos_tan, swing_vel_tan, p_start_next_tan, p_final_next_tan, flags are all NULL)");
  if (const int rc = check_swing_reference_batch(who, in); rc != QC_OK) return rc;
  if (in->gait_dt) return bad(": gait_dt must be NULL (no clock is advanced here: gait_phase is read as the forward call left it)");
  if (n == 0) return QC_OK;
  if (!io->state_before) return bad(": state_before is required (the swing records from before the forward call)");
  if (!in->Rwb || !in->x || !in->xdot || !in->w || !in->joint_q || !in->gait_phase) return bad(": Rwb, x, xdot, w, joint_q and gait_phase are required");
  if (n > (size_t)0xFFFFFF * (size_t)SWING_REFERENCE_TANGENT_BLOCK || io->n_dir > (size_t)0xFFFFFF * (size_t)SWING_REFERENCE_TANGENT_BLOCK / n)
    return bad(": n * n_dir is beyond one launch");
  return QC_OK;
}

// the directions the kernel walks: the flags come from the held decisions alone, so a call that asks for nothing else walks one
inline size_t swing_reference_tangent_dirs(const qc_swing_reference_tangent_io* io) {
  return (io->swing_pos_tan || io->swing_vel_tan || io->p_start_next_tan || io->p_final_next_tan) ? io->n_dir : 1;
}

// the kernel's arguments: the arrays of `in` the adjoint reads, the record's arrays
inline SwingReferenceTangentArgs swing_reference_tangent_constants(const qc_batch_in* in, const qc_swing_reference_tangent_io* io) {
  return SwingReferenceTangentArgs{in->Rwb, in->x, in->xdot, in->w, in->joint_q, in->gait_phase, in->stance, in->gait_duty,
                                   reinterpret_cast<const SwingState*>(io->state_before), (long)swing_reference_tangent_dirs(io), io->Rwb_rot_tan,
                                   io->x_tan, io->xdot_tan, io->w_tan, io->xdot_d_tan, io->joint_q_tan, io->p_start_tan, io->p_final_tan,
                                   io->swing_pos_tan, io->swing_vel_tan, io->p_start_next_tan, io->p_final_next_tan, io->flags};
}

// workgroups of swing_reference_tangent_kernel for n robots and K directions: one wave of pairs each, capped (a grid cap of its own)
inline unsigned swing_reference_tangent_blocks(size_t n, size_t n_dir) {
  return capped_blocks(n * n_dir, SWING_REFERENCE_TANGENT_BLOCK, SWING_REFERENCE_TANGENT_MAX_BLOCKS);
}

// ---------------------------------------------------------------- qc_commander_step_tangent_batch
// What is wrong with the call itself (message prefix "qc_commander_step_tangent_batch:").  The contract of `in` and `cmd` is
// qc_commander_step_adjoint_batch's: what that call refuses about them is refused here in its words, but for the launch bound - one
// lane per (direction, robot): the pairs must fit a launch.
inline int check_commander_step_tangent_args(const qc_handle* h, size_t n, const qc_batch_in* in, const qc_command_in* cmd,
                                             const qc_commander_step_tangent_io* io) {
  const char* who = "qc_commander_step_tangent_batch";
  if (const int rc = check_io(who, h && in && io, cmd, "qc_command_in", "qc_default_command"); rc != QC_OK) return rc;
  if (const int rc = check_io(who, true, io, "qc_commander_step_tangent_io", "qc_default_commander_step_tangent"); rc != QC_OK) return rc;
  const char* own = nullptr;
  if (io->n_dir == 0) own = ": n_dir must be >= 1";
  else if (!io->twist_tan && !io->Vb_tan && !io->Rwb_rot_tan && !io->x_tan && !io->Rwb_d_rot_prev_tan && !io->x_d_prev_tan && !io->xdot_d_prev_tan &&
           !io->w_d_prev_tan)
    own = ": no tangent given (twist_tan, Vb_tan, Rwb_rot_tan, x_tan, Rwb_d_rot_prev_tan, x_d_prev_tan, xdot_d_prev_tan, w_d_prev_tan are all NULL)";
  else if (!io->Rwb_d_rot_tan && !io->x_d_tan && !io->xdot_d_tan && !io->w_d_tan && !io->Vb_next_tan && !io->flags)
    own = ": no output requested (Rwb_d_rot_tan, x_d_tan, xdot_d_tan, w_d_tan, Vb_next_tan, flags are all NULL)";
  else if (io->twist_tan && !cmd->twist)
    own = ": twist_tan needs qc_command_in.twist";
  if (const int rc = check_commander_step_batch(who, n, in, cmd, own, io->state_before != nullptr,
                                                ": state_before is required (the commander records from before the forward call)");
      rc != QC_OK || n == 0)
    return rc;
  static_assert(COMMAND_TANGENT_BLOCK == SENSITIVITY_BLOCK, "n itself was bounded by the shared check");
  if (io->n_dir > (size_t)0xFFFFFF * (size_t)COMMAND_TANGENT_BLOCK / n)
    return fail(QC_ERR_INVALID, std::string(who) + ": n * n_dir is beyond one launch");
  return QC_OK;
}

// the directions the kernel walks: the flags come from the held decisions alone, so a call that asks for nothing else walks one
inline size_t commander_step_tangent_dirs(const qc_commander_step_tangent_io* io) {
  return (io->Rwb_d_rot_tan || io->x_d_tan || io->xdot_d_tan || io->w_d_tan || io->Vb_next_tan) ? io->n_dir : 1;
}

// the kernel's arguments: what the adjoint reads of `in` and `cmd`, the record's arrays
inline CommanderStepTangentArgs commander_step_tangent_constants(const qc_batch_in* in, const qc_command_in* cmd, const qc_commander_step_tangent_io* io) {
  return CommanderStepTangentArgs{in->Rwb, in->x, cmd->twist, cmd->fresh, reinterpret_cast<const CmdState*>(io->state_before), cmd->stand_height,
                                  cmd->stand_tol, cmd->cmd_dt, (long)commander_step_tangent_dirs(io), io->twist_tan, io->Vb_tan, io->Rwb_rot_tan,
                                  io->x_tan, io->Rwb_d_rot_prev_tan, io->x_d_prev_tan, io->xdot_d_prev_tan, io->w_d_prev_tan, io->Rwb_d_rot_tan,
                                  io->x_d_tan, io->xdot_d_tan, io->w_d_tan, io->Vb_next_tan, io->flags};
}

// workgroups of the two kernels of qc_command_tangent.hpp for n robots and K directions: one wave of pairs each, capped
inline unsigned command_tangent_blocks(size_t n, size_t n_dir) { return capped_blocks(n * n_dir, COMMAND_TANGENT_BLOCK, COMMAND_TANGENT_MAX_BLOCKS); }

// ---------------------------------------------------------------- qc_com_reference_tangent_batch
// What is wrong with the call itself (message prefix "qc_com_reference_tangent_batch:"): qc_com_reference_adjoint_batch's refusals
// about `in`, the mode, the gain and the schedule in its words, the tangent's own about its arrays in their place, and the launch bound
// on the pairs.
inline int check_com_reference_tangent_args(const qc_handle* h, size_t n, const qc_batch_in* in, const qc_com_reference_tangent_io* io) {
  const char* who = "qc_com_reference_tangent_batch";
  if (const int rc = check_io(who, h && in, io, "qc_com_reference_tangent_io", "qc_default_com_reference_tangent"); rc != QC_OK) return rc;
  const char* own = check_com_mode(io->mode, io->gain);
  if (own) {
  } else if (io->n_dir == 0) own = ": n_dir must be >= 1";
  else if (!io->x_d_in_tan && !io->feet_tan && !io->joint_q_tan && !io->Rwb_rot_tan && !io->x_tan && !io->phase_tan && !io->schedule_tan)
    own = ": no tangent given (x_d_in_tan, feet_tan, joint_q_tan, Rwb_rot_tan, x_tan, phase_tan, schedule_tan are all NULL)";
  else if (!io->x_d_out_tan && !io->com_xy_tan && !io->flags)
    own = ": no output requested (x_d_out_tan, com_xy_tan, flags are all NULL)";
  else if (io->joint_q_tan && !in->joint_q)
    own = ": joint_q_tan needs in->joint_q";
  if (const int rc = check_com_reference_batch(who, n, in, own, io->schedule); rc != QC_OK || n == 0) return rc;
  static_assert(COMMAND_TANGENT_BLOCK == SENSITIVITY_BLOCK, "n itself was bounded by the shared check");
  if (io->n_dir > (size_t)0xFFFFFF * (size_t)COMMAND_TANGENT_BLOCK / n)
    return fail(QC_ERR_INVALID, std::string(who) + ": n * n_dir is beyond one launch");
  return QC_OK;
}

inline size_t com_reference_tangent_dirs(const qc_com_reference_tangent_io* io) { return (io->x_d_out_tan || io->com_xy_tan) ? io->n_dir : 1; }

// the kernel's arguments: SupportIn as the forward call packs it (world mode), the tangents
inline ComReferenceTangentArgs com_reference_tangent_constants(const qc_batch_in* in, const qc_com_reference_tangent_io* io) {
  ComReferenceTangentArgs a{};
  static_cast<SupportIn&>(a) = support_in(in, io->schedule, io->schedule_shared, true);
  a.mode = io->mode;
  a.gain = io->gain;
  a.n_dir = (long)com_reference_tangent_dirs(io);
  a.x_d_in_tan = io->x_d_in_tan;
  a.feet_tan = io->feet_tan;
  a.joint_q_tan = io->joint_q_tan;
  a.Rwb_rot_tan = io->Rwb_rot_tan;
  a.x_tan = io->x_tan;
  a.phase_tan = io->phase_tan;
  a.schedule_tan = io->schedule_tan;
  a.x_d_out_tan = io->x_d_out_tan;
  a.com_xy_tan = io->com_xy_tan;
  a.flags = io->flags;
  return a;
}

// ---------------------------------------------------------------- qc_plant_step_model_batch, qc_leg_plant_step_model_batch, qc_plant_step_model_adjoint_batch
// What the three calls of include/qc_plant_model.h refuse about the model, after everything the base call refuses about its record:
// no model, a model of another revision, and - for n > 0: n = 0 reads no array, of the model's either - a model that changes nothing
// (`base`: the call to make instead).
inline int check_plant_model(const char* who, const char* base, size_t n, const qc_plant_model* m) {
  if (!m) return fail(QC_ERR_INVALID, std::string(who) + ": null argument");
  if (const int rc = check_struct_size(who, "qc_plant_model", "qc_default_plant_model", m->struct_size, sizeof(qc_plant_model)); rc != QC_OK) return rc;
  if (n > 0 && !m->mass && !m->Ib && !m->wrench_world)
    return fail(QC_ERR_INVALID, std::string(who) + ": the model gives neither mass, Ib nor wrench_world - call " + base);
  return QC_OK;
}

inline int check_plant_model_args(const qc_handle* h, size_t n, const qc_plant_io* io, const qc_plant_model* m) {
  const char* who = "qc_plant_step_model_batch";
  if (const int rc = check_io(who, h != nullptr, io, "qc_plant_io", "qc_default_plant"); rc != QC_OK) return rc;
  if (const int rc = check_plant_io(who, n, io, nullptr, io->grf_body && io->foot_world, ": grf_body and foot_world are required", PLANT_BLOCK); rc != QC_OK) return rc;
  return check_plant_model(who, "qc_plant_step_batch", n, m);
}

inline int check_leg_plant_model_args(const qc_handle* h, size_t n, const qc_leg_plant_io* io, const qc_plant_model* m) {
  const char* who = "qc_leg_plant_step_model_batch";
  if (const int rc = check_io(who, h != nullptr, io, "qc_leg_plant_io", "qc_default_leg_plant"); rc != QC_OK) return rc;
  const char* own = nullptr;
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(io->leg_inertia[k]) || !(io->leg_inertia[k] > 0.0))
      own = ": leg_inertia (hip, thigh, calf) must be finite and > 0; qc_default_leg_plant leaves it at 0, the caller gives it";
  if (const int rc = check_plant_io(who, n, io, own, io->joint_q && io->joint_qdot && io->joint_tau, ": joint_q, joint_qdot and joint_tau are required", LEG_PLANT_BLOCK);
      rc != QC_OK)
    return rc;
  return check_plant_model(who, "qc_leg_plant_step_batch", n, m);
}

// (`bar` may be NULL; an output of either record will do)
inline int check_plant_model_adjoint_args(const qc_handle* h, size_t n, const qc_plant_adjoint_io* io, const qc_plant_model* m, const qc_plant_model_bar* bar) {
  const char* who = "qc_plant_step_model_adjoint_batch";
  if (const int rc = check_io(who, h != nullptr, io, "qc_plant_adjoint_io", "qc_default_plant_adjoint"); rc != QC_OK) return rc;
  if (bar)
    if (const int rc = check_struct_size(who, "qc_plant_model_bar", "qc_default_plant_model_bar", bar->struct_size, sizeof(qc_plant_model_bar)); rc != QC_OK) return rc;
  const char* own = nullptr;
  if (!io->Rwb_next_bar && !io->x_next_bar && !io->xdot_next_bar && !io->w_next_bar && !io->feet_next_bar)
    own = ": no input cotangent given (Rwb_next_bar, x_next_bar, xdot_next_bar, w_next_bar, feet_next_bar are all NULL)";
  else if (!io->Rwb_bar && !io->x_bar && !io->xdot_bar && !io->w_bar && !io->grf_bar && !io->foot_world_bar &&
           !(bar && (bar->wrench_bar || bar->mass_bar || bar->Ib_bar)))
    own = ": no output requested (Rwb_bar, x_bar, xdot_bar, w_bar, grf_bar, foot_world_bar and the model's wrench_bar, mass_bar, Ib_bar are all NULL)";
  if (const int rc = check_plant_io(who, n, io, own, io->grf_body && io->foot_world, ": grf_body and foot_world are required", PLANT_BLOCK); rc != QC_OK) return rc;
  return check_plant_model(who, "qc_plant_step_adjoint_batch", n, m);
}

// The body's constants under a model: what the model supplies per robot is not asked of the handle (a placeholder - 1, the identity -
// travels in its place and is never read by that instantiation); the rest is judged as body_constants judges it.
inline int model_body_constants(const char* who, double mass, const double* Ib, double dt, const qc_plant_model* m, BodyConst& b) {
  if (!m->mass && (!std::isfinite(mass) || !(mass > 0.0))) return fail(QC_ERR_INVALID, std::string(who) + ": the handle's mass is not finite and > 0");
  b.mass = m->mass ? 1.0 : mass;
  if (m->Ib) {
    for (int k = 0; k < 9; k++) b.Ib[k] = b.Ib_inv[k] = (k % 4 == 0) ? 1.0 : 0.0;
  } else {
    if (const int rc = plant_inertia_inverse(Ib, b.Ib_inv, who); rc != QC_OK) return rc;
    std::memcpy(b.Ib, Ib, sizeof(b.Ib));
  }
  b.g = PLANT_G;
  b.dt = dt;
  return QC_OK;
}

inline PlantModelArgs plant_model_args(const qc_plant_model* m) { return PlantModelArgs{m->mass, m->Ib, m->wrench_world, m->flags}; }
inline PlantModelBarArgs plant_model_bar_args(const qc_plant_model_bar* bar) {
  return bar ? PlantModelBarArgs{bar->wrench_bar, bar->mass_bar, bar->Ib_bar, bar->flags} : PlantModelBarArgs{nullptr, nullptr, nullptr, nullptr};
}
// which of the eight instantiations <MASS, IB, WRENCH> a model selects: bit 0 mass, bit 1 Ib, bit 2 wrench_world (0 is refused)
inline int plant_model_variant(const qc_plant_model* m) { return (m->mass ? 1 : 0) | (m->Ib ? 2 : 0) | (m->wrench_world ? 4 : 0); }

inline int plant_model_constants(double mass, const double* Ib, const qc_plant_io* io, const qc_plant_model* m, PlantArgs& a) {
  if (const int rc = model_body_constants("qc_plant_step_model_batch", mass, Ib, io->dt, m, a); rc != QC_OK) return rc;
  a.Rwb = io->Rwb; a.x = io->x; a.xdot = io->xdot; a.w = io->w; a.grf_body = io->grf_body; a.foot_world = io->foot_world; a.feet = io->feet;
  return QC_OK;
}

inline int leg_plant_model_constants(double mass, const double* Ib, const qc_leg_plant_io* io, const qc_plant_model* m, LegPlantArgs& a) {
  if (const int rc = model_body_constants("qc_leg_plant_step_model_batch", mass, Ib, io->dt, m, a); rc != QC_OK) return rc;
  for (int k = 0; k < 3; k++) a.leg_inertia[k] = io->leg_inertia[k];
  a.Rwb = io->Rwb; a.x = io->x; a.xdot = io->xdot; a.w = io->w; a.joint_q = io->joint_q; a.joint_qdot = io->joint_qdot; a.joint_tau = io->joint_tau;
  a.stance = io->stance; a.gait_phase = io->gait_phase; a.gait_duty = io->gait_duty; a.cmd_state = reinterpret_cast<const CmdState*>(io->cmd_state);
  a.foot_world = io->foot_world; a.flags = io->flags;
  return QC_OK;
}

inline int plant_model_adjoint_constants(double mass, const double* Ib, const qc_plant_adjoint_io* io, const qc_plant_model* m, PlantAdjointArgs& a) {
  if (const int rc = model_body_constants("qc_plant_step_model_adjoint_batch", mass, Ib, io->dt, m, a); rc != QC_OK) return rc;
  a.Rwb = io->Rwb; a.x = io->x; a.xdot = io->xdot; a.w = io->w; a.grf_body = io->grf_body; a.foot_world = io->foot_world;
  a.Rwb_next_bar = io->Rwb_next_bar; a.x_next_bar = io->x_next_bar; a.xdot_next_bar = io->xdot_next_bar; a.w_next_bar = io->w_next_bar;
  a.feet_next_bar = io->feet_next_bar;
  a.Rwb_bar = io->Rwb_bar; a.x_bar = io->x_bar; a.xdot_bar = io->xdot_bar; a.w_bar = io->w_bar; a.grf_bar = io->grf_bar; a.foot_world_bar = io->foot_world_bar;
  return QC_OK;
}

}  // namespace qc
